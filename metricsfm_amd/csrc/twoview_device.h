// Two-view Point3D::Trianglate2 on the device, shared by seed.hip and newpoints.hip.  Include it behind
//   #pragma clang fp contract(off)
// in a file that uses + - * / sqrt only: tests/seed_ref.cpp and tests/newpoints_ref.cpp, built with -ffp-contract=off, agree
// with it bit for bit (tri.hip is contracted and agrees to 1e-9).
#pragma once

struct View { const double *R, *t, *c, *fk; double x, y; };

// Point3D::Trianglate2 for two views: tri_midpoint_track of tri.hip with the loop over the observations written out
__device__ static inline bool tri_two_views(const View* V, double th_error, double cos_min, double* X, double* mse_out) {
  double A[16], bv[4] = {0, 0, 0, 0};
#pragma unroll
  for (int k = 0; k < 16; k++) A[k] = 0.0;
#pragma unroll
  for (int i = 0; i < 2; i++) {
    const double* R = V[i].R;
    const double* o = V[i].c;
    const double f = V[i].fk[0];
    const double d0 = V[i].x, d1 = V[i].y;
    double dw[3] = {R[0] * d0 + R[3] * d1 + R[6] * f, R[1] * d0 + R[4] * d1 + R[7] * f, R[2] * d0 + R[5] * d1 + R[8] * f};
    const double nrm = sqrt(dw[0] * dw[0] + dw[1] * dw[1] + dw[2] * dw[2]);
    dw[0] /= nrm; dw[1] /= nrm; dw[2] /= nrm;
    const double dh[4] = {dw[0], dw[1], dw[2], 0.0};
    const double oh[4] = {o[0], o[1], o[2], 1.0};
#pragma unroll
    for (int r = 0; r < 4; r++) {
      double acc = 0.0;
#pragma unroll
      for (int q = 0; q < 4; q++) {
        const double at = (r == q ? 1.0 : 0.0) - dh[r] * dh[q];
        A[r * 4 + q] += at;
        acc += at * oh[q];
      }
      bv[r] += acc;
    }
  }
  // Eigen::LLT<Matrix4d>: fail on a non-positive pivot (structure.cc:247-251)
  double L[16];
#pragma unroll
  for (int k = 0; k < 16; k++) L[k] = 0.0;
  bool pd = true;
#pragma unroll
  for (int j = 0; j < 4; j++) {
    double d = A[j * 4 + j];
#pragma unroll
    for (int k = 0; k < j; k++) d -= L[j * 4 + k] * L[j * 4 + k];
    if (!(d > 0.0)) pd = false;
    L[j * 4 + j] = sqrt(d);
#pragma unroll
    for (int i = j + 1; i < 4; i++) {
      double s = A[i * 4 + j];
#pragma unroll
      for (int k = 0; k < j; k++) s -= L[i * 4 + k] * L[j * 4 + k];
      L[i * 4 + j] = s / L[j * 4 + j];
    }
  }
  if (!pd) return false;
  double y[4], x[4];
#pragma unroll
  for (int i = 0; i < 4; i++) {
    double s = bv[i];
#pragma unroll
    for (int k = 0; k < i; k++) s -= L[i * 4 + k] * y[k];
    y[i] = s / L[i * 4 + i];
  }
#pragma unroll
  for (int i = 3; i >= 0; i--) {
    double s = y[i];
#pragma unroll
    for (int k = i + 1; k < 4; k++) s -= L[k * 4 + i] * x[k];
    x[i] = s / L[i * 4 + i];
  }
  X[0] = x[0] / x[3]; X[1] = x[1] / x[3]; X[2] = x[2] / x[3];
  // structure.cc:267-300
  double m = 0.0;
  bool behind = false;
#pragma unroll
  for (int i = 0; i < 2; i++) {
    if (behind) break;
    const double* R = V[i].R;
    const double* tt = V[i].t;
    const double* fk = V[i].fk;
    const double pc0 = R[0] * X[0] + R[1] * X[1] + R[2] * X[2] + tt[0];
    const double pc1 = R[3] * X[0] + R[4] * X[1] + R[5] * X[2] + tt[1];
    const double pc2 = R[6] * X[0] + R[7] * X[1] + R[8] * X[2] + tt[2];
    if (pc2 < 0) { behind = true; break; }
    const double u0 = pc0 / pc2, v0 = pc1 / pc2;
    const double r2 = u0 * u0 + v0 * v0;
    const double distortion = 1.0 + r2 * (fk[1] + fk[2] * r2);
    const double u = fk[0] * distortion * u0, v = fk[0] * distortion * v0;
    const double du = u - V[i].x, dv = v - V[i].y;
    m += du * du + dv * dv;
  }
  m = behind ? 100000.0 : m / 2;
  *mse_out = m;
  // structure.cc:325-355
  double a[3] = {X[0] - V[0].c[0], X[1] - V[0].c[1], X[2] - V[0].c[2]};
  const double na = sqrt(a[0] * a[0] + a[1] * a[1] + a[2] * a[2]);
  a[0] /= na; a[1] /= na; a[2] /= na;
  double d[3] = {X[0] - V[1].c[0], X[1] - V[1].c[1], X[2] - V[1].c[2]};
  const double nd = sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
  d[0] /= nd; d[1] /= nd; d[2] /= nd;
  const bool angle_ok = a[0] * d[0] + a[1] * d[1] + a[2] * d[2] < cos_min;
  return !(sqrt(m) > th_error || !angle_ok);
}
