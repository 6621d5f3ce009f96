// Point3D's geometry on the device, each piece stated once: Trianglate2 (SfM/src/structure.cc:211-265), Reprojection
// (:267-300) and the angle gate of SufficientTriangulationAngle (:325-355).  tri.hip, seed.hip, newpoints.hip, adjust.hip and
// gpsreg.hip build their kernels from these functions; tests/point3d_ref.h is the host's independent restatement.
//
// This header carries no `#pragma clang fp contract`: it takes the state of the file that includes it.  seed.hip,
// newpoints.hip, adjust.hip and gpsreg.hip include it behind `#pragma clang fp contract(off)` and use + - * / sqrt only, so the
// C++ references of tests/, built with -ffp-contract=off, agree with them bit for bit.  tri.hip includes it contracted, as the
// compiler's default has it, and agrees with the oracle to 1e-9.
#pragma once

struct View { const double *R, *t, *c, *fk; double x, y; };   // one observation: its camera's R, t, centre, (f, k1, k2); the image point

// ---- Trianglate2 ----
// the unit ray through the image point (x, y) in world coordinates: R^T (x, y, f), normalised (:224-236)
__device__ __forceinline__ void p3d_ray(const double* R, double f, double x, double y, double* d) {
  d[0] = R[0] * x + R[3] * y + R[6] * f; d[1] = R[1] * x + R[4] * y + R[7] * f; d[2] = R[2] * x + R[5] * y + R[8] * f;
  const double n = sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
  d[0] /= n; d[1] /= n; d[2] /= n;
}

// one ray d from the centre o into the homogeneous 4 x 4 normal equations: A += I - d d^T, bv += (I - d d^T) o (:237-245)
__device__ __forceinline__ void p3d_accumulate(const double* d, const double* o, double* A, double* bv) {
  const double dh[4] = {d[0], d[1], d[2], 0.0};
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

// Eigen::LLT<Matrix4d> of A, failing on a non-positive pivot (:247-251), the two triangular solves and the division by the
// fourth coordinate (:252-258).  X is written only when the factorisation holds.
__device__ __forceinline__ bool p3d_solve(const double* A, const double* bv, double* X) {
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
  return true;
}

// ---- Reprojection ----
// the point in the camera's frame; the depth test on pc[2] belongs to the caller
__device__ __forceinline__ void p3d_camera_point(const double* R, const double* t, const double* X, double* pc) {
  pc[0] = R[0] * X[0] + R[1] * X[1] + R[2] * X[2] + t[0];
  pc[1] = R[3] * X[0] + R[4] * X[1] + R[5] * X[2] + t[1];
  pc[2] = R[6] * X[0] + R[7] * X[1] + R[8] * X[2] + t[2];
}

// its image with the radial distortion (k1, k2) = fk[1], fk[2], relative to the principal point (:286-292)
__device__ __forceinline__ void p3d_project(const double* fk, const double* pc, double* uv) {
  const double x = pc[0] / pc[2], y = pc[1] / pc[2];
  const double r2 = x * x + y * y;
  const double distortion = 1.0 + r2 * (fk[1] + fk[2] * r2);
  uv[0] = fk[0] * distortion * x; uv[1] = fk[0] * distortion * y;
}

// the squared reprojection error of X against the image point (x, y); -1.0 when the depth is negative (strict: a NaN walks on)
__device__ __forceinline__ double p3d_row_error(const double* R, const double* t, const double* fk, const double* X, double x, double y) {
  double pc[3], uv[2];
  p3d_camera_point(R, t, X, pc);
  if (pc[2] < 0) return -1.0;
  p3d_project(fk, pc, uv);
  const double du = uv[0] - x, dv = uv[1] - y;
  return du * du + dv * dv;
}

// the mean of the row terms term(i) over the rows i in [b, e) that keep(i) admits, summed in row order; a negative term ends the
// walk and makes the error the constant 100000 (:280-284)
template <class Term, class Keep>
__device__ __forceinline__ double p3d_ordered_mse(int b, int e, Term term, Keep keep) {
  double m = 0.0;
  int count = 0;
  for (int i = b; i < e; i++) {
    if (!keep(i)) continue;
    const double er = term(i);
    if (er < 0.0) return 100000.0;
    m += er;
    count++;
  }
  return m / count;
}
template <class Term>
__device__ __forceinline__ double p3d_ordered_mse(int b, int e, Term term) {
  return p3d_ordered_mse(b, e, term, [](int) { return true; });
}

// ---- SufficientTriangulationAngle ----
// the unit direction from the camera centre c to X
__device__ __forceinline__ void p3d_direction(const double* c, const double* X, double* a) {
  a[0] = X[0] - c[0]; a[1] = X[1] - c[1]; a[2] = X[2] - c[2];
  const double n = sqrt(a[0] * a[0] + a[1] * a[1] + a[2] * a[2]);
  a[0] /= n; a[1] /= n; a[2] /= n;
}

// a pair of unit directions that opens wide enough
__device__ __forceinline__ bool p3d_pair_wide(const double* a, const double* d, double cos_min) {
  return a[0] * d[0] + a[1] * d[1] + a[2] * d[2] < cos_min;
}

// the verdict of Trianglate2 (:259-264)
__device__ __forceinline__ bool p3d_accepted(double mse, double th_error, bool wide) { return !(sqrt(mse) > th_error || !wide); }

// ---- Trianglate2 for two views (seed.hip, newpoints.hip) ----
// X and *mse_out are written only when the LLT holds
__device__ __forceinline__ bool tri_two_views(const View* V, double th_error, double cos_min, double* X, double* mse_out) {
  double A[16], bv[4] = {0, 0, 0, 0};
#pragma unroll
  for (int k = 0; k < 16; k++) A[k] = 0.0;
#pragma unroll
  for (int i = 0; i < 2; i++) {
    double d[3];
    p3d_ray(V[i].R, V[i].fk[0], V[i].x, V[i].y, d);
    p3d_accumulate(d, V[i].c, A, bv);
  }
  if (!p3d_solve(A, bv, X)) return false;
  const double m = p3d_ordered_mse(0, 2, [&](int i) { return p3d_row_error(V[i].R, V[i].t, V[i].fk, X, V[i].x, V[i].y); });
  *mse_out = m;
  double a[3], d[3];
  p3d_direction(V[0].c, X, a);
  p3d_direction(V[1].c, X, d);
  return p3d_accepted(m, th_error, p3d_pair_wide(a, d, cos_min));
}
