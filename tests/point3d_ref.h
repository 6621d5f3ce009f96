// Sequential restatement of Point3D::Trianglate2 (SfM/src/structure.cc:211-265), Point3D::Reprojection (:267-300) and
// Point3D::SufficientTriangulationAngle (:325-355) on a list of observations, shared by tests/seed_ref.cpp and
// tests/newpoints_ref.cpp.  It is the tests' own statement: it includes nothing of metricsfm_amd/csrc, so that the bit-for-bit
// tests compare two texts.  Built with g++ -O2 -ffp-contract=off: + - * / sqrt only.
#pragma once
#include <cmath>
#include <vector>

namespace {

struct Cam { double R[9], t[3], c[3], fk[3]; };
struct Obs { const Cam* cam; double x, y; };

// Point3D::Reprojection, structure.cc:267-300
double reprojection(const std::vector<Obs>& obs, const double* X) {
  double mse = 0.0;
  int count = 0;
  for (const Obs& o : obs) {
    const double* R = o.cam->R;
    const double* tt = o.cam->t;
    const double* fk = o.cam->fk;
    const double pc0 = R[0] * X[0] + R[1] * X[1] + R[2] * X[2] + tt[0];
    const double pc1 = R[3] * X[0] + R[4] * X[1] + R[5] * X[2] + tt[1];
    const double pc2 = R[6] * X[0] + R[7] * X[1] + R[8] * X[2] + tt[2];
    if (pc2 < 0) return 100000.0;
    const double x = pc0 / pc2, y = pc1 / pc2;
    const double r2 = x * x + y * y;
    const double distortion = 1.0 + r2 * (fk[1] + fk[2] * r2);
    const double u = fk[0] * distortion * x, v = fk[0] * distortion * y;
    const double du = u - o.x, dv = v - o.y;
    mse += du * du + dv * dv;
    count++;
  }
  return mse / count;
}

// Point3D::SufficientTriangulationAngle, structure.cc:325-355; *cos_out = the cosine of the last pair of rays it looked at
bool sufficient_angle(const std::vector<Obs>& obs, const double* X, double cos_min, double* cos_out) {
  for (size_t i = 0; i + 1 < obs.size(); i++) {
    const double* ci = obs[i].cam->c;
    double a[3] = {X[0] - ci[0], X[1] - ci[1], X[2] - ci[2]};
    const double na = std::sqrt(a[0] * a[0] + a[1] * a[1] + a[2] * a[2]);
    a[0] /= na; a[1] /= na; a[2] /= na;
    for (size_t j = i + 1; j < obs.size(); j++) {
      const double* cj = obs[j].cam->c;
      double d[3] = {X[0] - cj[0], X[1] - cj[1], X[2] - cj[2]};
      const double nd = std::sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
      d[0] /= nd; d[1] /= nd; d[2] /= nd;
      const double cs = a[0] * d[0] + a[1] * d[1] + a[2] * d[2];
      *cos_out = cs;
      if (cs < cos_min) return true;
    }
  }
  return false;
}

// Point3D::Trianglate2, structure.cc:211-265: sum of (I - d d^T) over the rays in homogeneous 4 x 4 form, Eigen::LLT
// returns 0: LLT failed (X, mse untouched), 1: solved but rejected, 2: accepted
int trianglate2(const std::vector<Obs>& obs, double th_error, double cos_min, double* X, double* mse, double* cos_out) {
  double A[16], bv[4] = {0, 0, 0, 0};
  for (int k = 0; k < 16; k++) A[k] = 0.0;
  for (const Obs& ob : obs) {
    const double* R = ob.cam->R;
    const double* o = ob.cam->c;
    const double f = ob.cam->fk[0];
    double dw[3] = {R[0] * ob.x + R[3] * ob.y + R[6] * f, R[1] * ob.x + R[4] * ob.y + R[7] * f, R[2] * ob.x + R[5] * ob.y + R[8] * f};
    const double n = std::sqrt(dw[0] * dw[0] + dw[1] * dw[1] + dw[2] * dw[2]);
    dw[0] /= n; dw[1] /= n; dw[2] /= n;
    const double dh[4] = {dw[0], dw[1], dw[2], 0.0};
    const double oh[4] = {o[0], o[1], o[2], 1.0};
    for (int r = 0; r < 4; r++) {
      double acc = 0.0;
      for (int q = 0; q < 4; q++) {
        const double at = (r == q ? 1.0 : 0.0) - dh[r] * dh[q];
        A[r * 4 + q] += at;
        acc += at * oh[q];
      }
      bv[r] += acc;
    }
  }
  double L[16];
  for (int k = 0; k < 16; k++) L[k] = 0.0;
  bool pd = true;
  for (int j = 0; j < 4; j++) {
    double d = A[j * 4 + j];
    for (int k = 0; k < j; k++) d -= L[j * 4 + k] * L[j * 4 + k];
    if (!(d > 0.0)) pd = false;
    L[j * 4 + j] = std::sqrt(d);
    for (int i = j + 1; i < 4; i++) {
      double s = A[i * 4 + j];
      for (int k = 0; k < j; k++) s -= L[i * 4 + k] * L[j * 4 + k];
      L[i * 4 + j] = s / L[j * 4 + j];
    }
  }
  if (!pd) return 0;
  double y[4], x[4];
  for (int i = 0; i < 4; i++) {
    double s = bv[i];
    for (int k = 0; k < i; k++) s -= L[i * 4 + k] * y[k];
    y[i] = s / L[i * 4 + i];
  }
  for (int i = 3; i >= 0; i--) {
    double s = y[i];
    for (int k = i + 1; k < 4; k++) s -= L[k * 4 + i] * x[k];
    x[i] = s / L[i * 4 + i];
  }
  X[0] = x[0] / x[3]; X[1] = x[1] / x[3]; X[2] = x[2] / x[3];
  *mse = reprojection(obs, X);
  const bool angle_ok = sufficient_angle(obs, X, cos_min, cos_out);
  return !(std::sqrt(*mse) > th_error || !angle_ok) ? 2 : 1;
}

}  // namespace
