// Sequential restatement, over plain arrays, of the four steps SLAMGPS::Run takes between Triangulation and the end of
// FullBundleAdjustment beside the adjustment (SfM/src/slam_gps.cc:98-119): one point, one camera, one row at a time, as the
// reference walks them.  Built with g++ -O2 -ffp-contract=off and loaded with ctypes (tests/gpsreg_ref.py): the device steps use
// + - * / sqrt only, so the library's gpsreg.hip must agree bit for bit; the orientation also calls acos, tan and atan2 of the
// same C library.  tests/test_gpsreg_ref.py pins this file against numpy.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <limits>
#include <vector>

namespace {

typedef double M3[9];   // row-major

// ---- the 3x3 SVD: Eigen 3's two-sided JacobiSVD restated from its published algorithm (no QR step for a square input) ----
struct Jacobi { double c, s; };   // the rotation [c s; -s c]

// rows p and q of M become c x + s y and -s x + c y
void apply_left(M3 M, int p, int q, Jacobi j) {
  for (int k = 0; k < 3; k++) {
    const double x = M[3 * p + k], y = M[3 * q + k];
    M[3 * p + k] = j.c * x + j.s * y;
    M[3 * q + k] = -j.s * x + j.c * y;
  }
}
// columns p and q of M become c x + s y and -s x + c y
void apply_right_t(M3 M, int p, int q, Jacobi j) {
  for (int k = 0; k < 3; k++) {
    const double x = M[3 * k + p], y = M[3 * k + q];
    M[3 * k + p] = j.c * x + j.s * y;
    M[3 * k + q] = -j.s * x + j.c * y;
  }
}

// the 2x2 real Jacobi SVD of the pivot block: left and right rotations that make it diagonal
void jacobi_2x2(const M3 W, int p, int q, Jacobi* left, Jacobi* right) {
  const double tiny = std::numeric_limits<double>::min();
  double m00 = W[3 * p + p], m01 = W[3 * p + q], m10 = W[3 * q + p], m11 = W[3 * q + q];
  Jacobi rot1;
  const double t = m00 + m11, d = m10 - m01;
  if (std::fabs(d) < tiny) {
    rot1.s = 0.0; rot1.c = 1.0;
  } else {
    const double u = t / d, tmp = std::sqrt(1.0 + u * u);
    rot1.s = 1.0 / tmp; rot1.c = u / tmp;
  }
  const double n00 = rot1.c * m00 + rot1.s * m10, n01 = rot1.c * m01 + rot1.s * m11, n11 = -rot1.s * m01 + rot1.c * m11;
  m00 = n00; m01 = n01; m11 = n11;   // (the block is symmetric now)
  const double deno = 2.0 * std::fabs(m01);
  if (deno < tiny) {
    right->c = 1.0; right->s = 0.0;
  } else {
    const double tau = (m00 - m11) / deno, w = std::sqrt(tau * tau + 1.0);
    const double tt = tau > 0.0 ? 1.0 / (tau + w) : 1.0 / (tau - w);
    const double sign_t = tt > 0.0 ? 1.0 : -1.0, n = 1.0 / std::sqrt(tt * tt + 1.0);
    right->s = -sign_t * (m01 / std::fabs(m01)) * std::fabs(tt) * n;
    right->c = n;
  }
  left->c = rot1.c * right->c + rot1.s * right->s;   // rot1 * right^T
  left->s = rot1.s * right->c - rot1.c * right->s;
}

void svd3(const M3 A, M3 U, double S[3], M3 V) {
  const double tiny = std::numeric_limits<double>::min(), precision = 2.0 * std::numeric_limits<double>::epsilon();
  double scale = 0.0;
  for (int k = 0; k < 9; k++) scale = std::max(scale, std::fabs(A[k]));
  if (scale == 0.0) scale = 1.0;
  M3 W;
  for (int k = 0; k < 9; k++) { W[k] = A[k] / scale; U[k] = V[k] = (k % 4 == 0) ? 1.0 : 0.0; }
  double max_diag = std::max(std::fabs(W[0]), std::max(std::fabs(W[4]), std::fabs(W[8])));
  bool finished = false;
  while (!finished) {
    finished = true;
    for (int p = 1; p < 3; p++)
      for (int q = 0; q < p; q++) {
        const double threshold = std::max(tiny, precision * max_diag);
        if (std::fabs(W[3 * p + q]) > threshold || std::fabs(W[3 * q + p]) > threshold) {
          finished = false;
          Jacobi jl, jr;
          jacobi_2x2(W, p, q, &jl, &jr);
          apply_left(W, p, q, jl);
          apply_right_t(U, p, q, jl);                   // U = U jl^T
          const Jacobi jrt = {jr.c, -jr.s};
          apply_right_t(W, p, q, jrt);                  // W = W jr
          apply_right_t(V, p, q, jrt);                  // V = V jr
          max_diag = std::max(max_diag, std::max(std::fabs(W[3 * p + p]), std::fabs(W[3 * q + q])));
        }
      }
  }
  for (int i = 0; i < 3; i++) {
    const double a = W[4 * i];
    S[i] = std::fabs(a);
    if (a < 0.0) for (int k = 0; k < 3; k++) U[3 * k + i] = -U[3 * k + i];
  }
  for (int i = 0; i < 3; i++) S[i] *= scale;
  for (int i = 0; i < 3; i++) {   // descending, the swaps applied to the columns of U and V
    int pos = i;
    for (int k = i + 1; k < 3; k++) if (S[k] > S[pos]) pos = k;
    if (S[pos] == 0.0) break;
    if (pos != i) {
      std::swap(S[i], S[pos]);
      for (int k = 0; k < 3; k++) { std::swap(U[3 * k + i], U[3 * k + pos]); std::swap(V[3 * k + i], V[3 * k + pos]); }
    }
  }
}

void mat_mat(const M3 A, const M3 B, M3 C) {
  for (int r = 0; r < 3; r++)
    for (int c = 0; c < 3; c++) C[3 * r + c] = A[3 * r] * B[c] + A[3 * r + 1] * B[3 + c] + A[3 * r + 2] * B[6 + c];
}
void mat_vec(const M3 A, const double* x, double* y) {
  for (int r = 0; r < 3; r++) y[r] = A[3 * r] * x[0] + A[3 * r + 1] * x[1] + A[3 * r + 2] * x[2];
}
double det3(const M3 A) {
  return A[0] * (A[4] * A[8] - A[5] * A[7]) - A[1] * (A[3] * A[8] - A[5] * A[6]) + A[2] * (A[3] * A[7] - A[4] * A[6]);
}
void inverse3(const M3 A, M3 I) {   // cofactors times 1 / det
  const double c00 = A[4] * A[8] - A[5] * A[7], c01 = A[5] * A[6] - A[3] * A[8], c02 = A[3] * A[7] - A[4] * A[6];
  const double invdet = 1.0 / (A[0] * c00 + A[1] * c01 + A[2] * c02);
  I[0] = c00 * invdet; I[1] = (A[2] * A[7] - A[1] * A[8]) * invdet; I[2] = (A[1] * A[5] - A[2] * A[4]) * invdet;
  I[3] = c01 * invdet; I[4] = (A[0] * A[8] - A[2] * A[6]) * invdet; I[5] = (A[2] * A[3] - A[0] * A[5]) * invdet;
  I[6] = c02 * invdet; I[7] = (A[1] * A[6] - A[0] * A[7]) * invdet; I[8] = (A[0] * A[4] - A[1] * A[3]) * invdet;
}

// rotation::RotationMatrixToAngleAxis, SfM/src/utils/basic_funcs.cc (the statement of host/objectsfm.cc)
void rotation_to_angle_axis(const M3 R, double* axis) {
  double q[4];
  const double trace = R[0] + R[4] + R[8];
  if (trace >= 0.0) {
    double t = std::sqrt(trace + 1.0);
    q[0] = 0.5 * t; t = 0.5 / t;
    q[1] = (R[7] - R[5]) * t; q[2] = (R[2] - R[6]) * t; q[3] = (R[3] - R[1]) * t;
  } else {
    int i = 0;
    if (R[4] > R[0]) i = 1;
    if (R[8] > R[4 * i]) i = 2;
    const int j = (i + 1) % 3, k = (j + 1) % 3;
    double t = std::sqrt(R[4 * i] - R[4 * j] - R[4 * k] + 1.0);
    q[i + 1] = 0.5 * t; t = 0.5 / t;
    q[0] = (R[3 * k + j] - R[3 * j + k]) * t; q[j + 1] = (R[3 * j + i] + R[3 * i + j]) * t; q[k + 1] = (R[3 * k + i] + R[3 * i + k]) * t;
  }
  const double s2 = q[1] * q[1] + q[2] * q[2] + q[3] * q[3];
  double k = 2.0;
  if (s2 > 0.0) {
    const double s = std::sqrt(s2);
    k = 2.0 * ((q[0] < 0.0) ? std::atan2(-s, -q[0]) : std::atan2(s, q[0])) / s;
  }
  axis[0] = q[1] * k; axis[1] = q[2] * k; axis[2] = q[3] * k;
}

// Camera::Transformation, SfM/src/camera.cc:79-87
void camera_transformation(double* R, double* t, double* c, double* aa, const M3 Rg, const double* tg, double scale) {
  M3 Ri, Rn, sR;
  double v[3];
  inverse3(Rg, Ri);
  mat_mat(R, Ri, Rn);                                        // pos_rt_.R = pos_rt_.R * R.inverse()
  for (int k = 0; k < 9; k++) { R[k] = Rn[k]; sR[k] = scale * Rg[k]; }
  mat_vec(sR, c, v);
  for (int k = 0; k < 3; k++) c[k] = v[k] + tg[k];           // pos_ac_.c = scale * R * pos_ac_.c + t
  mat_vec(R, c, v);
  for (int k = 0; k < 3; k++) t[k] = -v[k];                  // pos_rt_.t = -pos_rt_.R * pos_ac_.c
  rotation_to_angle_axis(R, aa);
}

}  // namespace

extern "C" {

void gr_svd3(const double* A, double* U, double* S, double* V) { svd3(A, U, S, V); }

// SimilarityTransformation, SfM/src/utils/transformation.cpp:142-216
int gr_similarity(int n, const double* src, const double* dst, const double* weight, double* Rg, double* tg, double* scale_out, double* err_out) {
  if (n < 3) return 0;                                                             // :151-153
  double s_center[3] = {0, 0, 0}, d_center[3] = {0, 0, 0};
  for (int i = 0; i < n; i++) for (int k = 0; k < 3; k++) { s_center[k] += src[3 * i + k]; d_center[k] += dst[3 * i + k]; }   // :159-162
  for (int k = 0; k < 3; k++) { s_center[k] /= n; d_center[k] /= n; }              // :163-164
  M3 cov = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  double s_mv = 0.0;
  for (int i = 0; i < n; i++) {                                                    // :172-182
    double ds[3], dd[3];
    for (int k = 0; k < 3; k++) { ds[k] = src[3 * i + k] - s_center[k]; dd[k] = dst[3 * i + k] - d_center[k]; }
    s_mv += (ds[0] * ds[0] + ds[1] * ds[1] + ds[2] * ds[2]) * weight[i];
    for (int r = 0; r < 3; r++) for (int c = 0; c < 3; c++) cov[3 * r + c] += ds[r] * dd[c] * weight[i];
  }
  s_mv /= n;                                                                       // :185
  for (int k = 0; k < 9; k++) cov[k] /= n;                                         // :186
  M3 U, V, Ut, VUt, VZ;
  double S[3];
  svd3(cov, U, S, V);                                                              // :189-192
  for (int r = 0; r < 3; r++) for (int c = 0; c < 3; c++) Ut[3 * r + c] = U[3 * c + r];
  mat_mat(V, Ut, VUt);
  const double Z[3] = {1.0, 1.0, det3(VUt)};                                       // :193-195
  for (int r = 0; r < 3; r++) for (int c = 0; c < 3; c++) VZ[3 * r + c] = V[3 * r + c] * Z[c];
  mat_mat(VZ, Ut, Rg);                                                             // :197
  const double scale = (S[0] * Z[0] + S[1] * Z[1] + S[2] * Z[2]) / s_mv;           // :199-203
  M3 sR;
  double v[3];
  for (int k = 0; k < 9; k++) sR[k] = -scale * Rg[k];
  mat_vec(sR, s_center, v);
  for (int k = 0; k < 3; k++) tg[k] = v[k] + d_center[k];                          // :205
  for (int k = 0; k < 9; k++) sR[k] = scale * Rg[k];
  double sum_err = 0.0;
  for (int i = 0; i < n; i++) {                                                    // :208-212
    mat_vec(sR, src + 3 * i, v);
    const double d0 = v[0] + tg[0] - dst[3 * i], d1 = v[1] + tg[1] - dst[3 * i + 1], d2 = v[2] + tg[2] - dst[3 * i + 2];
    sum_err += std::sqrt(d0 * d0 + d1 * d1 + d2 * d2);
  }
  *scale_out = scale;
  *err_out = sum_err / n;                                                          // :213
  return 1;
}

// SLAMGPS::AbsoluteOrientationWithGPSGlobal, slam_gps.cc:1596-1674.  cam_R / cam_c / gps are in / out.
int gr_orient_global(int n, int window, double clip_deg, double* cam_R, double* cam_t, double* cam_c, double* cam_aa, double* gps, double* weight,
                     double* Rg, double* tg, double* scale, double* err, double* offset) {
  const double pi = 3.1415926535897932384626433832795;   // CV_PI
  for (int i = 0; i < n; i++) {                                                    // :1606-1624
    int ids = i - window;
    if (ids < 0) ids = 0;
    int ide = i + window;
    if (ide > n - 1) ide = n - 1;
    const double dxs = gps[3 * ids] - gps[3 * i], dys = gps[3 * ids + 1] - gps[3 * i + 1];
    const double dxe = gps[3 * ide] - gps[3 * i], dye = gps[3 * ide + 1] - gps[3 * i + 1];
    double angle = std::acos((dxs * dxe + dys * dye) / std::sqrt(dxs * dxs + dys * dys + 0.1) / std::sqrt(dxe * dxe + dye * dye + 0.1));
    angle = std::fabs(angle - pi);
    if (angle >= pi * clip_deg / 180.0) angle = pi * clip_deg / 180.0;
    weight[i] = std::tan(angle);
  }
  if (!gr_similarity(n, cam_c, gps, weight, Rg, tg, scale, err)) return 0;         // :1632
  for (int i = 0; i < n; i++) camera_transformation(cam_R + 9 * i, cam_t + 3 * i, cam_c + 3 * i, cam_aa + 3 * i, Rg, tg, *scale);   // :1639-1641
  offset[0] = offset[1] = offset[2] = 0.0;                                         // :1651-1655
  for (int i = 0; i < n; i++) for (int k = 0; k < 3; k++) offset[k] += cam_c[3 * i + k];
  for (int k = 0; k < 3; k++) offset[k] /= n;
  const M3 eye = {1, 0, 0, 0, 1, 0, 0, 0, 1};
  const double neg[3] = {-offset[0], -offset[1], -offset[2]};
  for (int i = 0; i < n; i++) camera_transformation(cam_R + 9 * i, cam_t + 3 * i, cam_c + 3 * i, cam_aa + 3 * i, eye, neg, 1.0);    // :1657-1660
  for (int i = 0; i < n; i++) for (int k = 0; k < 3; k++) gps[3 * i + k] -= offset[k];                                              // :1668-1673
  return 1;
}

// SLAMGPS::GetAccuracy, slam_gps.cc:1573-1594, over AccuracyAssessment::ErrorReprojectionPts / Pti, accuracy_accessment.cc:38-113.
// ok = !is_bad_estimated_ (in / out); a track with fewer than min_views rows is bad on entry (slam_gps.cc:638-648).
void gr_accuracy(int n_tracks, const int32_t* off, const int32_t* cam, const double* xy, const double* cam_R, const double* cam_t,
                 const double* cam_fk, const double* cam_dc, const double* X, const uint8_t* ok_in, int min_views, double th_outlier, double* e_avg_out,
                 double* e_mse_out, int32_t* n_used, uint8_t* ok_out, int32_t* n_outliers, int32_t* n_inliers) {
  int count_outliers = 0;
  for (int p = 0; p < n_tracks; p++) {
    const bool bad = ok_in[p] == 0 || off[p + 1] - off[p] < min_views;
    double err_p = 1000.0, e_avg = 0.0, e_mse = 0.0;                               // accuracy_accessment.cc:94
    int n_obs = 0;
    if (!bad) {                                                                    // :95-97
      std::vector<double> errors;
      for (int i = off[p]; i < off[p + 1]; i++) {                                  // :45-61
        const double* R = cam_R + 9 * (size_t)cam[i];
        const double* t = cam_t + 3 * (size_t)cam[i];
        const double* fk = cam_fk + 3 * (size_t)cam[i];
        const double pc0 = R[0] * X[3 * p] + R[1] * X[3 * p + 1] + R[2] * X[3 * p + 2] + t[0];
        const double pc1 = R[3] * X[3 * p] + R[4] * X[3 * p + 1] + R[5] * X[3 * p + 2] + t[1];
        const double pc2 = R[6] * X[3 * p] + R[7] * X[3 * p + 1] + R[8] * X[3 * p + 2] + t[2];
        if (pc2 > 0) {
          const double x = pc0 / pc2, y = pc1 / pc2;
          const double r2 = x * x + y * y;
          const double distortion = 1.0 + r2 * (fk[1] + fk[2] * r2);
          const double dcx = cam_dc ? cam_dc[2 * (size_t)cam[i]] : 0.0, dcy = cam_dc ? cam_dc[2 * (size_t)cam[i] + 1] : 0.0;
          const double u = fk[0] * distortion * x + dcx, v = fk[0] * distortion * y + dcy;
          const double du = u - xy[2 * (size_t)i], dv = v - xy[2 * (size_t)i + 1];
          errors.push_back(du * du + dv * dv);                                     // std::pow(d, 2)
        }
      }
      if (errors.size() > 1) {                                                     // :64-66
        for (size_t k = 0; k < errors.size(); k++) e_avg += errors[k];
        e_avg /= errors.size();
        for (size_t k = 0; k < errors.size(); k++) e_mse += (errors[k] - e_avg) * (errors[k] - e_avg);
        e_mse = std::sqrt(e_mse / (errors.size() - 1));
        n_obs = (int)errors.size();
        err_p = e_avg;                                                             // :103
      } else {
        e_avg = 0.0;
      }
    }
    e_avg_out[p] = err_p; e_mse_out[p] = n_obs ? e_mse : 0.0; n_used[p] = n_obs;
    bool is_bad = bad;
    if (err_p > th_outlier) { is_bad = true; count_outliers++; }                   // slam_gps.cc:1587-1591
    ok_out[p] = !is_bad;
  }
  *n_outliers = count_outliers;
  *n_inliers = n_tracks - count_outliers;                                          // :1593
}

// the point loop of SLAMGPS::GPSRegistration2, slam_gps.cc:920-978
void gr_register_points(int n_tracks, const int32_t* off, const int32_t* cam, const uint8_t* ok, int n_cams, const double* cam_c, const double* gps,
                        double* X) {
  std::vector<double> cam_offset(3 * (size_t)n_cams);
  for (int c = 0; c < n_cams; c++) for (int k = 0; k < 3; k++) cam_offset[3 * c + k] = gps[3 * c + k] - cam_c[3 * c + k];   // :920-924
  for (int p = 0; p < n_tracks; p++) {
    if (!ok[p]) continue;                                                          // :940-942
    double offset_i[3] = {0.0, 0.0, 0.0}, weight_i = 0.0;
    for (int i = off[p]; i < off[p + 1]; i++) {
      const int id_cam = cam[i];
      const double dx = X[3 * p] - cam_c[3 * id_cam], dy = X[3 * p + 1] - cam_c[3 * id_cam + 1], dz = X[3 * p + 2] - cam_c[3 * id_cam + 2];
      const double dis = std::sqrt(dx * dx + dy * dy + dz * dz);
      const double w = 1.0 / (std::sqrt(dis) + 5.0);
      weight_i += w;
      for (int k = 0; k < 3; k++) offset_i[k] += w * cam_offset[3 * id_cam + k];
    }
    for (int k = 0; k < 3; k++) offset_i[k] /= weight_i;                           // :970-972
    for (int k = 0; k < 3; k++) X[3 * p + k] += offset_i[k];                       // :975-977
  }
}

}  // extern "C"
