// What rectify.hip does without a device: the argument checks, the rectification geometry of include/msfm.h, "Stereo
// rectification" (binary64 on the host, every operation in the order written here, nothing fused), the parameter block the kernel
// reads, and the integer blend of the warp, which the kernel and nothing else calls.  Plain C++.
// A check returns an empty string or the refusal's text.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <string>

#if defined(__HIPCC__)
#define RECT_HD __host__ __device__
#else
#define RECT_HD
#endif
#if defined(__clang__)
#pragma clang fp contract(off)   // to the end of the file that includes this: a * b + c stays two roundings, on host and device
#endif

#define RECT_MAX_SIDE 16384
#define RECT_STATS 3             // = MSFM_RECTIFY_STATS; order and meaning of SGM_STATS
#define RECT_ST_WAITS 0
#define RECT_ST_H2D 1
#define RECT_ST_LAUNCHES 2
#define RECT_FETCH_KINDS 6
#define RECT_PI_GUARD 1e-6       // a relative rotation this close to pi has lost its axis in the skew part

struct RectGeometry {
  double R1[9], R2[9], P1[12], P2[12], Q[16];
  int idx;
};
// one camera's part of the parameter block: iR = inv(P[:, :3] R), then the camera's own fx, fy, cx, cy
struct RectCamera {
  double iR[9];
  double fx, fy, cx, cy;
};
struct RectParams {
  RectCamera cam[2];
};
#define RECT_PARAM_BYTES 208
static_assert(sizeof(RectParams) == RECT_PARAM_BYTES, "the parameter block is 2 x 13 doubles");

static inline std::string rect_check_size(int width, int height) {
  char buf[128];
  if (width < 1 || width > RECT_MAX_SIDE || height < 1 || height > RECT_MAX_SIDE) {
    snprintf(buf, sizeof buf, "%d x %d: a side outside [1, %d]", width, height, RECT_MAX_SIDE);
    return buf;
  }
  return "";
}

static inline std::string rect_check_pair(const void* left, int left_stride, const void* right, int right_stride, int width) {
  char buf[128];
  if (!left || !right) return "null argument";
  if (left_stride < width || right_stride < width) {
    snprintf(buf, sizeof buf, "stride = %d below width = %d", left_stride < width ? left_stride : right_stride, width);
    return buf;
  }
  return "";
}

// bytes per pixel of a fetch kind: 0 / 1 the rectified planes, 2 .. 5 the maps; 0 for a kind outside the range
static inline int rect_fetch_item(int kind) {
  if (kind == 0 || kind == 1) return 1;
  return (kind >= 2 && kind < RECT_FETCH_KINDS) ? 4 : 0;
}

static inline void rect_mul33(const double* A, const double* B, double* C) {
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) C[3 * i + j] = (A[3 * i] * B[j] + A[3 * i + 1] * B[3 + j]) + A[3 * i + 2] * B[6 + j];
}
static inline void rect_mul31(const double* A, const double* x, double* y) {
  for (int i = 0; i < 3; i++) y[i] = (A[3 * i] * x[0] + A[3 * i + 1] * x[1]) + A[3 * i + 2] * x[2];
}
static inline void rect_transpose(const double* A, double* T) {
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) T[3 * i + j] = A[3 * j + i];
}
static inline double rect_norm3(const double* v) { return sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]); }

// the inverse by the adjugate: every cofactor divided by the determinant along the first row
static inline void rect_inv33(const double* a, double* inv) {
  const double c[9] = {a[4] * a[8] - a[5] * a[7], a[2] * a[7] - a[1] * a[8], a[1] * a[5] - a[2] * a[4],
                       a[5] * a[6] - a[3] * a[8], a[0] * a[8] - a[2] * a[6], a[2] * a[3] - a[0] * a[5],
                       a[3] * a[7] - a[4] * a[6], a[1] * a[6] - a[0] * a[7], a[0] * a[4] - a[1] * a[3]};
  const double det = (a[0] * c[0] + a[1] * c[3]) + a[2] * c[6];
  for (int i = 0; i < 9; i++) inv[i] = c[i] / det;
}

// the rotation matrix of a rotation vector; the identity for the zero vector
static inline void rect_rodrigues(const double* v, double* R) {
  const double th = rect_norm3(v);
  for (int i = 0; i < 9; i++) R[i] = (i % 4 == 0) ? 1.0 : 0.0;
  if (th == 0) return;
  const double c = cos(th), s = sin(th), c1 = 1.0 - c;
  const double k[3] = {v[0] / th, v[1] / th, v[2] / th};
  const double Kx[9] = {0, -k[2], k[1], k[2], 0, -k[0], -k[1], k[0], 0};
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) R[3 * i + j] = (c * R[3 * i + j] + (c1 * k[i]) * k[j]) + s * Kx[3 * i + j];
}

// the rotation vector of a rotation matrix, from the skew part and the trace; *theta: its angle
static inline void rect_rotvec(const double* R, double* om, double* theta) {
  double c = (((R[0] + R[4]) + R[8]) - 1.0) * 0.5;
  c = c > 1.0 ? 1.0 : (c < -1.0 ? -1.0 : c);
  const double th = acos(c);
  const double r[3] = {(R[7] - R[5]) * 0.5, (R[2] - R[6]) * 0.5, (R[3] - R[1]) * 0.5};
  const double s = rect_norm3(r);
  for (int i = 0; i < 3; i++) om[i] = s == 0 ? 0.0 : r[i] * (th / s);
  *theta = th;
}

static inline bool rect_all_finite(const double* v, int n) {
  for (int i = 0; i < n; i++)
    if (!std::isfinite(v[i])) return false;
  return true;
}

// msfm_stereo_rectify's arithmetic; g is written only when the result is the empty string
static inline std::string rect_geometry(const double* K1, const double* R1, const double* t1, const double* K2, const double* R2,
                                        const double* t2, int width, int height, RectGeometry& out) {
  if (!K1 || !R1 || !t1 || !K2 || !R2 || !t2) return "null argument";
  const std::string bad = rect_check_size(width, height);
  if (!bad.empty()) return bad;
  if (!rect_all_finite(K1, 9) || !rect_all_finite(R1, 9) || !rect_all_finite(t1, 3) || !rect_all_finite(K2, 9) || !rect_all_finite(R2, 9) ||
      !rect_all_finite(t2, 3))
    return "a non-finite value in K, R or t";
  if (!(K1[0] > 0 && K1[4] > 0 && K2[0] > 0 && K2[4] > 0)) return "a focal length that is not positive";
  RectGeometry g;
  double R1i[9], R21[9], t21[3], om[3], theta, half[3], rr[9], rrT[9], t[3];
  rect_inv33(R1, R1i);
  rect_mul33(R2, R1i, R21);
  rect_mul31(R21, t1, t21);
  for (int i = 0; i < 3; i++) t21[i] = -t21[i] + t2[i];   // dense_reconstruction.cc:309, t used as a translation
  if (!rect_all_finite(R21, 9) || !rect_all_finite(t21, 3)) return "R1 has no inverse";
  rect_rotvec(R21, om, &theta);
  if (M_PI - theta < RECT_PI_GUARD) return "the relative rotation is a half turn: its axis is lost";
  for (int i = 0; i < 3; i++) half[i] = -0.5 * om[i];
  rect_rodrigues(half, rr);
  rect_mul31(rr, t21, t);
  const int idx = fabs(t[0]) > fabs(t[1]) ? 0 : 1;
  const double c = t[idx], nt = rect_norm3(t);
  if (!(nt > 0)) return "the two cameras have one centre: no baseline";
  double uu[3] = {0, 0, 0};
  uu[idx] = c > 0 ? 1.0 : -1.0;
  double ww[3] = {t[1] * uu[2] - t[2] * uu[1], t[2] * uu[0] - t[0] * uu[2], t[0] * uu[1] - t[1] * uu[0]};
  const double nw = rect_norm3(ww);
  if (nw > 0) {
    const double f = acos(fabs(c) / nt) / nw;
    for (int i = 0; i < 3; i++) ww[i] = ww[i] * f;
  }
  double wR[9], trect[3];
  rect_rodrigues(ww, wR);
  rect_transpose(rr, rrT);
  rect_mul33(wR, rrT, g.R1);
  rect_mul33(wR, rr, g.R2);
  rect_mul31(g.R2, t21, trect);
  const int o = idx ^ 1;
  const double fc = K1[4 * o] < K2[4 * o] ? K1[4 * o] : K2[4 * o];
  double cc[2][2];
  for (int k = 0; k < 2; k++) {
    const double* K = k ? K2 : K1;
    const double* R = k ? g.R2 : g.R1;
    double sx = 0, sy = 0;
    for (int q = 0; q < 4; q++) {
      const double n[3] = {((q & 1 ? width - 1 : 0) - K[2]) / K[0], ((q & 2 ? height - 1 : 0) - K[5]) / K[4], 1.0};
      double p[3];
      rect_mul31(R, n, p);
      sx = sx + (p[0] / p[2]) * fc;
      sy = sy + (p[1] / p[2]) * fc;
    }
    cc[k][0] = (width - 1) * 0.5 - sx * 0.25;
    cc[k][1] = (height - 1) * 0.5 - sy * 0.25;
  }
  const double ccx = (cc[0][0] + cc[1][0]) * 0.5, ccy = (cc[0][1] + cc[1][1]) * 0.5;   // CALIB_ZERO_DISPARITY
  const double P[12] = {fc, 0, ccx, 0, 0, fc, ccy, 0, 0, 0, 1, 0};
  for (int i = 0; i < 12; i++) g.P1[i] = g.P2[i] = P[i];
  g.P2[4 * idx + 3] = trect[idx] * fc;
  const double Q[16] = {1, 0, 0, -ccx, 0, 1, 0, -ccy, 0, 0, 0, fc, 0, 0, -1.0 / trect[idx], 0};
  for (int i = 0; i < 16; i++) g.Q[i] = Q[i];
  g.idx = idx;
  if (!rect_all_finite(g.R1, 9) || !rect_all_finite(g.R2, 9) || !rect_all_finite(g.P1, 12) || !rect_all_finite(g.P2, 12) ||
      !rect_all_finite(g.Q, 16))
    return "the poses give no finite rectification";
  out = g;
  return "";
}

// the parameter block of the maps: per camera iR = inv(P[:, :3] R) and the camera's own K without its skew entry
static inline void rect_params(const RectGeometry& g, const double* K1, const double* K2, RectParams& out) {
  for (int k = 0; k < 2; k++) {
    const double* P = k ? g.P2 : g.P1;
    const double* K = k ? K2 : K1;
    const double A[9] = {P[0], P[1], P[2], P[4], P[5], P[6], P[8], P[9], P[10]};
    double M[9];
    rect_mul33(A, k ? g.R2 : g.R1, M);
    rect_inv33(M, out.cam[k].iR);
    out.cam[k].fx = K[0]; out.cam[k].fy = K[4]; out.cam[k].cx = K[2]; out.cam[k].cy = K[5];
  }
}

// The warp's blend: sx, sy are the source position in 1/32 pixel (already rounded).  A tap outside the source counts 0, each tap
// on its own.  The four weights are products of two 5-bit fractions, so this is OpenCV's table of 15-bit weights without a rounding.
RECT_HD static inline uint8_t rect_blend(const uint8_t* __restrict__ src, int w, int h, int sx, int sy) {
  const int ix = sx >> 5, iy = sy >> 5, ax = sx & 31, ay = sy & 31;
  const bool x0 = ix >= 0 && ix < w, x1 = ix + 1 >= 0 && ix + 1 < w, y0 = iy >= 0 && iy < h, y1 = iy + 1 >= 0 && iy + 1 < h;
  const int p00 = (x0 && y0) ? src[(size_t)iy * w + ix] : 0;
  const int p01 = (x1 && y0) ? src[(size_t)iy * w + ix + 1] : 0;
  const int p10 = (x0 && y1) ? src[(size_t)(iy + 1) * w + ix] : 0;
  const int p11 = (x1 && y1) ? src[(size_t)(iy + 1) * w + ix + 1] : 0;
  const int S = (32 - ax) * (32 - ay) * p00 + ax * (32 - ay) * p01 + (32 - ax) * ay * p10 + ax * ay * p11;
  return (uint8_t)((S + 512) >> 10);
}
