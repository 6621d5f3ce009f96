// Sequential CPU restatement of msfm_homography_ransac_batch (metricsfm_amd/csrc/geo.hip): cv::findHomography(pts1,
// pts2, mask, RANSAC, th) of OpenCV 2.4 (cvFindHomography + CvHomographyEstimator + CvModelEstimator2::runRANSAC +
// CvLevMarq) written as one plain loop per pair, with the counter-based sampler and the summation orders of the GPU
// path.  Built by tests/test_homography_ref.py with `g++ -O2 -ffp-contract=off -shared` and loaded with ctypes; the GPU
// tests compare against it bit for bit.  Only + - * / sqrt on doubles, in the order written.
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <algorithm>
#include <cstring>
#include <vector>

namespace {

uint64_t sm64(uint64_t& s) {
  s += 0x9E3779B97F4A7C15ull;
  uint64_t z = s;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

// cvRANSACUpdateNumIters
int update_num_iters(double p, double ep, int model_points, int max_iters) {
  p = std::max(p, 0.0); p = std::min(p, 1.0);
  ep = std::max(ep, 0.0); ep = std::min(ep, 1.0);
  double num = std::max(1.0 - p, DBL_MIN);
  double denom = 1.0 - std::pow(1.0 - ep, model_points);
  if (denom < DBL_MIN) return 0;
  num = std::log(num);
  denom = std::log(denom);
  if (denom >= 0 || -num >= max_iters * (-denom)) return max_iters;
  return (int)std::lrint(num / denom);
}

// CvModelEstimator2::checkSubset with checkPartialSubsets = false: no three of the four points collinear
bool check_subset(const double* x, const double* y) {
  for (int i = 0; i < 4; i++)
    for (int j = 0; j < i; j++) {
      const double dx1 = x[j] - x[i], dy1 = y[j] - y[i];
      for (int k = 0; k < j; k++) {
        const double dx2 = x[k] - x[i], dy2 = y[k] - y[i];
        if (fabs(dx2 * dy1 - dy2 * dx1) <= FLT_EPSILON * (fabs(dx1) + fabs(dy1) + fabs(dx2) + fabs(dy2))) return false;
      }
    }
  return true;
}

// H = invHnorm * H0 * Hnorm2, then H /= H[8]; false if any entry is not finite
bool denormalise(const double* H0, double csx, double csy, double cx, double cy, double sMx, double sMy, double cMx, double cMy,
                 double* H) {
  const double a[9] = {1.0 / csx, 0.0, cx, 0.0, 1.0 / csy, cy, 0.0, 0.0, 1.0};
  const double b[9] = {sMx, 0.0, -cMx * sMx, 0.0, sMy, -cMy * sMy, 0.0, 0.0, 1.0};
  double t[9], u[9];
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) {
      double s = a[i * 3 + 0] * H0[0 * 3 + j];
      s = s + a[i * 3 + 1] * H0[1 * 3 + j];
      s = s + a[i * 3 + 2] * H0[2 * 3 + j];
      t[i * 3 + j] = s;
    }
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) {
      double s = t[i * 3 + 0] * b[0 * 3 + j];
      s = s + t[i * 3 + 1] * b[1 * 3 + j];
      s = s + t[i * 3 + 2] * b[2 * 3 + j];
      u[i * 3 + j] = s;
    }
  bool fin = true;
  for (int k = 0; k < 8; k++) { H[k] = u[k] / u[8]; fin = fin && fabs(H[k]) <= DBL_MAX; }
  H[8] = 1.0;
  return fin;
}

// The exact homography of four correspondences (CvHomographyEstimator::runKernel on a sample): normalise, null vector of
// the 8x9 DLT system by Gauss-Jordan with full pivoting, denormalise.  false: no model.
bool solve4(const double* X1, const double* Y1, const double* X2, const double* Y2, double* H) {
  double cx = 0, cy = 0, cMx = 0, cMy = 0;
  for (int i = 0; i < 4; i++) { cx = cx + X2[i]; cy = cy + Y2[i]; cMx = cMx + X1[i]; cMy = cMy + Y1[i]; }
  cx = cx / 4.0; cy = cy / 4.0; cMx = cMx / 4.0; cMy = cMy / 4.0;
  double sx = 0, sy = 0, sMx = 0, sMy = 0;
  for (int i = 0; i < 4; i++) {
    sx = sx + fabs(X2[i] - cx); sy = sy + fabs(Y2[i] - cy);
    sMx = sMx + fabs(X1[i] - cMx); sMy = sMy + fabs(Y1[i] - cMy);
  }
  if (fabs(sx) < DBL_EPSILON || fabs(sy) < DBL_EPSILON || fabs(sMx) < DBL_EPSILON || fabs(sMy) < DBL_EPSILON) return false;
  sx = 4.0 / sx; sy = 4.0 / sy; sMx = 4.0 / sMx; sMy = 4.0 / sMy;
  double A[8][9];
  for (int i = 0; i < 4; i++) {
    const double x = (X2[i] - cx) * sx, y = (Y2[i] - cy) * sy;
    const double X = (X1[i] - cMx) * sMx, Y = (Y1[i] - cMy) * sMy;
    const double lx[9] = {X, Y, 1.0, 0.0, 0.0, 0.0, -x * X, -x * Y, -x};
    const double ly[9] = {0.0, 0.0, 0.0, X, Y, 1.0, -y * X, -y * Y, -y};
    for (int c = 0; c < 9; c++) { A[2 * i][c] = lx[c]; A[2 * i + 1][c] = ly[c]; }
  }
  int perm[9];
  for (int c = 0; c < 9; c++) perm[c] = c;
  for (int i = 0; i < 8; i++) {
    int pr = i, pc = i;
    double best = -1.0;
    for (int r = i; r < 8; r++)
      for (int c = i; c < 9; c++) {
        const double v = fabs(A[r][c]);
        if (v > best) { best = v; pr = r; pc = c; }
      }
    if (!(best > 0.0)) return false;
    if (pr != i)
      for (int c = 0; c < 9; c++) { const double t = A[i][c]; A[i][c] = A[pr][c]; A[pr][c] = t; }
    if (pc != i) {
      for (int r = 0; r < 8; r++) { const double t = A[r][i]; A[r][i] = A[r][pc]; A[r][pc] = t; }
      const int t = perm[i]; perm[i] = perm[pc]; perm[pc] = t;
    }
    const double piv = A[i][i];
    for (int c = i; c < 9; c++) A[i][c] = A[i][c] / piv;
    for (int r = 0; r < 8; r++) {
      if (r == i) continue;
      const double f = A[r][i];
      for (int c = i; c < 9; c++) A[r][c] = A[r][c] - f * A[i][c];
    }
  }
  double h0[9];
  for (int j = 0; j < 9; j++) h0[perm[j]] = j < 8 ? -A[j][8] : 1.0;
  return denormalise(h0, sx, sy, cx, cy, sMx, sMy, cMx, cMy, H);
}

// Symmetric eigen-decomposition by cyclic Jacobi (n <= 9, A row-major n x n, destroyed): w[k] eigenvalues, V column k its
// eigenvector.  Rotation (p, q) in row order p < q; an off-diagonal entry negligible against both diagonal entries is
// set to zero; at most 50 sweeps.
void jacobi_eigen(double* A, int n, double* w, double* V) {
  for (int i = 0; i < n; i++)
    for (int j = 0; j < n; j++) V[i * n + j] = i == j ? 1.0 : 0.0;
  for (int sweep = 0; sweep < 50; sweep++) {
    bool any = false;
    for (int p = 0; p < n - 1; p++)
      for (int q = p + 1; q < n; q++) {
        const double apq = A[p * n + q];
        if (apq == 0.0) continue;
        const double app = A[p * n + p], aqq = A[q * n + q];
        const double g = 100.0 * fabs(apq);
        if (fabs(app) + g == fabs(app) && fabs(aqq) + g == fabs(aqq)) { A[p * n + q] = 0.0; A[q * n + p] = 0.0; continue; }
        any = true;
        const double theta = (aqq - app) / (2.0 * apq);
        double t;
        if (fabs(theta) > 1e150) t = 0.5 / theta;
        else {
          t = 1.0 / (fabs(theta) + sqrt(theta * theta + 1.0));
          if (theta < 0.0) t = -t;
        }
        const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
        for (int k = 0; k < n; k++) {
          const double akp = A[k * n + p], akq = A[k * n + q];
          A[k * n + p] = c * akp - s * akq;
          A[k * n + q] = s * akp + c * akq;
        }
        for (int k = 0; k < n; k++) {
          const double apk = A[p * n + k], aqk = A[q * n + k];
          A[p * n + k] = c * apk - s * aqk;
          A[q * n + k] = s * apk + c * aqk;
        }
        A[p * n + q] = 0.0; A[q * n + p] = 0.0;
        for (int k = 0; k < n; k++) {
          const double vkp = V[k * n + p], vkq = V[k * n + q];
          V[k * n + p] = c * vkp - s * vkq;
          V[k * n + q] = s * vkp + c * vkq;
        }
      }
    if (!any) break;
  }
  for (int k = 0; k < n; k++) w[k] = A[k * n + k];
}

// 10^k for k = -16 .. 16 (CvLevMarq's lambda; OpenCV forms it as exp(k ln 10))
const double kLambda[33] = {1e-16, 1e-15, 1e-14, 1e-13, 1e-12, 1e-11, 1e-10, 1e-9, 1e-8, 1e-7, 1e-6, 1e-5, 1e-4, 1e-3, 1e-2, 1e-1, 1e0,
                            1e1,   1e2,   1e3,   1e4,   1e5,   1e6,   1e7,   1e8,   1e9,   1e10, 1e11, 1e12, 1e13, 1e14, 1e15, 1e16};

// CvLevMarq::step: param = prev - (JtJ with its diagonal times (1 + lambda))^+ JtErr, the pseudo-inverse by the
// eigen-decomposition (the damped matrix is symmetric positive semi-definite), singular values <= 2 eps sum(w) dropped.
// JtJ: the upper triangle of the 8x8, row-major [36].
void lm_step(const double* prev, const double* JtJ, const double* JtErr, int lam, double* param) {
  double A[64], V[64], w[8];
  int e = 0;
  for (int j = 0; j < 8; j++)
    for (int k = j; k < 8; k++) { A[j * 8 + k] = JtJ[e]; A[k * 8 + j] = JtJ[e]; e++; }
  const double f = 1.0 + kLambda[lam + 16];
  for (int j = 0; j < 8; j++) A[j * 8 + j] = A[j * 8 + j] * f;
  jacobi_eigen(A, 8, w, V);
  int ord[8];
  for (int k = 0; k < 8; k++) ord[k] = k;
  for (int k = 0; k < 7; k++) {   // descending, as cvSVD returns them
    int m = k;
    for (int i = k + 1; i < 8; i++)
      if (w[ord[m]] < w[ord[i]]) m = i;
    const int t = ord[k]; ord[k] = ord[m]; ord[m] = t;
  }
  double th = 0.0;
  for (int k = 0; k < 8; k++) th = th + w[ord[k]];
  th = th * (2.0 * DBL_EPSILON);
  double x[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  for (int k = 0; k < 8; k++) {
    const int c = ord[k];
    const double wi = w[c];
    if (fabs(wi) <= th) continue;
    double s = 0.0;
    for (int j = 0; j < 8; j++) s = s + V[j * 8 + c] * JtErr[j];
    s = s * (1.0 / wi);
    for (int j = 0; j < 8; j++) x[j] = x[j] + V[j * 8 + c] * s;
  }
  for (int j = 0; j < 8; j++) param[j] = prev[j] - x[j];
}

// Sums over the inliers of a pair in the order of the GPU's polish kernel: lane l of 64 accumulates correspondences
// l, l + 64, ... in ascending order, then the 64 partials are added by the butterfly d = 32, 16, ..., 1.
struct Lanes {
  int nv;
  std::vector<double> v;   // [64][nv]
  explicit Lanes(int n) : nv(n), v((size_t)64 * n, 0.0) {}
  double* lane(int l) { return v.data() + (size_t)l * nv; }
  void reduce(double* out) {
    for (int d = 32; d > 0; d >>= 1) {
      std::vector<double> nvv(v.size());
      for (int l = 0; l < 64; l++)
        for (int k = 0; k < nv; k++) nvv[(size_t)l * nv + k] = v[(size_t)l * nv + k] + v[(size_t)(l ^ d) * nv + k];
      v.swap(nvv);
    }
    for (int k = 0; k < nv; k++) out[k] = v[k];
  }
};

// cvFindHomography's refit on the inliers (runKernel over all of them): LtL summed in the lane order above, its
// eigenvector of the smallest eigenvalue.  false: the inliers have no spread (H is left as it is).
bool refit(int N, const double* X1, const double* Y1, const double* X2, const double* Y2, const uint8_t* in, double* H) {
  double s4[5];
  {
    Lanes L(5);
    for (int e = 0; e < N; e++) {
      if (!in[e]) continue;
      double* a = L.lane(e & 63);
      a[0] = a[0] + X2[e]; a[1] = a[1] + Y2[e]; a[2] = a[2] + X1[e]; a[3] = a[3] + Y1[e]; a[4] = a[4] + 1.0;
    }
    L.reduce(s4);
  }
  const double cnt = s4[4];
  const double cx = s4[0] / cnt, cy = s4[1] / cnt, cMx = s4[2] / cnt, cMy = s4[3] / cnt;
  double d4[4];
  {
    Lanes L(4);
    for (int e = 0; e < N; e++) {
      if (!in[e]) continue;
      double* a = L.lane(e & 63);
      a[0] = a[0] + fabs(X2[e] - cx); a[1] = a[1] + fabs(Y2[e] - cy); a[2] = a[2] + fabs(X1[e] - cMx); a[3] = a[3] + fabs(Y1[e] - cMy);
    }
    L.reduce(d4);
  }
  if (fabs(d4[0]) < DBL_EPSILON || fabs(d4[1]) < DBL_EPSILON || fabs(d4[2]) < DBL_EPSILON || fabs(d4[3]) < DBL_EPSILON) return false;
  const double sx = cnt / d4[0], sy = cnt / d4[1], sMx = cnt / d4[2], sMy = cnt / d4[3];
  double LtL[45];
  {
    Lanes L(45);
    for (int e = 0; e < N; e++) {
      if (!in[e]) continue;
      const double x = (X2[e] - cx) * sx, y = (Y2[e] - cy) * sy;
      const double X = (X1[e] - cMx) * sMx, Y = (Y1[e] - cMy) * sMy;
      const double lx[9] = {X, Y, 1.0, 0.0, 0.0, 0.0, -x * X, -x * Y, -x};
      const double ly[9] = {0.0, 0.0, 0.0, X, Y, 1.0, -y * X, -y * Y, -y};
      double* a = L.lane(e & 63);
      int q = 0;
      for (int j = 0; j < 9; j++)
        for (int k = j; k < 9; k++) { a[q] = a[q] + (lx[j] * lx[k] + ly[j] * ly[k]); q++; }
    }
    L.reduce(LtL);
  }
  double A[81], V[81], w[9];
  int q = 0;
  for (int j = 0; j < 9; j++)
    for (int k = j; k < 9; k++) { A[j * 9 + k] = LtL[q]; A[k * 9 + j] = LtL[q]; q++; }
  jacobi_eigen(A, 9, w, V);
  int m = 0;
  for (int k = 1; k < 9; k++)
    if (w[k] < w[m]) m = k;
  double h0[9], Hn[9];
  for (int k = 0; k < 9; k++) h0[k] = V[k * 9 + m];
  if (!denormalise(h0, sx, sy, cx, cy, sMx, sMy, cMx, cMy, Hn)) return false;
  for (int k = 0; k < 9; k++) H[k] = Hn[k];
  return true;
}

// One evaluation of CvHomographyEstimator::refine's loop body over the inliers: JtJ (upper, 36), JtErr (8), errNorm.
void lm_eval(int N, const double* X1, const double* Y1, const double* X2, const double* Y2, const uint8_t* in, const double* h,
             bool jac, double* out /*[45]*/) {
  Lanes L(45);
  for (int e = 0; e < N; e++) {
    if (!in[e]) continue;
    const double Mx = X1[e], My = Y1[e];
    double ww = h[6] * Mx + h[7] * My + 1.0;
    ww = fabs(ww) > DBL_EPSILON ? 1.0 / ww : 0.0;
    const double xi = (h[0] * Mx + h[1] * My + h[2]) * ww;
    const double yi = (h[3] * Mx + h[4] * My + h[5]) * ww;
    const double e0 = xi - X2[e], e1 = yi - Y2[e];
    double* a = L.lane(e & 63);
    if (jac) {
      const double J0[8] = {Mx * ww, My * ww, ww, 0.0, 0.0, 0.0, -Mx * ww * xi, -My * ww * xi};
      const double J1[8] = {0.0, 0.0, 0.0, Mx * ww, My * ww, ww, -Mx * ww * yi, -My * ww * yi};
      int q = 0;
      for (int j = 0; j < 8; j++) {
        for (int k = j; k < 8; k++) { a[q] = a[q] + (J0[j] * J0[k] + J1[j] * J1[k]); q++; }
      }
      for (int j = 0; j < 8; j++) a[36 + j] = a[36 + j] + (J0[j] * e0 + J1[j] * e1);
    }
    a[44] = a[44] + (e0 * e0 + e1 * e1);
  }
  L.reduce(out);
}

// CvHomographyEstimator::refine(M, m, H, 10) through CvLevMarq::updateAlt's state machine.
void refine(int N, const double* X1, const double* Y1, const double* X2, const double* Y2, const uint8_t* in, double* H) {
  double param[8], prev[8], ev[45], JtJ[36], JtErr[8];
  for (int k = 0; k < 8; k++) param[k] = H[k];
  int lam = -3, iters = 0;
  lm_eval(N, X1, Y1, X2, Y2, in, param, true, ev);
  double errNorm = ev[44];
  for (int k = 0; k < 36; k++) JtJ[k] = ev[k];
  for (int k = 0; k < 8; k++) JtErr[k] = ev[36 + k];
  for (;;) {
    for (int k = 0; k < 8; k++) prev[k] = param[k];
    lm_step(prev, JtJ, JtErr, lam, param);
    double prevErr = errNorm;
    lm_eval(N, X1, Y1, X2, Y2, in, param, false, ev);
    errNorm = ev[44];
    while (errNorm > prevErr) {
      if (++lam > 16) break;
      lm_step(prev, JtJ, JtErr, lam, param);
      lm_eval(N, X1, Y1, X2, Y2, in, param, false, ev);
      errNorm = ev[44];
    }
    lam = std::max(lam - 1, -16);
    double dn = 0.0, pn = 0.0;
    for (int k = 0; k < 8; k++) { const double d = param[k] - prev[k]; dn = dn + d * d; pn = pn + prev[k] * prev[k]; }
    const double change = sqrt(dn) / (sqrt(pn) + DBL_EPSILON);
    if (++iters >= 10 || change < DBL_EPSILON) break;
    lm_eval(N, X1, Y1, X2, Y2, in, param, true, ev);
    for (int k = 0; k < 36; k++) JtJ[k] = ev[k];
    for (int k = 0; k < 8; k++) JtErr[k] = ev[36 + k];
  }
  for (int k = 0; k < 8; k++) H[k] = param[k];
  H[8] = 1.0;
}

// err = (float)(dx^2 + dy^2) of the transfer into image 2, inlier iff (double)err <= th2
bool h_inlier(const double* H, double x1, double y1, double x2, double y2, double th2) {
  const double ww = 1.0 / (H[6] * x1 + H[7] * y1 + 1.0);
  const double dx = (H[0] * x1 + H[1] * y1 + H[2]) * ww - x2;
  const double dy = (H[3] * x1 + H[4] * y1 + H[5]) * ww - y2;
  const float err = (float)(dx * dx + dy * dy);
  return (double)err <= th2;
}

// sample h of pair p: 0 = model in H, 1 = no model (degenerate spread / pivot), 2 = no admissible subset in 300 attempts
int sample_model(uint64_t seed, int p, int h, int N, const double* X1, const double* Y1, const double* X2, const double* Y2,
                 double* H) {
  uint64_t s = seed ^ ((uint64_t)p * 0xD1342543DE82EF95ull) ^ ((uint64_t)h * 0xA24BAED4963EE407ull);
  for (int att = 0; att < 300; att++) {
    int idx[4];
    for (int k = 0; k < 4; k++) {
      for (;;) {
        const int v = (int)(sm64(s) % (uint64_t)N);
        bool dup = false;
        for (int j = 0; j < k; j++) dup = dup || (idx[j] == v);
        if (!dup) { idx[k] = v; break; }
      }
    }
    double a1[4], b1[4], a2[4], b2[4];
    for (int k = 0; k < 4; k++) { a1[k] = X1[idx[k]]; b1[k] = Y1[idx[k]]; a2[k] = X2[idx[k]]; b2[k] = Y2[idx[k]]; }
    if (!check_subset(a1, b1) || !check_subset(a2, b2)) continue;
    return solve4(a1, b1, a2, b2, H) ? 0 : 1;
  }
  return 2;
}

}  // namespace

extern "C" int hr_update_num_iters(double p, double ep, int model_points, int max_iters) {
  return update_num_iters(p, ep, model_points, max_iters);
}

extern "C" int hr_homography_ransac_batch(int n_pairs, const int* offsets, const float* pt1, const float* pt2, double threshold,
                                          double confidence, int max_iterations, int polish, uint64_t seed, double* Hout,
                                          uint8_t* inlier, int* n_inliers, uint8_t* ok) {
  if (threshold <= 0.0) threshold = 3.0;
  const double th2 = threshold * threshold;
  for (int p = 0; p < n_pairs; p++) {
    const int o = offsets[p], N = offsets[p + 1] - o;
    double* Hp = Hout + (size_t)p * 9;
    for (int k = 0; k < 9; k++) Hp[k] = 0.0;
    ok[p] = 0;
    if (N < 4) {
      for (int e = 0; e < N; e++) inlier[o + e] = 0;
      n_inliers[p] = 0;
      continue;
    }
    std::vector<double> X1(N), Y1(N), X2(N), Y2(N);
    for (int e = 0; e < N; e++) {
      X1[e] = pt1[2 * (o + e)]; Y1[e] = pt1[2 * (o + e) + 1];
      X2[e] = pt2[2 * (o + e)]; Y2[e] = pt2[2 * (o + e) + 1];
    }
    for (int e = 0; e < N; e++) inlier[o + e] = 1;   // cvFindHomography's temporary mask starts at ones
    n_inliers[p] = N;
    if (N == 4) {
      double H[9];
      if (solve4(X1.data(), Y1.data(), X2.data(), Y2.data(), H)) {
        for (int k = 0; k < 9; k++) Hp[k] = H[k];
        ok[p] = 1;
      }
      continue;
    }
    std::vector<int> R(N + 1);
    for (int g = 0; g <= N; g++) R[g] = update_num_iters(confidence, (double)(N - g) / N, 4, max_iterations);
    int niters = max_iterations, best = 3, best_h = -1;
    double Hb[9];
    std::vector<uint8_t> mask(N), tmp(N);
    for (int h = 0; h < niters; h++) {
      double H[9];
      const int st = sample_model(seed, p, h, N, X1.data(), Y1.data(), X2.data(), Y2.data(), H);
      if (st == 2) break;   // (at h == 0: no model at all)
      if (st == 1) continue;
      int g = 0;
      for (int e = 0; e < N; e++) {
        tmp[e] = h_inlier(H, X1[e], Y1[e], X2[e], Y2[e], th2) ? 1 : 0;
        g += tmp[e];
      }
      if (g > best) {
        best = g; best_h = h;
        mask.swap(tmp);
        for (int k = 0; k < 9; k++) Hb[k] = H[k];
        const int r = R[g];
        if (r < niters) niters = r;
      }
    }
    if (best_h < 0) continue;
    for (int e = 0; e < N; e++) inlier[o + e] = mask[e];
    n_inliers[p] = best;
    ok[p] = 1;
    if (polish) {
      refit(N, X1.data(), Y1.data(), X2.data(), Y2.data(), mask.data(), Hb);
      refine(N, X1.data(), Y1.data(), X2.data(), Y2.data(), mask.data(), Hb);
    }
    for (int k = 0; k < 9; k++) Hp[k] = Hb[k];
  }
  return 0;
}
