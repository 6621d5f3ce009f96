// Batched two-view RANSAC for gfx950: one estimator-independent two-pass core, instantiated for the fundamental matrix (F)
// and for the homography (H).
//
// THE CORE (k_ransac_models / k_ransac_count / k_ransac_select, host driver ransac_two_pass, all templates over an estimator):
//   models   one GPU thread = one sample: the minimal solver, its work matrix in LDS (E::WORK doubles per thread), writes one
//            record per sample (E::Rec: E::MODELS matrices and a status).
//   scoring  one LANE = one correspondence and the model is uniform over the wave: its nine numbers arrive through the scalar
//            cache as SGPR operands, a count is the wave sum of the lanes' inlier flags.  256 threads per block; the pair's
//            correspondences wait in LDS (1 024 at a time), wave w takes samples [32 w, 32 w + 32) of the block's 128 one
//            after the other.  The first form of this file scored with one thread per sample walking all matches, its three
//            models in scratch memory and lanes idle wherever a sample had fewer models: 5.2 ms for the first 128 samples of
//            the 9 120 pairs of 96 images, of which the solver was 0.24.
//   replay   all samples of a range are scored in parallel; one wave per pair then replays OpenCV's sequential loop over the
//            per-sample counts in sample order (the budget shrinks whenever a better model appears: cvRANSACUpdateNumIters,
//            tabulated on the host as R[g] per distinct N), which selects exactly the model the sequential loop would have
//            kept, recomputes it and writes the matrix, the inlier mask, the count and the verdict.
//   two passes  most pairs stop after a few dozen samples: pass 1 scores and replays the first H1 = min(H, 128) samples of
//            every admitted pair; a pair whose budget is still above H1 goes onto the need list (E::TRIM: with its budget), and pass 2
//            scores samples [H1, Hs) for the listed pairs only and replays [0, Hs).  Hs = H, or with E::TRIM the largest
//            listed budget, and then each pair's samples at or past its own budget are not drawn either (`lim`).
// What an estimator carries (everything else is shared):
//    1. sample -> models: E::sample (F: geo_solve7, 0..3 matrices; H: hr_sample, one matrix and a status 0 model, 1 no model,
//       2 no admissible subset in 300 attempts); E::n_models(status).
//    2. count encoding: E::code (F: -1 for a model slot the sample does not have; H: -1 no model, -2 status 2).
//    3. replay: best starts at E::POINTS - 1; with E::HAS_STOP the loop ends at the first -2.
//    4. no winner: mask E::NO_WINNER_MASK everywhere (F 0 with n_inliers 0; H 1 with n_inliers N), zero matrix, ok 0.
//    5. verdict with a winner: E::verdict (F: count >= min_inliers; H: 1).
//    6. inlier predicate: E::inlier (geo_inlier: binary64 compare; hr_inlier: error rounded to binary32, then compared).
//    7. second range: E::TRIM (H scores [H1, Hs) with a per-pair limit; F scores [H1, H) for every deferred pair and has
//       the budget code compiled out: it records no budgets).
//    8. the KTimer class names E::T_SCORE, E::T_REST, E::T_SELECT.
//   In the host wrappers (geo_fransac_dev / geo_hransac_dev), not in the traits:
//    9. admission: F N >= min_points && N >= 8; H N > 4 && (!active || active[p]).
//   10. before the passes F zero-fills the four outputs, H runs k_hransac_small; after them H runs k_hransac_polish if asked.
//   11. H maps threshold <= 0 to 3.0.
//
// F: the geometric-verification stage that follows the ratio tests in the reference's matching loop:
//   GeoVerification::GeoVerificationFundamental   SfM/src/utils/geo_verification.cc:30-58
//     -> cv::findFundamentalMat(pt1, pt2, status, cv::FM_RANSAC, 3.0)   (OpenCV 2.4, not in the tree)
//   called per image pair from FineMatchingGraph::BuildMatchGraph, fine_matching_graph.cc:138-153.
// OpenCV's FM_RANSAC is restated from its published algorithm (CvFMEstimator): 7-point minimal
// solver (null space of the 7x9 epipolar system, cubic det(l F1 + (1-l) F2) = 0, up to three
// models per sample), symmetric squared point-to-epipolar-line error max(d1^2, d2^2) <= 3^2,
// confidence 0.99, at most 2000 samples with the adaptive stop of cvRANSACUpdateNumIters, no final
// refit.  OpenCV's random stream is not reproducible outside OpenCV, so parity with the reference
// is statistical; parity with oracle/ (same counter-based sampler) is exact:
// this file uses only + - * / sqrt on doubles, in a fixed order, with contraction off.
//
// H: cv::findHomography(pts1, pts2, mask, RANSAC, th) of OpenCV 2.4 (cvFindHomography +
// CvHomographyEstimator + CvModelEstimator2::runRANSAC + CvLevMarq), called per image pair by SLAMGPS::FeatureMatching
// step 1 (slam_gps.cc:400-408).  Restated from OpenCV's published source, which is not on this machine; where memory of it
// could be wrong, or where this restatement departs from it on purpose:
//   - sampler: counter based (as geo_solve7), not OpenCV's cvRNG stream; a repeated index is redrawn, a subset with three
//     collinear points in either image (checkSubset, checkPartialSubsets = false: |dx2 dy1 - dy2 dx1| <= FLT_EPSILON
//     (|dx1| + |dy1| + |dx2| + |dy2|)) costs one of 300 attempts; 300 failures end the loop (at sample 0: no model).
//   - model of a sample: OpenCV forms the 9x9 LtL of the normalised DLT rows and takes cvEigenVV's last eigenvector; here
//     the exact 8x9 null space by Gauss-Jordan with full pivoting (the same vector for four points, other rounding).  A
//     sample whose normalisation has a sum of absolute deviations < DBL_EPSILON, whose system is rank deficient, or whose
//     denormalised H is not finite has no model (OpenCV would keep a NaN / inf model that scores 0 and never wins).
//   - N == 4 (cvFindHomography's direct fit, no RANSAC): the same exact null space on the four points in their order; a
//     rank-deficient system (four collinear points, say) or a non-finite H gives ok = 0 with the mask of ones.  OpenCV's
//     runKernel returns 1 there for any set whose spreads are >= DBL_EPSILON, with the LtL eigenvector it finds: a departure,
//     unlike the "no model" of a RANSAC sample (which could only ever score 0 and never win).
//   - H is scaled by division by H[8] (OpenCV multiplies by 1 / H[8]), so that H[8] = 1 exactly.
//   - error: err = (float)(dx^2 + dy^2) of the transfer into image 2 with ww = 1 / (h6 x + h7 y + 1), inlier iff
//     (double)err <= th^2 - OpenCV keeps err in a CV_32F row and compares it with the double threshold^2.
//   - stop: a sample wins if good > max(best, 3); niters = cvRANSACUpdateNumIters(0.995, (N - good) / N, 4, niters),
//     tabulated per distinct N on the host with max_iters = the option's limit and capped by the current niters.
//   - polish (cvFindHomography after a successful RANSAC): refit on the inliers (LtL summed over them, eigenvector of its
//     smallest eigenvalue by cyclic Jacobi - OpenCV's Jacobi picks the largest off-diagonal pivot instead), then CvLevMarq
//     for 10 iterations on h0..h7: lambda = 10^k as the decimal literal (OpenCV: exp(k ln 10)), diagonal times (1 + lambda),
//     the step by the eigen-decomposition of the damped 8x8 (OpenCV: cvSVD + cvSVBkSb, singular values <= 2 eps sum(w)
//     dropped), stop after 10 iterations or when |dp| / (|p| + DBL_EPSILON) < DBL_EPSILON.  Sums over the inliers run in
//     the polish kernel's order: lane l of a wave takes correspondences l, l + 64, ... ascending, then the butterfly
//     d = 32 .. 1 (tests/hransac_ref.cpp restates it); OpenCV sums the compressed inliers in index order.
//   - the mask is that of the best sample's model, not recomputed after the polish (as OpenCV returns it).
// Beside the core the H path has k_hransac_small (pairs of at most four correspondences and pairs the caller left out)
// and k_hransac_polish, one wave per pair each.
#include "common.h"

#include <cfloat>
#include <mutex>
#include <unordered_map>
#include <cmath>

#pragma clang fp contract(off)

#define GEO_WAVE 64

__device__ static inline double geo_det3(const double* m) {
  return m[0] * (m[4] * m[8] - m[5] * m[7]) - m[1] * (m[3] * m[8] - m[5] * m[6]) + m[2] * (m[3] * m[7] - m[4] * m[6]);
}
__device__ static inline void geo_cof3(const double* m, double* c) {
  c[0] = m[4] * m[8] - m[5] * m[7];
  c[1] = -(m[3] * m[8] - m[5] * m[6]);
  c[2] = m[3] * m[7] - m[4] * m[6];
  c[3] = -(m[1] * m[8] - m[2] * m[7]);
  c[4] = m[0] * m[8] - m[2] * m[6];
  c[5] = -(m[0] * m[7] - m[1] * m[6]);
  c[6] = m[1] * m[5] - m[2] * m[4];
  c[7] = -(m[0] * m[5] - m[2] * m[3]);
  c[8] = m[0] * m[4] - m[1] * m[3];
}

// Real roots of c3 x^3 + c2 x^2 + c1 x + c0 by bisection inside the Cauchy bound, two Newton
// steps and deflation: arithmetic and sqrt only, so that host and device agree to the last bit.
__device__ static inline int geo_cubic(double c3, double c2, double c1, double c0, double* roots) {
  const double a = c2 / c3, b = c1 / c3, c = c0 / c3;
  if (!(fabs(a) <= DBL_MAX && fabs(b) <= DBL_MAX && fabs(c) <= DBL_MAX)) {
    // not a cubic (c3 == 0 or overflow): at most the quadratic / linear roots
    if (c2 != 0.0) {
      const double p = c1 / c2, q = c0 / c2, disc = p * p - 4.0 * q;
      if (!(disc >= 0.0)) return 0;
      const double sq = sqrt(disc), t = -0.5 * (p + (p >= 0.0 ? sq : -sq));
      int n = 0;
      roots[n++] = t;
      if (t != 0.0) roots[n++] = q / t;
      return n;
    }
    if (c1 != 0.0) { roots[0] = -c0 / c1; return 1; }
    return 0;
  }
  double R = fabs(a);
  if (fabs(b) > R) R = fabs(b);
  if (fabs(c) > R) R = fabs(c);
  R = 1.0 + R;
  double lo = -R, hi = R;
  for (int it = 0; it < 100; it++) {
    const double mid = 0.5 * (lo + hi);
    const double f = ((mid + a) * mid + b) * mid + c;
    if (f <= 0.0) lo = mid; else hi = mid;
  }
  double r = 0.5 * (lo + hi);
  for (int it = 0; it < 2; it++) {
    const double f = ((r + a) * r + b) * r + c;
    const double fp = (3.0 * r + 2.0 * a) * r + b;
    if (fp != 0.0) {
      const double rn = r - f / fp;
      if (fabs(rn) <= DBL_MAX) r = rn;
    }
  }
  int n = 0;
  roots[n++] = r;
  const double p = a + r, q = b + r * p, disc = p * p - 4.0 * q;
  if (disc >= 0.0) {
    const double sq = sqrt(disc), t = -0.5 * (p + (p >= 0.0 ? sq : -sq));
    roots[n++] = t;
    if (t != 0.0) roots[n++] = q / t;
  }
  return n;
}

// The 7-point solver for sample `h` of pair `pair`.  A: this thread's 7x9 work matrix, element
// (r, c) at A[(r * 9 + c) * stride]  (LDS, one column of a [63][stride] array per thread).  Returns the number of
// models (0..3) and writes them to M[0..].
__device__ static inline int geo_solve7(uint64_t seed, int pair, int h, int N, const float2* __restrict__ p1,
                                          const float2* __restrict__ p2, double* A, int stride, double (*M)[9]) {
  int n = 0;
  uint64_t s = seed ^ ((uint64_t)pair * 0xD1342543DE82EF95ull) ^ ((uint64_t)h * 0xA24BAED4963EE407ull);
  int idx[7];
  for (int k = 0; k < 7; k++) {
    for (;;) {
      const int v = (int)(sm64(s) % (uint64_t)N);
      bool dup = false;
      for (int j = 0; j < k; j++) dup = dup || (idx[j] == v);
      if (!dup) { idx[k] = v; break; }
    }
  }
#define AT(r, c) A[((r) * 9 + (c)) * stride]
  for (int k = 0; k < 7; k++) {
    const double x1 = p1[idx[k]].x, y1 = p1[idx[k]].y, x2 = p2[idx[k]].x, y2 = p2[idx[k]].y;
    AT(k, 0) = x2 * x1; AT(k, 1) = x2 * y1; AT(k, 2) = x2;
    AT(k, 3) = y2 * x1; AT(k, 4) = y2 * y1; AT(k, 5) = y2;
    AT(k, 6) = x1; AT(k, 7) = y1; AT(k, 8) = 1.0;
  }
  int perm[9];
  for (int c = 0; c < 9; c++) perm[c] = c;
  // Gauss-Jordan with full pivoting (first maximum in row-major order)
  for (int i = 0; i < 7; i++) {
    int pr = i, pc = i;
    double best = -1.0;
    for (int r = i; r < 7; r++)
      for (int c = i; c < 9; c++) {
        const double v = fabs(AT(r, c));
        if (v > best) { best = v; pr = r; pc = c; }
      }
    if (!(best > 0.0)) return 0;  // degenerate sample (or NaN input): no model
    if (pr != i)
      for (int c = 0; c < 9; c++) { const double t = AT(i, c); AT(i, c) = AT(pr, c); AT(pr, c) = t; }
    if (pc != i) {
      for (int r = 0; r < 7; r++) { const double t = AT(r, i); AT(r, i) = AT(r, pc); AT(r, pc) = t; }
      // perm lives in registers: swap by value
      int pi = 0, pp = 0;
      for (int c = 0; c < 9; c++) { if (c == i) pi = perm[c]; if (c == pc) pp = perm[c]; }
      for (int c = 0; c < 9; c++) { if (c == i) perm[c] = pp; else if (c == pc) perm[c] = pi; }
    }
    const double piv = AT(i, i);
    for (int c = i; c < 9; c++) AT(i, c) = AT(i, c) / piv;
    for (int r = 0; r < 7; r++) {
      if (r == i) continue;
      const double f = AT(r, i);
      for (int c = i; c < 9; c++) AT(r, c) = AT(r, c) - f * AT(i, c);
    }
  }
  // null space: x = (-B[:,k], e_k) in the permuted column order
  double f1[9], f2[9];
  for (int j = 0; j < 9; j++) {
    const double xa = j < 7 ? -AT(j, 7) : (j == 7 ? 1.0 : 0.0);
    const double xb = j < 7 ? -AT(j, 8) : (j == 8 ? 1.0 : 0.0);
    for (int c = 0; c < 9; c++)
      if (c == perm[j]) { f1[c] = xa; f2[c] = xb; }
  }
#undef AT
  double G[9], cf[9];
  for (int k = 0; k < 9; k++) G[k] = f1[k] - f2[k];
  const double c0 = geo_det3(f2), c3 = geo_det3(G);
  geo_cof3(f2, cf);
  double c1 = 0.0;
  for (int k = 0; k < 9; k++) c1 = c1 + cf[k] * G[k];
  geo_cof3(G, cf);
  double c2 = 0.0;
  for (int k = 0; k < 9; k++) c2 = c2 + cf[k] * f2[k];
  double roots[3];
  const int nr = geo_cubic(c3, c2, c1, c0, roots);
  for (int q = 0; q < nr; q++) {
    const double lam = roots[q];
    double F[9];
    bool fin = true;
    for (int k = 0; k < 9; k++) { F[k] = f2[k] + lam * G[k]; fin = fin && (fabs(F[k]) <= DBL_MAX); }
    if (!fin) continue;
    const double mu = F[8];
    if (fabs(mu) > DBL_EPSILON) {
      const double inv = 1.0 / mu;
      for (int k = 0; k < 9; k++) F[k] = F[k] * inv;
    }
    for (int k = 0; k < 9; k++) M[n][k] = F[k];
    n++;
  }
  return n;
}

// max(d1^2 / |l1|^2, d2^2 / |l2|^2) with l2 = F x1 (line in image 2), l1 = F^T x2
__device__ static inline bool geo_inlier(const double* F, double x1, double y1, double x2, double y2, double th2) {
  double a = F[0] * x1 + F[1] * y1 + F[2];
  double b = F[3] * x1 + F[4] * y1 + F[5];
  double c = F[6] * x1 + F[7] * y1 + F[8];
  const double s2 = 1.0 / (a * a + b * b);
  const double d2 = x2 * a + y2 * b + c;
  a = F[0] * x2 + F[3] * y2 + F[6];
  b = F[1] * x2 + F[4] * y2 + F[7];
  c = F[2] * x2 + F[5] * y2 + F[8];
  const double s1 = 1.0 / (a * a + b * b);
  const double d1 = x1 * a + y1 * b + c;
  const double e1 = d1 * d1 * s1, e2 = d2 * d2 * s2;
  const double err = e1 > e2 ? e1 : e2;
  return err <= th2;  // false for NaN
}

__device__ static inline bool hr_check_subset(const double* x, const double* y) {
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

__device__ static inline bool hr_denormalise(const double* H0, double csx, double csy, double cx, double cy, double sMx, double sMy,
                                             double cMx, double cMy, double* H) {
  const double a[9] = {1.0 / csx, 0.0, cx, 0.0, 1.0 / csy, cy, 0.0, 0.0, 1.0};
  const double b[9] = {sMx, 0.0, -cMx * sMx, 0.0, sMy, -cMy * sMy, 0.0, 0.0, 1.0};
  double t[9], u[9];
#pragma unroll
  for (int i = 0; i < 3; i++)
#pragma unroll
    for (int j = 0; j < 3; j++) {
      double s = a[i * 3 + 0] * H0[0 * 3 + j];
      s = s + a[i * 3 + 1] * H0[1 * 3 + j];
      s = s + a[i * 3 + 2] * H0[2 * 3 + j];
      t[i * 3 + j] = s;
    }
#pragma unroll
  for (int i = 0; i < 3; i++)
#pragma unroll
    for (int j = 0; j < 3; j++) {
      double s = t[i * 3 + 0] * b[0 * 3 + j];
      s = s + t[i * 3 + 1] * b[1 * 3 + j];
      s = s + t[i * 3 + 2] * b[2 * 3 + j];
      u[i * 3 + j] = s;
    }
  bool fin = true;
#pragma unroll
  for (int k = 0; k < 8; k++) { H[k] = u[k] / u[8]; fin = fin && fabs(H[k]) <= DBL_MAX; }
  H[8] = 1.0;
  return fin;
}

// The exact homography of four correspondences; A: the 8x9 work matrix, element (r, c) at A[(r * 9 + c) * stride].
__device__ static inline bool hr_solve4(const double* X1, const double* Y1, const double* X2, const double* Y2, double* A, int stride,
                                        double* H) {
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
#define AT(r, c) A[((r) * 9 + (c)) * stride]
  for (int i = 0; i < 4; i++) {
    const double x = (X2[i] - cx) * sx, y = (Y2[i] - cy) * sy;
    const double X = (X1[i] - cMx) * sMx, Y = (Y1[i] - cMy) * sMy;
    const double lx[9] = {X, Y, 1.0, 0.0, 0.0, 0.0, -x * X, -x * Y, -x};
    const double ly[9] = {0.0, 0.0, 0.0, X, Y, 1.0, -y * X, -y * Y, -y};
#pragma unroll
    for (int c = 0; c < 9; c++) { AT(2 * i, c) = lx[c]; AT(2 * i + 1, c) = ly[c]; }
  }
  int perm[9];
  for (int c = 0; c < 9; c++) perm[c] = c;
  for (int i = 0; i < 8; i++) {
    int pr = i, pc = i;
    double best = -1.0;
    for (int r = i; r < 8; r++)
      for (int c = i; c < 9; c++) {
        const double v = fabs(AT(r, c));
        if (v > best) { best = v; pr = r; pc = c; }
      }
    if (!(best > 0.0)) return false;
    if (pr != i)
      for (int c = 0; c < 9; c++) { const double t = AT(i, c); AT(i, c) = AT(pr, c); AT(pr, c) = t; }
    if (pc != i) {
      for (int r = 0; r < 8; r++) { const double t = AT(r, i); AT(r, i) = AT(r, pc); AT(r, pc) = t; }
      int pi = 0, pp = 0;   // perm lives in registers: swap by value
      for (int c = 0; c < 9; c++) { if (c == i) pi = perm[c]; if (c == pc) pp = perm[c]; }
      for (int c = 0; c < 9; c++) { if (c == i) perm[c] = pp; else if (c == pc) perm[c] = pi; }
    }
    const double piv = AT(i, i);
    for (int c = i; c < 9; c++) AT(i, c) = AT(i, c) / piv;
    for (int r = 0; r < 8; r++) {
      if (r == i) continue;
      const double f = AT(r, i);
      for (int c = i; c < 9; c++) AT(r, c) = AT(r, c) - f * AT(i, c);
    }
  }
  double h0[9];
  for (int j = 0; j < 9; j++) {
    const double v = j < 8 ? -AT(j, 8) : 1.0;
    for (int c = 0; c < 9; c++)
      if (c == perm[j]) h0[c] = v;
  }
#undef AT
  return hr_denormalise(h0, sx, sy, cx, cy, sMx, sMy, cMx, cMy, H);
}

// Cyclic Jacobi on a symmetric n x n (n <= 9) in memory the caller owns (LDS): w eigenvalues, V column k eigenvector k.
__device__ static void hr_jacobi(double* A, int n, double* w, double* V) {
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

__constant__ double hr_lambda[33] = {1e-16, 1e-15, 1e-14, 1e-13, 1e-12, 1e-11, 1e-10, 1e-9, 1e-8, 1e-7, 1e-6, 1e-5, 1e-4, 1e-3, 1e-2, 1e-1, 1e0,
                                     1e1,   1e2,   1e3,   1e4,   1e5,   1e6,   1e7,   1e8,   1e9,   1e10, 1e11, 1e12, 1e13, 1e14, 1e15, 1e16};

// CvLevMarq::step in LDS (lane 0): JtJ upper [36], A / V [64] scratch
__device__ static void hr_lm_step(const double* prev, const double* JtJ, const double* JtErr, int lam, double* A, double* V, double* param) {
  double w[8];
  int e = 0;
  for (int j = 0; j < 8; j++)
    for (int k = j; k < 8; k++) { A[j * 8 + k] = JtJ[e]; A[k * 8 + j] = JtJ[e]; e++; }
  const double f = 1.0 + hr_lambda[lam + 16];
  for (int j = 0; j < 8; j++) A[j * 8 + j] = A[j * 8 + j] * f;
  double wl[8];
  hr_jacobi(A, 8, wl, V);
  for (int k = 0; k < 8; k++) w[k] = wl[k];
  int ord[8];
  for (int k = 0; k < 8; k++) ord[k] = k;
  for (int k = 0; k < 7; k++) {
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

__device__ static inline bool hr_inlier(const double* H, double x1, double y1, double x2, double y2, double th2) {
  const double ww = 1.0 / (H[6] * x1 + H[7] * y1 + 1.0);
  const double dx = (H[0] * x1 + H[1] * y1 + H[2]) * ww - x2;
  const double dy = (H[3] * x1 + H[4] * y1 + H[5]) * ww - y2;
  const float err = (float)(dx * dx + dy * dy);
  return (double)err <= th2;   // false for NaN
}

// sample h of pair `pair`: 0 = model in H, 1 = no model, 2 = no admissible subset in 300 attempts
__device__ static inline int hr_sample(uint64_t seed, int pair, int h, int N, const float2* __restrict__ p1, const float2* __restrict__ p2,
                                       double* A, int stride, double* H) {
  uint64_t s = seed ^ ((uint64_t)pair * 0xD1342543DE82EF95ull) ^ ((uint64_t)h * 0xA24BAED4963EE407ull);
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
#pragma unroll
    for (int k = 0; k < 4; k++) {
      const float2 u = p1[idx[k]], v = p2[idx[k]];
      a1[k] = u.x; b1[k] = u.y; a2[k] = v.x; b2[k] = v.y;
    }
    if (!hr_check_subset(a1, b1) || !hr_check_subset(a2, b2)) continue;
    return hr_solve4(a1, b1, a2, b2, A, stride, H) ? 0 : 1;
  }
  return 2;
}

// ---- the estimators (the header comment lists what each member stands for) ----
struct FEstimator {
  static constexpr int POINTS = 7, MODELS = 3, WORK = 63;   // WORK: the 7x9 matrix of geo_solve7
  static constexpr int NO_MODEL = 0;                        // the status is the number of models
  static constexpr bool HAS_STOP = false, TRIM = false;
  static constexpr int NO_WINNER_MASK = 0;
  static constexpr const char *T_SCORE = "geo_fransac_score", *T_REST = "geo_fransac_score_rest", *T_SELECT = "geo_fransac_select";
  struct Rec { double M[3][9]; int st, pad; };
  __device__ static inline int sample(uint64_t seed, int pair, int h, int N, const float2* __restrict__ p1, const float2* __restrict__ p2,
                                      double* A, int stride, double (*M)[9]) {
    return geo_solve7(seed, pair, h, N, p1, p2, A, stride, M);
  }
  __device__ static inline int n_models(int st) { return st; }
  __device__ static inline int code(int st, int q, int c) { return q < st ? c : -1; }
  __device__ static inline bool inlier(const double* F, double x1, double y1, double x2, double y2, double th2) {
    return geo_inlier(F, x1, y1, x2, y2, th2);
  }
  __device__ static inline int verdict(int c, int min_inliers) { return c >= min_inliers ? 1 : 0; }   // match_inliers.size() < 30 -> false
};

struct HEstimator {
  static constexpr int POINTS = 4, MODELS = 1, WORK = 72;   // WORK: the 8x9 matrix of hr_solve4
  static constexpr int NO_MODEL = 1;                        // the status is hr_sample's
  static constexpr bool HAS_STOP = true, TRIM = true;
  static constexpr int NO_WINNER_MASK = 1;
  static constexpr const char *T_SCORE = "geo_hransac_score", *T_REST = "geo_hransac_score_rest", *T_SELECT = "geo_hransac_select";
  struct Rec { double M[1][9]; int st, pad; };
  __device__ static inline int sample(uint64_t seed, int pair, int h, int N, const float2* __restrict__ p1, const float2* __restrict__ p2,
                                      double* A, int stride, double (*M)[9]) {
    return hr_sample(seed, pair, h, N, p1, p2, A, stride, M[0]);
  }
  __device__ static inline int n_models(int st) { return st == 0 ? 1 : 0; }
  __device__ static inline int code(int st, int q, int c) { return st == 0 ? c : -st; }
  __device__ static inline bool inlier(const double* H, double x1, double y1, double x2, double y2, double th2) {
    return hr_inlier(H, x1, y1, x2, y2, th2);
  }
  __device__ static inline int verdict(int, int) { return 1; }
};

// The three kernels are `static`: the LDS arrays of a template kernel otherwise get linkonce linkage, which keeps the
// compiler from trimming them (k_ransac_select then takes 16 / 24 bytes more than it needs).

// The models of samples [h0, h1) of the pairs in `slot_pair`: grid (ceil((h1 - h0) / 64), n_slots), thread = sample.
// models[slot][h - h0]: the sample's record.  lim (may be NULL): row y's budget; samples at or past it can never be replayed
// and are written as "no model" without being drawn (the scoring skips them).  Compiled in with E::TRIM only.
template <class E>
static __global__ __launch_bounds__(GEO_WAVE) void k_ransac_models(int h0, int h1, const int* __restrict__ slot_pair, const int* __restrict__ lim,
                                                             const int* __restrict__ off, const float2* __restrict__ pt1,
                                                             const float2* __restrict__ pt2, uint64_t seed, typename E::Rec* __restrict__ models) {
  __shared__ double A[E::WORK * GEO_WAVE];
  const int slot = blockIdx.y, pair = slot_pair[slot], h = h0 + blockIdx.x * GEO_WAVE + threadIdx.x;
  const int o = off[pair], N = off[pair + 1] - o;
  if (h >= h1) return;
  double M[E::MODELS][9];
  const int st = E::TRIM && lim && h >= lim[slot] ? E::NO_MODEL : E::sample(seed, pair, h, N, pt1 + o, pt2 + o, A + threadIdx.x, GEO_WAVE, M);
  typename E::Rec* r = models + (size_t)slot * (h1 - h0) + (h - h0);
  for (int q = 0; q < E::MODELS; q++)
    for (int k = 0; k < 9; k++) r->M[q][k] = q < E::n_models(st) ? M[q][k] : 0.0;
  r->st = st;
  r->pad = 0;
}

// Inlier counts of those models: grid (ceil((h1 - h0) / 128), n_slots), 256 threads; the pair's correspondences wait in LDS
// (1024 at a time), wave w takes samples [32 w, 32 w + 32) of the block's 128 one after the other, lane = correspondence.
// counts[slot][cs samples][E::MODELS] (E::code): this launch's samples start at sample `co` of a slot's row (a range taken
// in several pieces shares one array).
#define GEO_CNT_SAMPLES 128
template <class E>
static __global__ __launch_bounds__(256) void k_ransac_count(int h0, int h1, const int* __restrict__ slot_pair, const int* __restrict__ lim,
                                                       const int* __restrict__ off, const float2* __restrict__ pt1, const float2* __restrict__ pt2,
                                                       double th2, const typename E::Rec* __restrict__ models, int* __restrict__ counts, int cs, int co) {
  __shared__ float4 pts[1024];
  __shared__ int cnt_s[GEO_CNT_SAMPLES * E::MODELS];
  const int slot = blockIdx.y, pair = slot_pair[slot];
  const int o = off[pair], N = off[pair + 1] - o;
  const int HS = h1 - h0;
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
  const int s_first = blockIdx.x * GEO_CNT_SAMPLES + 32 * wave;   // first sample (relative to h0) of this wave
  if (E::TRIM && lim && h0 + (int)blockIdx.x * GEO_CNT_SAMPLES >= lim[slot]) {   // every sample of this block is past the budget
    for (int e = threadIdx.x; e < GEO_CNT_SAMPLES * E::MODELS; e += 256) {
      const int hs = blockIdx.x * GEO_CNT_SAMPLES + e / E::MODELS, q = e % E::MODELS;
      if (hs < HS) counts[((size_t)slot * cs + co + hs) * E::MODELS + q] = E::code(E::NO_MODEL, q, 0);
    }
    return;
  }
  for (int e = threadIdx.x; e < GEO_CNT_SAMPLES * E::MODELS; e += 256) cnt_s[e] = 0;
  for (int base = 0; base < N; base += 1024) {
    const int nb = min(1024, N - base);
    __syncthreads();
    for (int e = threadIdx.x; e < nb; e += 256) {
      const float2 a = pt1[o + base + e], b = pt2[o + base + e];
      pts[e] = make_float4(a.x, a.y, b.x, b.y);
    }
    __syncthreads();
    for (int j = 0; j < 32; j++) {
      const int hs = s_first + j;
      if (hs >= HS) break;
      const typename E::Rec* r = models + (size_t)slot * HS + hs;   // (uniform over the wave: scalar loads)
      const int nm = E::n_models(r->st);
      for (int q = 0; q < nm; q++) {
        double F[9];
#pragma unroll
        for (int k = 0; k < 9; k++) F[k] = r->M[q][k];
        int c = 0;
        for (int e = lane; e < nb; e += 64) {
          const float4 p = pts[e];
          c += E::inlier(F, p.x, p.y, p.z, p.w, th2) ? 1 : 0;
        }
        c = wave_sum_int(c);
        if (lane == 0) cnt_s[(32 * wave + j) * E::MODELS + q] += c;   // (only this wave touches these entries)
      }
    }
  }
  __syncthreads();
  for (int e = threadIdx.x; e < GEO_CNT_SAMPLES * E::MODELS; e += 256) {
    const int hs = blockIdx.x * GEO_CNT_SAMPLES + e / E::MODELS, q = e % E::MODELS;
    if (hs < HS) counts[((size_t)slot * cs + co + hs) * E::MODELS + q] = E::code(models[(size_t)slot * HS + hs].st, q, cnt_s[e]);
  }
}

// One wave per pair: replay the sequential loop over the counts, recompute the winning sample's model, write the matrix
// (H: unpolished), the mask, n_inliers and the verdict.  H = max_iterations (the loop's first budget); pass 1 (grid = the
// admitted pairs, `slot_pair`) replays samples [0, H1) and, for a pair whose budget b is still above H1, appends it to
// need_list and (E::TRIM) records b in need_budget and raises *need_max to b; the others are final.  Pass 2 (grid = that
// list) replays [0, Hs): the replay of [0, H1) reaches the same budget b <= Hs again, and the budget only shrinks, so no sample at or past
// Hs can be reached; counts2 holds samples [H1, Hs) of the k-th listed pair at row k.
template <class E>
static __global__ __launch_bounds__(GEO_WAVE) void k_ransac_select(int H, int Hs, int H1, int pass, const int* __restrict__ slot_pair, int* __restrict__ need_list,
                                                             int* __restrict__ need_count, int* __restrict__ need_max, int* __restrict__ need_budget,
                                                             const int* __restrict__ off, const float2* __restrict__ pt1,
                                                             const float2* __restrict__ pt2, uint64_t seed, double th2, int min_inliers,
                                                             const int* __restrict__ counts1, const int* __restrict__ counts2,
                                                             const int* __restrict__ niters_tab, const int* __restrict__ tab_off, double* __restrict__ Mout,
                                                             uint8_t* __restrict__ inlier, int* __restrict__ n_inliers, uint8_t* __restrict__ ok) {
  __shared__ double A[E::WORK];
  __shared__ double Mw[9];
  __shared__ int win[3];
  __shared__ int cl[E::MODELS * 1024];
  const int lane = threadIdx.x;
  if (pass == 2 && (int)blockIdx.x >= *need_count) return;
  const int slot = pass == 2 ? need_list[blockIdx.x] : (int)blockIdx.x;
  const int pair = slot_pair[slot];
  const int o = off[pair], N = off[pair + 1] - o;
  const int Hscan = pass == 1 ? H1 : Hs;
  if (lane == 0) { win[0] = -1; win[1] = 0; win[2] = H; }
  {
    const int* R = niters_tab + tab_off[pair];  // N + 1 entries (the table of this N)
    int best = E::POINTS - 1;                   // a model must beat modelPoints - 1
    for (int h0 = 0; h0 < Hscan; h0 += 1024) {
      __syncthreads();
      if (h0 >= win[2]) break;  // uniform: win[2] is shared
      const int nh = min(1024, Hscan - h0);
      for (int e = lane; e < E::MODELS * nh; e += GEO_WAVE) {
        const int h = h0 + e / E::MODELS, q = e % E::MODELS;
        cl[e] = h < H1 ? counts1[((size_t)slot * H1 + h) * E::MODELS + q]
                       : counts2[((size_t)blockIdx.x * (Hs - H1) + (h - H1)) * E::MODELS + q];
      }
      __syncthreads();
      if (lane == 0) {
        int niters = win[2];
        for (int h = h0; h < h0 + nh && h < niters; h++)
          for (int q = 0; q < E::MODELS; q++) {
            const int g = cl[(h - h0) * E::MODELS + q];
            // getSubset failed: the loop over h ends (at h = 0 without a model) - niters = h stops it, `break` only leaves the q loop
            if (E::HAS_STOP && g == -2) { niters = h; break; }
            if (g > best) {
              best = g; win[0] = h; win[1] = q;
              const int r = R[g];
              if (r < niters) niters = r;
            }
          }
        win[2] = niters;
      }
    }
  }
  __syncthreads();
  if (pass == 1) {
    const bool more = win[2] > H1 && H1 < H;  // the sequential loop would have gone on past H1
    if (more) {
      if (lane == 0) {
        const int k = atomicAdd(need_count, 1);
        need_list[k] = slot;
        if (E::TRIM) {   // (an estimator that does not trim records nothing: profiles/ransac_core_ab.jsonl, the variant lines, has the cost)
          need_budget[k] = win[2];
          atomicMax(need_max, win[2]);
        }
      }
      return;
    }
  }
  const int wh = win[0];
  if (wh < 0) {
    for (int e = lane; e < N; e += GEO_WAVE) inlier[o + e] = E::NO_WINNER_MASK;
    if (lane == 0) {
      for (int k = 0; k < 9; k++) Mout[(size_t)pair * 9 + k] = 0.0;
      n_inliers[pair] = E::NO_WINNER_MASK ? N : 0;
      ok[pair] = 0;
    }
    return;
  }
  if (lane == 0) {
    double M[E::MODELS][9];
    E::sample(seed, pair, wh, N, pt1 + o, pt2 + o, A, 1, M);
    for (int k = 0; k < 9; k++) { Mw[k] = M[E::MODELS > 1 ? win[1] : 0][k]; Mout[(size_t)pair * 9 + k] = Mw[k]; }
  }
  __syncthreads();
  double F[9];
  for (int k = 0; k < 9; k++) F[k] = Mw[k];
  int c = 0;
  for (int e = lane; e < N; e += GEO_WAVE) {
    const float2 a = pt1[o + e], b = pt2[o + e];
    const bool in = E::inlier(F, a.x, a.y, b.x, b.y, th2);
    inlier[o + e] = in ? 1 : 0;
    c += in ? 1 : 0;
  }
  c = wave_sum_int(c);
  if (lane == 0) {
    n_inliers[pair] = c;
    ok[pair] = E::verdict(c, min_inliers);
  }
}

// l = F [x1, y1, 1]; l /= hypot(l0, l1); inlier iff |l . [x2, y2, 1]| < th   (geo_verification.cc:60-79),
// for every pair whose F was accepted.
__global__ __launch_bounds__(256) void k_epipolar_batch(int total, const int* __restrict__ pair_of, const float2* __restrict__ pt1,
                                                         const float2* __restrict__ pt2, const double* __restrict__ F,
                                                         const uint8_t* __restrict__ ok, double th, uint8_t* __restrict__ inlier) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= total) return;
  const int p = pair_of[e];
  if (ok && !ok[p]) { inlier[e] = 0; return; }
  const double* f = F + (size_t)p * 9;
  const double x1 = pt1[e].x, y1 = pt1[e].y, x2 = pt2[e].x, y2 = pt2[e].y;
  double l0 = f[0] * x1 + f[1] * y1 + f[2];
  double l1 = f[3] * x1 + f[4] * y1 + f[5];
  double l2 = f[6] * x1 + f[7] * y1 + f[8];
  const double n = sqrt(l0 * l0 + l1 * l1);
  l0 = l0 / n; l1 = l1 / n; l2 = l2 / n;
  const double dis = l0 * x2 + l1 * y2 + l2;
  inlier[e] = fabs(dis) < th ? 1 : 0;
}

__global__ void k_gather_int(int n, const int* __restrict__ idx, const int* __restrict__ src, int* __restrict__ dst) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) dst[i] = src[idx[i]];
}

// cvRANSACUpdateNumIters(p, ep, model_points, max_iters) for ep = (N - g) / N, clamped to max_iters
static int geo_update_num_iters(double p, double ep, int model_points, int max_iters) {
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

// R[g] = cvRANSACUpdateNumIters(confidence, (N - g) / N, E::POINTS, H) for g inliers of N: a pow and two logs per entry.  The
// table of a pair depends on its N alone, so one table per DISTINCT N is formed (and kept from call to call while confidence
// and sample limit stay the same: the matching loop verifies thousands of pairs with one set of options) - at 9 120 pairs of
// ~125 good matches each the per-pair tables were 1.1 M evaluations, 7 of the 15 ms of msfm_chain_verify on sixteen host
// threads.  tab: the tables of this call's admitted pairs back to back, tab_off[p]: where pair p's begins (0 for a pair that
// is not admitted: the kernels do not look at its table).  One cache per estimator (the static below).
template <class E>
static void ransac_iter_tables(double confidence, int H, int n_pairs, const int* offsets, const std::vector<int>& slot_pair,
                               std::vector<int>& tab, std::vector<int>& tab_off) {
  struct TabCache { std::mutex mu; double conf = -1.0; int H = -1; std::unordered_map<int, std::vector<int>> by_n; size_t entries = 0; };
  static TabCache cache;
  tab.clear();
  tab_off.assign(std::max(1, n_pairs), 0);
  std::lock_guard<std::mutex> lock(cache.mu);
  if (cache.conf != confidence || cache.H != H || cache.entries > (size_t)32 << 20) {
    cache.by_n.clear(); cache.entries = 0; cache.conf = confidence; cache.H = H;
  }
  std::vector<int> missing;
  for (int p : slot_pair) {
    const int N = offsets[p + 1] - offsets[p];
    if (cache.by_n.find(N) == cache.by_n.end()) { cache.by_n[N]; missing.push_back(N); }
  }
  std::vector<std::vector<int>*> slot(missing.size());
  for (size_t k = 0; k < missing.size(); k++) { slot[k] = &cache.by_n[missing[k]]; slot[k]->resize((size_t)missing[k] + 1); cache.entries += (size_t)missing[k] + 1; }
  par_ranges(missing.size(), host_threads(), [&](int, size_t k0, size_t k1) {
    for (size_t k = k0; k < k1; k++) {
      const int N = missing[k];
      int* R = slot[k]->data();
      for (int g = 0; g <= N; g++) R[g] = geo_update_num_iters(confidence, (double)(N - g) / N, E::POINTS, H);
    }
  }, 4);
  std::unordered_map<int, int> at;   // N -> offset of its table in this call's upload
  for (int p : slot_pair) {
    const int N = offsets[p + 1] - offsets[p];
    auto it = at.find(N);
    if (it == at.end()) {
      it = at.emplace(N, (int)tab.size()).first;
      const std::vector<int>& R = cache.by_n[N];
      tab.insert(tab.end(), R.begin(), R.end());
    }
    tab_off[p] = it->second;
  }
  if (tab.empty()) tab.push_back(H);   // (no admitted pair: the upload is never empty)
}

struct RansacRun { int H; double confidence, th2; uint64_t seed; int min_inliers; };
// The device buffers of one run.  The driver only enqueues: its caller declares these in front of its scope.
template <class E>
struct RansacWork {
  DevBuf<int> tab_off, tab, slot_pair, need, budget, counts1, counts2, need_pair;
  DevBuf<typename E::Rec> models1, models2;
};

// The two passes for the pairs in slot_pair (not empty) on points that are already resident: d_off (device) and offsets (host)
// delimit the pairs' correspondences in p1 / p2; the results of the listed pairs go to dM, d_in, d_nin, d_ok.  Ends with
// work enqueued on the stream (after a second pass: with that pass enqueued).
template <class E>
static int ransac_two_pass(msfm_ctx* ctx, const RansacRun& run, int n_pairs, const int* offsets, const int* d_off, const float2* p1,
                           const float2* p2, const std::vector<int>& slot_pair, RansacWork<E>& w, double* dM, uint8_t* d_in, int* d_nin,
                           uint8_t* d_ok) {
  hipStream_t s = ctx->stream;
  const int H = run.H, n_slots = (int)slot_pair.size();
  std::vector<int> tab, tab_off;
  ransac_iter_tables<E>(run.confidence, H, n_pairs, offsets, slot_pair, tab, tab_off);
  HIP_TRY(ctx, w.tab_off.from(tab_off, s));
  HIP_TRY(ctx, w.tab.from(tab, s));
  // Most pairs stop after a few dozen samples (cvRANSACUpdateNumIters): score the first H1 samples of every pair,
  // replay them, and run the remaining samples only for the pairs whose budget is still open.
  const int H1 = std::min(H, 128);
  HIP_TRY(ctx, w.slot_pair.from(slot_pair, s));
  HIP_TRY(ctx, w.need.alloc((size_t)n_slots + 2));   // [0]: how many, [1]: their largest budget, [2..]: the slots
  if (E::TRIM) HIP_TRY(ctx, w.budget.alloc(n_slots));   // the budget of each listed slot after pass 1 (without E::TRIM: none, and [1] stays 0)
  HIP_TRY(ctx, hipMemsetAsync(w.need.p, 0, 2 * sizeof(int), s));
  HIP_TRY(ctx, w.counts1.alloc((size_t)n_slots * H1 * E::MODELS));
  HIP_TRY(ctx, w.models1.alloc((size_t)n_slots * H1));
  // the models of a sample range live in memory only between the two kernels: a long range is taken in pieces of `piece`
  // samples that reuse one model buffer (F: 224 bytes per sample and pair: 1 872 samples at once would be 420 KB per pair)
  auto score = [&](int h0, int h1, int piece, int ns, const int* slots, const int* lim, typename E::Rec* models, int* counts, const char* name) {
    KTimer t(ctx, name);
    for (int a = h0; a < h1; a += piece) {
      const int b = std::min(h1, a + piece);
      for (int q0 = 0; q0 < ns; q0 += 32768) {   // grid.y limit
        const int np = std::min(32768, ns - q0);
        const int* lq = lim ? lim + q0 : (const int*)nullptr;
        hipLaunchKernelGGL(k_ransac_models<E>, dim3(cdiv(b - a, GEO_WAVE), np), dim3(GEO_WAVE), 0, s, a, b, slots + q0, lq, d_off, p1, p2, run.seed,
                           models + (size_t)q0 * piece);
        hipLaunchKernelGGL(k_ransac_count<E>, dim3(cdiv(b - a, GEO_CNT_SAMPLES), np), dim3(256), 0, s, a, b, slots + q0, lq, d_off, p1, p2, run.th2,
                           models + (size_t)q0 * piece, counts + (size_t)q0 * (h1 - h0) * E::MODELS, h1 - h0, a - h0);
      }
    }
  };
  auto select = [&](int pass, int grid, int Hs) {
    KTimer t(ctx, E::T_SELECT);
    hipLaunchKernelGGL(k_ransac_select<E>, dim3(grid), dim3(GEO_WAVE), 0, s, H, Hs, H1, pass, w.slot_pair.p, w.need.p + 2, w.need.p, w.need.p + 1,
                       w.budget.p, d_off, p1, p2, run.seed, run.th2, run.min_inliers, w.counts1.p, w.counts2.p, w.tab.p, w.tab_off.p, dM, d_in,
                       d_nin, d_ok);
  };
  score(0, H1, H1, n_slots, w.slot_pair.p, nullptr, w.models1.p, w.counts1.p, E::T_SCORE);
  select(1, n_slots, H1);
  if (H1 < H) {
    int need[2] = {0, 0};   // pairs still open after the first H1 samples, and the largest budget among them
    HIP_TRY(ctx, hipMemcpyAsync(need, w.need.p, 2 * sizeof(int), hipMemcpyDeviceToHost, s));
    HIP_TRY(ctx, hipStreamSynchronize(s));
    const int n_need = need[0];
    if (n_need > 0) {
      // samples at or past a pair's budget can never be replayed.  E::TRIM: score [H1, Hs) only, Hs = the largest open budget
      // (<= H), and within it each pair's samples below its own budget (w.budget, in need-list order); otherwise all of [H1, H)
      const int Hs = E::TRIM ? std::min(H, need[1]) : H;
      const int piece = std::min(Hs - H1, 256);
      HIP_TRY(ctx, w.counts2.alloc((size_t)n_need * (Hs - H1) * E::MODELS));
      HIP_TRY(ctx, w.models2.alloc((size_t)n_need * piece));
      // the list holds SLOTS; the kernels of the second range want pairs
      HIP_TRY(ctx, w.need_pair.alloc(n_need));
      hipLaunchKernelGGL(k_gather_int, dim3(cdiv(n_need, 256)), dim3(256), 0, s, n_need, w.need.p + 2, w.slot_pair.p, w.need_pair.p);
      score(H1, Hs, piece, n_need, w.need_pair.p, E::TRIM ? w.budget.p : (const int*)nullptr, w.models2.p, w.counts2.p, E::T_REST);
      select(2, n_need, Hs);
    }
  }
  HIP_TRY(ctx, hipGetLastError());
  return MSFM_OK;
}

// Behind the two public batch calls: upload the offsets and the two point arrays, allocate the four outputs, run(d_off, d1,
// d2, dM, d_in, d_nin, d_ok), download.
template <class Run>
static int ransac_batch_io(msfm_ctx* ctx, int n_pairs, const int* offsets, const float* pt1, const float* pt2, double* M, uint8_t* inlier,
                           int* n_inliers, uint8_t* ok, Run&& run) {
  const int total = offsets[n_pairs];
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  DevBuf<int> d_off, d_nin;
  DevBuf<float> d1, d2;
  DevBuf<double> dM;
  DevBuf<uint8_t> d_in, d_ok;
  DevScope sc(ctx);
  HIP_TRY(ctx, sc.up(d_off, offsets, (size_t)n_pairs + 1));
  HIP_TRY(ctx, sc.up(d1, pt1, 2 * (size_t)total));
  HIP_TRY(ctx, sc.up(d2, pt2, 2 * (size_t)total));
  HIP_TRY(ctx, dM.alloc((size_t)n_pairs * 9));
  HIP_TRY(ctx, d_in.alloc((size_t)std::max(1, total)));
  HIP_TRY(ctx, d_nin.alloc(n_pairs));
  HIP_TRY(ctx, d_ok.alloc(n_pairs));
  MSFM_TRY(run(d_off.p, d1.p, d2.p, dM.p, d_in.p, d_nin.p, d_ok.p));
  HIP_TRY(ctx, sc.down(M, dM.p, 9 * (size_t)n_pairs));
  HIP_TRY(ctx, sc.down(inlier, d_in.p, (size_t)total));
  HIP_TRY(ctx, sc.down(n_inliers, d_nin.p, (size_t)n_pairs));
  HIP_TRY(ctx, sc.down(ok, d_ok.p, (size_t)n_pairs));
  HIP_TRY(ctx, sc.finish());
  return MSFM_OK;
}

MSFM_API void msfm_fransac_default_options(msfm_fransac_options* o) {
  if (!o) return;
  o->threshold = 3.0;
  o->confidence = 0.99;
  o->max_iterations = 2000;
  o->min_points = 30;
  o->min_inliers = 30;
  o->seed = 0x4D53464D46ull;
}

// The verification of a batch of pairs on points that are already resident: d1 / d2 hold the pairs' matches back to back,
// h_offsets (host) and d_off (device) delimit them; results stay on the device.  msfm_fundamental_ransac_batch is this
// between an upload and a download, msfm_chain_verify (chain.hip) calls it on points gathered from the match codes.
int geo_fransac_dev(msfm_ctx* ctx, int n_pairs, const int* offsets, const int* d_off, const float* d1, const float* d2,
                    const msfm_fransac_options* opt, double* dF, uint8_t* d_in, int* d_nin, uint8_t* d_ok) {
  hipStream_t s = ctx->stream;
  // pairs without enough matches (GeoVerificationFundamental: pt1.size() < 30 -> false) get their verdict here; the others
  // form the slot list the kernels run over
  std::vector<int> slot_pair;
  for (int p = 0; p < n_pairs; p++) {
    const int N = offsets[p + 1] - offsets[p];
    if (N >= opt->min_points && N >= 8) slot_pair.push_back(p);
  }
  HIP_TRY(ctx, hipMemsetAsync(dF, 0, sizeof(double) * 9 * (size_t)n_pairs, s));
  HIP_TRY(ctx, hipMemsetAsync(d_in, 0, (size_t)std::max(1, offsets[n_pairs]), s));
  HIP_TRY(ctx, hipMemsetAsync(d_nin, 0, sizeof(int) * (size_t)n_pairs, s));
  HIP_TRY(ctx, hipMemsetAsync(d_ok, 0, (size_t)n_pairs, s));
  RansacWork<FEstimator> w;
  DevScope sc(ctx);
  if (!slot_pair.empty())
    MSFM_TRY(ransac_two_pass<FEstimator>(ctx, {opt->max_iterations, opt->confidence, opt->threshold * opt->threshold, opt->seed, opt->min_inliers},
                                         n_pairs, offsets, d_off, reinterpret_cast<const float2*>(d1), reinterpret_cast<const float2*>(d2),
                                         slot_pair, w, dF, d_in, d_nin, d_ok));
  HIP_TRY(ctx, sc.finish());   // (the buffers of the run are released on return)
  return MSFM_OK;
}

MSFM_API int msfm_fundamental_ransac_batch(msfm_ctx* ctx, int n_pairs, const int* offsets, const float* pt1, const float* pt2,
                                           const msfm_fransac_options* opt, double* F, uint8_t* inlier, int* n_inliers, uint8_t* ok) {
  if (!ctx || n_pairs < 0 || !offsets || !opt || !F || !n_inliers || !ok) return MSFM_E_INVAL;
  if (opt->max_iterations < 1 || opt->max_iterations > 65536 || !(opt->threshold > 0.0)) return msfm_set_error(ctx, MSFM_E_INVAL, "fransac: bad options");
  if (n_pairs == 0) return MSFM_OK;
  MSFM_TRY(msfm_check_offsets(ctx, "fransac", n_pairs, offsets));
  if (offsets[n_pairs] > 0 && (!pt1 || !pt2 || !inlier)) return MSFM_E_INVAL;
  return ransac_batch_io(ctx, n_pairs, offsets, pt1, pt2, F, inlier, n_inliers, ok,
                         [&](const int* d_off, const float* d1, const float* d2, double* dF, uint8_t* d_in, int* d_nin, uint8_t* d_ok) {
                           return geo_fransac_dev(ctx, n_pairs, offsets, d_off, d1, d2, opt, dF, d_in, d_nin, d_ok);
                         });
}

// The closed-form filter of a batch on resident points (pair_of[e] = pair of match e): msfm_epipolar_filter_batch without its
// transfers; msfm_chain_verify calls it on the "all" sets gathered from the match codes.
int geo_epipolar_batch_dev(msfm_ctx* ctx, int total, const int* d_pair_of, const float* d1, const float* d2, const double* dF,
                           const uint8_t* d_ok, double th, uint8_t* d_in) {
  if (total == 0) return MSFM_OK;
  KTimer t(ctx, "geo_epipolar_filter");
  hipLaunchKernelGGL(k_epipolar_batch, dim3(cdiv(total, 256)), dim3(256), 0, ctx->stream, total, d_pair_of, reinterpret_cast<const float2*>(d1),
                     reinterpret_cast<const float2*>(d2), dF, d_ok, th, d_in);
  HIP_TRY(ctx, hipGetLastError());
  return MSFM_OK;
}

MSFM_API int msfm_epipolar_filter_batch(msfm_ctx* ctx, int n_pairs, const int* offsets, const float* pt1, const float* pt2,
                                        const double* F, const uint8_t* ok, double th, uint8_t* inlier) {
  if (!ctx || n_pairs < 0 || !offsets || !F) return MSFM_E_INVAL;
  if (n_pairs == 0) return MSFM_OK;
  const int total = offsets[n_pairs];
  if (total == 0) return MSFM_OK;
  if (!pt1 || !pt2 || !inlier) return MSFM_E_INVAL;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  std::vector<int> pair_of(total);
  for (int p = 0; p < n_pairs; p++) {
    if (offsets[p + 1] < offsets[p]) return msfm_set_error(ctx, MSFM_E_INVAL, "epipolar: offsets must be non-decreasing");
    for (int e = offsets[p]; e < offsets[p + 1]; e++) pair_of[e] = p;
  }
  DevBuf<int> d_po;
  DevBuf<float> d1, d2;
  DevBuf<double> dF;
  DevBuf<uint8_t> d_in, d_ok;
  DevScope sc(ctx);
  HIP_TRY(ctx, sc.up(d_po, pair_of));
  HIP_TRY(ctx, sc.up(d1, pt1, 2 * (size_t)total)); HIP_TRY(ctx, sc.up(d2, pt2, 2 * (size_t)total));
  HIP_TRY(ctx, sc.up(dF, F, 9 * (size_t)n_pairs));
  HIP_TRY(ctx, d_in.alloc(total));
  if (ok) HIP_TRY(ctx, sc.up(d_ok, ok, (size_t)n_pairs));
  {
    KTimer t(ctx, "geo_epipolar_filter");
    hipLaunchKernelGGL(k_epipolar_batch, dim3(cdiv(total, 256)), dim3(256), 0, s, total, d_po.p, reinterpret_cast<const float2*>(d1.p),
                       reinterpret_cast<const float2*>(d2.p), dF.p, ok ? d_ok.p : nullptr, th, d_in.p);
  }
  HIP_TRY(ctx, hipGetLastError());
  HIP_TRY(ctx, sc.down(inlier, d_in.p, (size_t)total));
  HIP_TRY(ctx, sc.finish());
  return MSFM_OK;
}

__device__ static inline double hr_wave_sum(double v) {
  for (int d = 32; d > 0; d >>= 1) v = v + __shfl_xor(v, d);
  return v;
}

// Pairs with N == 4 (cvFindHomography: the direct fit, mask all ones) and N < 4 (no model, mask 0), and pairs the caller
// left out (as "no model").  One wave per pair; pairs with N > 4 that run RANSAC are left to k_ransac_select.
__global__ __launch_bounds__(GEO_WAVE) void k_hransac_small(int n_pairs, const int* __restrict__ off, const uint8_t* __restrict__ active,
                                                             const float2* __restrict__ pt1, const float2* __restrict__ pt2, double* __restrict__ Hout,
                                                             uint8_t* __restrict__ inlier, int* __restrict__ n_inliers, uint8_t* __restrict__ ok) {
  __shared__ double A[72];
  const int pair = blockIdx.x, lane = threadIdx.x;
  const int o = off[pair], N = off[pair + 1] - o;
  if (N > 4 && (!active || active[pair])) return;
  for (int e = lane; e < N; e += GEO_WAVE) inlier[o + e] = N >= 4 ? 1 : 0;
  if (lane != 0) return;
  double H[9];
  bool good = false;
  if (N == 4) {
    double a1[4], b1[4], a2[4], b2[4];
    for (int k = 0; k < 4; k++) {
      const float2 u = pt1[o + k], v = pt2[o + k];
      a1[k] = u.x; b1[k] = u.y; a2[k] = v.x; b2[k] = v.y;
    }
    good = hr_solve4(a1, b1, a2, b2, A, 1, H);
  }
  for (int k = 0; k < 9; k++) Hout[(size_t)pair * 9 + k] = good ? H[k] : 0.0;
  n_inliers[pair] = N >= 4 ? N : 0;
  ok[pair] = good ? 1 : 0;
}

// cvFindHomography's polish of a successful RANSAC: refit on the inliers, then CvHomographyEstimator::refine (CvLevMarq,
// 10 iterations).  One wave per pair; the sums over the inliers in the lane order of the header comment, everything
// sequential (Jacobi, the LM step) on lane 0 in LDS.
__global__ __launch_bounds__(GEO_WAVE) void k_hransac_polish(const int* __restrict__ slot_pair, const int* __restrict__ off,
                                                              const float2* __restrict__ pt1, const float2* __restrict__ pt2,
                                                              const uint8_t* __restrict__ ok, const uint8_t* __restrict__ inlier,
                                                              double* __restrict__ Hout) {
  __shared__ double A[81], V[81], Hs[9], prm[8], prv[8], JtJ[36], JtErr[8];
  const int lane = threadIdx.x;
  const int pair = slot_pair[blockIdx.x];
  if (!ok[pair]) return;
  const int o = off[pair], N = off[pair + 1] - o;
  const float2* p1 = pt1 + o;
  const float2* p2 = pt2 + o;
  const uint8_t* in = inlier + o;
  if (lane < 9) Hs[lane] = Hout[(size_t)pair * 9 + lane];
  __syncthreads();
  // refit: centroids, spreads, LtL
  double s0 = 0, s1 = 0, s2 = 0, s3 = 0, s4 = 0;
  for (int e = lane; e < N; e += GEO_WAVE) {
    if (!in[e]) continue;
    const float2 u = p1[e], v = p2[e];
    s0 = s0 + (double)v.x; s1 = s1 + (double)v.y; s2 = s2 + (double)u.x; s3 = s3 + (double)u.y; s4 = s4 + 1.0;
  }
  s0 = hr_wave_sum(s0); s1 = hr_wave_sum(s1); s2 = hr_wave_sum(s2); s3 = hr_wave_sum(s3); s4 = hr_wave_sum(s4);
  const double cnt = s4;
  const double cx = s0 / cnt, cy = s1 / cnt, cMx = s2 / cnt, cMy = s3 / cnt;
  double d0 = 0, d1 = 0, d2 = 0, d3 = 0;
  for (int e = lane; e < N; e += GEO_WAVE) {
    if (!in[e]) continue;
    const float2 u = p1[e], v = p2[e];
    d0 = d0 + fabs((double)v.x - cx); d1 = d1 + fabs((double)v.y - cy); d2 = d2 + fabs((double)u.x - cMx); d3 = d3 + fabs((double)u.y - cMy);
  }
  d0 = hr_wave_sum(d0); d1 = hr_wave_sum(d1); d2 = hr_wave_sum(d2); d3 = hr_wave_sum(d3);
  if (!(fabs(d0) < DBL_EPSILON || fabs(d1) < DBL_EPSILON || fabs(d2) < DBL_EPSILON || fabs(d3) < DBL_EPSILON)) {
    const double sx = cnt / d0, sy = cnt / d1, sMx = cnt / d2, sMy = cnt / d3;
    double L[45];
#pragma unroll
    for (int q = 0; q < 45; q++) L[q] = 0.0;
    for (int e = lane; e < N; e += GEO_WAVE) {
      if (!in[e]) continue;
      const float2 u = p1[e], v = p2[e];
      const double x = ((double)v.x - cx) * sx, y = ((double)v.y - cy) * sy;
      const double X = ((double)u.x - cMx) * sMx, Y = ((double)u.y - cMy) * sMy;
      const double lx[9] = {X, Y, 1.0, 0.0, 0.0, 0.0, -x * X, -x * Y, -x};
      const double ly[9] = {0.0, 0.0, 0.0, X, Y, 1.0, -y * X, -y * Y, -y};
      int q = 0;
#pragma unroll
      for (int j = 0; j < 9; j++)
#pragma unroll
        for (int k = j; k < 9; k++) { L[q] = L[q] + (lx[j] * lx[k] + ly[j] * ly[k]); q++; }
    }
#pragma unroll
    for (int q = 0; q < 45; q++) L[q] = hr_wave_sum(L[q]);
    if (lane == 0) {
      int q = 0;
      for (int j = 0; j < 9; j++)
        for (int k = j; k < 9; k++) { A[j * 9 + k] = L[q]; A[k * 9 + j] = L[q]; q++; }
      double w[9];
      hr_jacobi(A, 9, w, V);
      int m = 0;
      for (int k = 1; k < 9; k++)
        if (w[k] < w[m]) m = k;
      double h0[9], Hn[9];
      for (int k = 0; k < 9; k++) h0[k] = V[k * 9 + m];
      if (hr_denormalise(h0, sx, sy, cx, cy, sMx, sMy, cMx, cMy, Hn))
        for (int k = 0; k < 9; k++) Hs[k] = Hn[k];
    }
  }
  __syncthreads();
  // refine: CvLevMarq::updateAlt's state machine
  auto eval = [&](bool jac, double* out) {   // out[45]: JtJ upper (36), JtErr (8), errNorm; the same in every lane
    double h[8];
    for (int k = 0; k < 8; k++) h[k] = prm[k];
    double a[45];
#pragma unroll
    for (int q = 0; q < 45; q++) a[q] = 0.0;
    for (int e = lane; e < N; e += GEO_WAVE) {
      if (!in[e]) continue;
      const float2 u = p1[e], v = p2[e];
      const double Mx = u.x, My = u.y;
      double ww = h[6] * Mx + h[7] * My + 1.0;
      ww = fabs(ww) > DBL_EPSILON ? 1.0 / ww : 0.0;
      const double xi = (h[0] * Mx + h[1] * My + h[2]) * ww;
      const double yi = (h[3] * Mx + h[4] * My + h[5]) * ww;
      const double e0 = xi - (double)v.x, e1 = yi - (double)v.y;
      if (jac) {
        const double J0[8] = {Mx * ww, My * ww, ww, 0.0, 0.0, 0.0, -Mx * ww * xi, -My * ww * xi};
        const double J1[8] = {0.0, 0.0, 0.0, Mx * ww, My * ww, ww, -Mx * ww * yi, -My * ww * yi};
        int q = 0;
#pragma unroll
        for (int j = 0; j < 8; j++)
#pragma unroll
          for (int k = j; k < 8; k++) { a[q] = a[q] + (J0[j] * J0[k] + J1[j] * J1[k]); q++; }
#pragma unroll
        for (int j = 0; j < 8; j++) a[36 + j] = a[36 + j] + (J0[j] * e0 + J1[j] * e1);
      }
      a[44] = a[44] + (e0 * e0 + e1 * e1);
    }
    if (jac) {
#pragma unroll
      for (int q = 0; q < 44; q++) out[q] = hr_wave_sum(a[q]);
    }
    out[44] = hr_wave_sum(a[44]);
  };
  if (lane < 8) prm[lane] = Hs[lane];
  __syncthreads();
  double ev[45];
  int lam = -3, iters = 0;
  eval(true, ev);
  double errNorm = ev[44];
  if (lane == 0) {
    for (int k = 0; k < 36; k++) JtJ[k] = ev[k];
    for (int k = 0; k < 8; k++) JtErr[k] = ev[36 + k];
  }
  __syncthreads();
  for (;;) {
    if (lane == 0) {
      for (int k = 0; k < 8; k++) prv[k] = prm[k];
      double pn[8];
      hr_lm_step(prv, JtJ, JtErr, lam, A, V, pn);
      for (int k = 0; k < 8; k++) prm[k] = pn[k];
    }
    __syncthreads();
    const double prevErr = errNorm;
    eval(false, ev);
    errNorm = ev[44];
    while (errNorm > prevErr) {   // uniform: every lane holds the same sums
      if (++lam > 16) break;
      __syncthreads();
      if (lane == 0) {
        double pn[8];
        hr_lm_step(prv, JtJ, JtErr, lam, A, V, pn);
        for (int k = 0; k < 8; k++) prm[k] = pn[k];
      }
      __syncthreads();
      eval(false, ev);
      errNorm = ev[44];
    }
    lam = max(lam - 1, -16);
    double dn = 0.0, pn = 0.0;
    for (int k = 0; k < 8; k++) { const double d = prm[k] - prv[k]; dn = dn + d * d; pn = pn + prv[k] * prv[k]; }
    const double change = sqrt(dn) / (sqrt(pn) + DBL_EPSILON);
    if (++iters >= 10 || change < DBL_EPSILON) break;
    eval(true, ev);
    __syncthreads();
    if (lane == 0) {
      for (int k = 0; k < 36; k++) JtJ[k] = ev[k];
      for (int k = 0; k < 8; k++) JtErr[k] = ev[36 + k];
    }
    __syncthreads();
  }
  if (lane < 8) Hout[(size_t)pair * 9 + lane] = prm[lane];
  if (lane == 8) Hout[(size_t)pair * 9 + 8] = 1.0;
}

MSFM_API void msfm_hransac_default_options(msfm_hransac_options* o) {
  if (!o) return;
  o->threshold = 3.0;
  o->confidence = 0.995;
  o->max_iterations = 2000;
  o->polish = 1;
  o->seed = 0x4D53464D48ull;
}

// The homography RANSAC of a batch on resident points (msfm_homography_ransac_batch without its transfers; msfm_slam_priors
// in prior.hip runs it on the correspondences it gathered).  active (host, may be NULL): pairs with active[p] == 0 are not
// run and get the "no model" result (H = 0, ok = 0, mask ones) - the sampler index of the others stays p.
int geo_hransac_dev(msfm_ctx* ctx, int n_pairs, const int* offsets, const int* d_off, const float* d1, const float* d2,
                    const msfm_hransac_options* opt, const uint8_t* active, double* dH, uint8_t* d_in, int* d_nin, uint8_t* d_ok) {
  hipStream_t s = ctx->stream;
  if (n_pairs == 0) return MSFM_OK;
  const double thr = opt->threshold > 0.0 ? opt->threshold : 3.0;
  const float2* p1 = reinterpret_cast<const float2*>(d1);
  const float2* p2 = reinterpret_cast<const float2*>(d2);
  std::vector<int> slot_pair;
  for (int p = 0; p < n_pairs; p++)
    if (offsets[p + 1] - offsets[p] > 4 && (!active || active[p])) slot_pair.push_back(p);
  DevBuf<uint8_t> d_active;
  RansacWork<HEstimator> w;
  DevScope sc(ctx);
  if (active) HIP_TRY(ctx, sc.up(d_active, active, (size_t)n_pairs));
  {
    KTimer t(ctx, "geo_hransac_small");
    hipLaunchKernelGGL(k_hransac_small, dim3(n_pairs), dim3(GEO_WAVE), 0, s, n_pairs, d_off, active ? d_active.p : (const uint8_t*)nullptr,
                       p1, p2, dH, d_in, d_nin, d_ok);
  }
  HIP_TRY(ctx, hipGetLastError());
  if (!slot_pair.empty()) {
    MSFM_TRY(ransac_two_pass<HEstimator>(ctx, {opt->max_iterations, opt->confidence, thr * thr, opt->seed, 0}, n_pairs, offsets, d_off, p1, p2,
                                         slot_pair, w, dH, d_in, d_nin, d_ok));
    if (opt->polish) {
      KTimer t(ctx, "geo_hransac_polish");
      hipLaunchKernelGGL(k_hransac_polish, dim3((int)slot_pair.size()), dim3(GEO_WAVE), 0, s, w.slot_pair.p, d_off, p1, p2, d_ok, d_in, dH);
    }
    HIP_TRY(ctx, hipGetLastError());
  }
  HIP_TRY(ctx, sc.finish());   // (the buffers of the run are released on return)
  return MSFM_OK;
}

int geo_hransac_check(msfm_ctx* ctx, int n_pairs, const int* offsets, const msfm_hransac_options* opt) {
  if (opt->max_iterations < 1 || opt->max_iterations > 65536) return msfm_set_error(ctx, MSFM_E_INVAL, "hransac: max_iterations out of [1, 65536]");
  if (!(opt->confidence > 0.0 && opt->confidence < 1.0)) return msfm_set_error(ctx, MSFM_E_INVAL, "hransac: confidence outside (0, 1)");
  if (!(opt->threshold == opt->threshold)) return msfm_set_error(ctx, MSFM_E_INVAL, "hransac: threshold is NaN");
  if (n_pairs == 0) return MSFM_OK;
  return msfm_check_offsets(ctx, "hransac", n_pairs, offsets);
}

MSFM_API int msfm_homography_ransac_batch(msfm_ctx* ctx, int n_pairs, const int* offsets, const float* pt1, const float* pt2,
                                          const msfm_hransac_options* opt, double* H, uint8_t* inlier, int* n_inliers, uint8_t* ok) {
  if (!ctx || n_pairs < 0 || !offsets || !opt || !H || !n_inliers || !ok) return MSFM_E_INVAL;
  MSFM_TRY(geo_hransac_check(ctx, n_pairs, offsets, opt));
  if (n_pairs == 0) return MSFM_OK;
  if (offsets[n_pairs] > 0 && (!pt1 || !pt2 || !inlier)) return msfm_set_error(ctx, MSFM_E_INVAL, "hransac: missing point or mask buffers");
  return ransac_batch_io(ctx, n_pairs, offsets, pt1, pt2, H, inlier, n_inliers, ok,
                         [&](const int* d_off, const float* d1, const float* d2, double* dH, uint8_t* d_in, int* d_nin, uint8_t* d_ok) {
                           return geo_hransac_dev(ctx, n_pairs, offsets, d_off, d1, d2, opt, nullptr, dH, d_in, d_nin, d_ok);
                         });
}
