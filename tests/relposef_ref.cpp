// Sequential CPU restatement of msfm_relpose_8pt_batch (metricsfm_amd/csrc/pose.hip):
// RelativePoseEstimation::RelativePoseWithoutFocalLength (SfM/src/orientation/relative_pose_estimation.cc:29-83) =
// the normalised eight-point RANSAC (fundamental_matrix_eight_point.cc), Hartley's focal lengths from F and E
// (relative_pose_from_fundamental_matrix.cc), the decomposition of E and its cheirality vote
// (relative_pose_from_essential_matrix.cc:33-104) - one pair after another, one sample after another, with the
// counter-based sampler and the operation order of the GPU path.  Built by tests/relposef_data.py with
// `g++ -O2 -ffp-contract=off -shared` and loaded with ctypes; the GPU tests compare against it bit for bit.  Only
// + - * / sqrt on doubles, in the order written.
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <vector>

namespace {

static inline uint64_t pose_sm64(uint64_t& s) {
  s += 0x9E3779B97F4A7C15ull;
  uint64_t z = s;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

// K distinct indices of [0, n): stands in for math::RandVectorN (utils/basic_funcs.cc:269-281).
template <int K>
static inline void pose_sample(uint64_t seed, uint64_t salt, int problem, int iter, int n, int* idx) {
  uint64_t s = seed ^ salt ^ ((uint64_t)problem * 0xD1342543DE82EF95ull) ^ ((uint64_t)iter * 0xA24BAED4963EE407ull);
  for (int k = 0; k < K; k++) {
    for (;;) {
      const int v = (int)(pose_sm64(s) % (uint64_t)n);
      bool dup = false;
      for (int j = 0; j < k; j++) dup = dup || (idx[j] == v);
      if (!dup) { idx[k] = v; break; }
    }
  }
}

// One-sided Jacobi SVD on the rows of At[N][M] (OpenCV 2.4 JacobiSVDImpl_<double>): row i of At becomes the i-th left
// singular vector, W is sorted descending, Vt[N][N] (ACCV) receives the right singular vectors.
template <int M, int N, bool ACCV>
static void pose_jsvd(double* At, double* W, double* Vt) {
  const double eps = DBL_EPSILON * 10, minval = DBL_MIN;
  for (int i = 0; i < N; i++) {
    double sd = 0;
    for (int k = 0; k < M; k++) { const double t = At[i * M + k]; sd += t * t; }
    W[i] = sd;
    if (ACCV) { for (int k = 0; k < N; k++) Vt[i * N + k] = 0; Vt[i * N + i] = 1; }
  }
  const int max_iter = M > 30 ? M : 30;
  for (int iter = 0; iter < max_iter; iter++) {
    bool changed = false;
    for (int i = 0; i < N - 1; i++)
      for (int j = i + 1; j < N; j++) {
        double* Ai = At + i * M;
        double* Aj = At + j * M;
        double a = W[i], p = 0, b = W[j];
        for (int k = 0; k < M; k++) p += Ai[k] * Aj[k];
        if (std::fabs(p) <= eps * std::sqrt(a * b)) continue;
        p *= 2;
        const double beta = a - b, gamma = std::sqrt(p * p + beta * beta);
        double c, s;
        if (beta < 0) {
          const double delta = (gamma - beta) * 0.5;
          s = std::sqrt(delta / gamma);
          c = p / (gamma * s * 2);
        } else {
          c = std::sqrt((gamma + beta) / (gamma * 2));
          s = p / (gamma * c * 2);
        }
        a = b = 0;
        for (int k = 0; k < M; k++) {
          const double t0 = c * Ai[k] + s * Aj[k];
          const double t1 = -s * Ai[k] + c * Aj[k];
          Ai[k] = t0; Aj[k] = t1;
          a += t0 * t0; b += t1 * t1;
        }
        W[i] = a; W[j] = b;
        changed = true;
        if (ACCV) {
          double* Vi = Vt + i * N;
          double* Vj = Vt + j * N;
          for (int k = 0; k < N; k++) {
            const double t0 = c * Vi[k] + s * Vj[k];
            const double t1 = -s * Vi[k] + c * Vj[k];
            Vi[k] = t0; Vj[k] = t1;
          }
        }
      }
    if (!changed) break;
  }
  for (int i = 0; i < N; i++) {
    double sd = 0;
    for (int k = 0; k < M; k++) { const double t = At[i * M + k]; sd += t * t; }
    W[i] = std::sqrt(sd);
  }
  for (int i = 0; i < N - 1; i++) {
    int j = i;
    for (int k = i + 1; k < N; k++)
      if (W[j] < W[k]) j = k;
    if (i != j) {
      { const double t = W[i]; W[i] = W[j]; W[j] = t; }
      for (int k = 0; k < M; k++) { const double t = At[i * M + k]; At[i * M + k] = At[j * M + k]; At[j * M + k] = t; }
      if (ACCV)
        for (int k = 0; k < N; k++) { const double t = Vt[i * N + k]; Vt[i * N + k] = Vt[j * N + k]; Vt[j * N + k] = t; }
    }
  }
  uint64_t rng = 0x12345678;
  for (int i = 0; i < N; i++) {
    double sd = W[i];
    int guard = 0;
    while (sd <= minval && guard++ < 64) {
      const double val0 = 1. / M;
      for (int k = 0; k < M; k++) {
        rng = (uint64_t)(unsigned)rng * 4164903690U + (unsigned)(rng >> 32);
        At[i * M + k] = ((unsigned)rng & 256) != 0 ? val0 : -val0;
      }
      for (int it = 0; it < 2; it++)
        for (int j = 0; j < i; j++) {
          sd = 0;
          for (int k = 0; k < M; k++) sd += At[i * M + k] * At[j * M + k];
          double asum = 0;
          for (int k = 0; k < M; k++) {
            const double t = At[i * M + k] - sd * At[j * M + k];
            At[i * M + k] = t;
            asum += std::fabs(t);
          }
          asum = asum ? 1 / asum : 0;
          for (int k = 0; k < M; k++) At[i * M + k] *= asum;
        }
      sd = 0;
      for (int k = 0; k < M; k++) { const double t = At[i * M + k]; sd += t * t; }
      sd = std::sqrt(sd);
    }
    const double s = 1 / sd;
    for (int k = 0; k < M; k++) At[i * M + k] *= s;
  }
}

// Eigen::FullPivLU elimination, row-major r x c (ld): pivot = first largest |a| in column-major scan order
static int p5_fullpiv_lu(double* a, int r, int c, int ld, int* perm_r, int* perm_c, double* maxpivot) {
  const int size = r < c ? r : c;
  for (int i = 0; i < r; i++) perm_r[i] = i;
  for (int j = 0; j < c; j++) perm_c[j] = j;
  int nonzero = size;
  *maxpivot = 0.0;
  for (int k = 0; k < size; k++) {
    int pr = k, pc = k;
    double best = -1.0;
    for (int j = k; j < c; j++)
      for (int i = k; i < r; i++) {
        const double v = std::fabs(a[i * ld + j]);
        if (v > best) { best = v; pr = i; pc = j; }
      }
    if (best == 0.0) { nonzero = k; break; }
    if (best > *maxpivot) *maxpivot = best;
    if (pr != k) {
      for (int j = 0; j < c; j++) { const double t = a[k * ld + j]; a[k * ld + j] = a[pr * ld + j]; a[pr * ld + j] = t; }
      const int t = perm_r[k]; perm_r[k] = perm_r[pr]; perm_r[pr] = t;
    }
    if (pc != k) {
      for (int i = 0; i < r; i++) { const double t = a[i * ld + k]; a[i * ld + k] = a[i * ld + pc]; a[i * ld + pc] = t; }
      const int t = perm_c[k]; perm_c[k] = perm_c[pc]; perm_c[pc] = t;
    }
    if (k < r - 1)
      for (int i = k + 1; i < r; i++) a[i * ld + k] /= a[k * ld + k];
    if (k < size - 1)
      for (int i = k + 1; i < r; i++)
        for (int j = k + 1; j < c; j++) a[i * ld + j] -= a[i * ld + k] * a[k * ld + j];
  }
  return nonzero;
}

#define F8_SALT 0x38707446ull
#define F8_MAXN 15

// NormalizeImagePoints (:175-203): centroid, then the RMS distance to it scaled to sqrt(2).  T = {s, tx, ty} stands
// for the matrix [s 0 tx; 0 s ty; 0 0 1].
static void f8_normalize(const double* x, int n, double* xn, double* T) {
  double cx = 0.0, cy = 0.0;
  for (int i = 0; i < n; i++) { cx += x[2 * i]; cy += x[2 * i + 1]; }
  cx = cx / n; cy = cy / n;
  double ss = 0.0;
  for (int i = 0; i < n; i++) {
    const double dx = x[2 * i] - cx, dy = x[2 * i + 1] - cy;
    ss += dx * dx + dy * dy;
  }
  const double s = 1.4142135623730951 / std::sqrt(ss / n);
  T[0] = s; T[1] = -1.0 * s * cx; T[2] = -1.0 * s * cy;
  for (int i = 0; i < n; i++) { xn[2 * i] = s * x[2 * i] + T[1]; xn[2 * i + 1] = s * x[2 * i + 1] + T[2]; }
}

// NormalizedEightPointFundamentalMatrix (:105-168) on n in [8, 15] matches x1[2n], x2[2n]; F row-major with
// x2^T F x1 = 0.  Eight matches: the kernel of the 8x9 constraint matrix by full-pivot LU, false unless it is
// one-dimensional; more: the last right singular vector, the constraint matrix padded with zero rows to F8_MAXN so
// that one instance of the Jacobi SVD serves every size (a zero row adds exact zeros to each of its sums).
static bool f8_fit(const double* x1, const double* x2, int n, double* F) {
  double a[2 * F8_MAXN], b[2 * F8_MAXN], T1[3], T2[3], fv[9];
  f8_normalize(x1, n, a, T1);
  f8_normalize(x2, n, b, T2);
  if (n == 8) {
    double A[72];
    for (int i = 0; i < 8; i++) {
      double* r = A + 9 * i;
      r[0] = a[2 * i] * b[2 * i]; r[1] = a[2 * i + 1] * b[2 * i]; r[2] = 1.0 * b[2 * i];
      r[3] = a[2 * i] * b[2 * i + 1]; r[4] = a[2 * i + 1] * b[2 * i + 1]; r[5] = 1.0 * b[2 * i + 1];
      r[6] = a[2 * i]; r[7] = a[2 * i + 1]; r[8] = 1.0;
    }
    int pr[8], pc[9];
    double maxpivot;
    const int nz = p5_fullpiv_lu(A, 8, 9, 9, pr, pc, &maxpivot);
    const double thr = maxpivot * (DBL_EPSILON * 8);
    int rank = 0;
    for (int i = 0; i < nz; i++) rank += std::fabs(A[i * 9 + i]) > thr;
    if (rank != 8) return false;
    double y[8];
    for (int i = 7; i >= 0; i--) y[i] = A[i * 9 + 8];
    for (int i = 7; i >= 0; i--) {
      y[i] = y[i] / A[i * 9 + i];
      for (int j = 0; j < i; j++) y[j] -= A[j * 9 + i] * y[i];
    }
    for (int i = 0; i < 8; i++) fv[pc[i]] = -y[i];
    fv[pc[8]] = 1.0;
  } else {
    double At[9 * F8_MAXN], W[9], Vt[81];
    for (int k = 0; k < F8_MAXN; k++) {
      double r[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
      if (k < n) {
        r[0] = a[2 * k] * b[2 * k]; r[1] = a[2 * k + 1] * b[2 * k]; r[2] = 1.0 * b[2 * k];
        r[3] = a[2 * k] * b[2 * k + 1]; r[4] = a[2 * k + 1] * b[2 * k + 1]; r[5] = 1.0 * b[2 * k + 1];
        r[6] = a[2 * k]; r[7] = a[2 * k + 1]; r[8] = 1.0;
      }
      for (int c = 0; c < 9; c++) At[c * F8_MAXN + k] = r[c];
    }
    pose_jsvd<F8_MAXN, 9, true>(At, W, Vt);
    for (int i = 0; i < 9; i++) fv[i] = Vt[72 + i];
  }
  // closest rank-2 matrix (:155-162), then T2^T F T1 (:165)
  double Ut[9], W[3], Vt[9], G[9], H[9];
  for (int i = 0; i < 3; i++)
    for (int k = 0; k < 3; k++) Ut[i * 3 + k] = fv[k * 3 + i];
  pose_jsvd<3, 3, true>(Ut, W, Vt);
  for (int r = 0; r < 3; r++)
    for (int c = 0; c < 3; c++) G[3 * r + c] = Ut[r] * W[0] * Vt[c] + Ut[3 + r] * W[1] * Vt[3 + c];
  for (int r = 0; r < 3; r++) {
    H[3 * r] = G[3 * r] * T1[0];
    H[3 * r + 1] = G[3 * r + 1] * T1[0];
    H[3 * r + 2] = G[3 * r] * T1[1] + G[3 * r + 1] * T1[2] + G[3 * r + 2];
  }
  for (int c = 0; c < 3; c++) {
    F[c] = T2[0] * H[c];
    F[3 + c] = T2[0] * H[3 + c];
    F[6 + c] = T2[1] * H[c] + T2[2] * H[3 + c] + H[6 + c];
  }
  return true;
}

// FocalLengthFromFMatrix (:56-123), F row-major.  The reference turns each epipole onto the x-z plane by
// theta = atan2(-e1, e0) and cos / sin of it; c = e0 / sqrt(e0^2 + e1^2), s = -e1 / sqrt(e0^2 + e1^2) are that same
// cosine and sine without a libm call.  A NaN f^2 passes the `< 0` test, as it does there.  e1, e2 (may be null)
// receive the epipoles.
static bool f8_focal(const double* F, double* f1, double* f2, double* e1out, double* e2out) {
  double A[9], W[3], V1[9], V2[9];
  for (int i = 0; i < 3; i++)
    for (int k = 0; k < 3; k++) A[i * 3 + k] = F[k * 3 + i];
  pose_jsvd<3, 3, true>(A, W, V1);
  for (int i = 0; i < 9; i++) A[i] = F[i];
  pose_jsvd<3, 3, true>(A, W, V2);
  const double* e1 = V1 + 6;
  const double* e2 = V2 + 6;
  if (e1out) for (int i = 0; i < 3; i++) { e1out[i] = e1[i]; e2out[i] = e2[i]; }
  if (e1[0] == 0 || e2[0] == 0) return false;
  const double n1 = std::sqrt(e1[0] * e1[0] + e1[1] * e1[1]), n2 = std::sqrt(e2[0] * e2[0] + e2[1] * e2[1]);
  const double c1 = e1[0] / n1, s1 = -e1[1] / n1, c2 = e2[0] / n2, s2 = -e2[1] / n2;
  double M[6], Fr[4];  // rows 0, 1 of rotation2 * F, then the upper-left 2x2 of (rotation2 * F) * rotation1^T
  for (int j = 0; j < 3; j++) { M[j] = c2 * F[j] - s2 * F[3 + j]; M[3 + j] = s2 * F[j] + c2 * F[3 + j]; }
  for (int i = 0; i < 2; i++) { Fr[2 * i] = M[3 * i] * c1 - M[3 * i + 1] * s1; Fr[2 * i + 1] = M[3 * i] * s1 + M[3 * i + 1] * c1; }
  const double e1x = c1 * e1[0] - s1 * e1[1], e1z = e1[2], e2x = c2 * e2[0] - s2 * e2[1], e2z = e2[2];
  const double i1 = 1.0 / e1z, i2 = 1.0 / e2z;
  const double a = i2 * Fr[0] * i1, b = i2 * Fr[1], c = Fr[2] * i1, d = Fr[3];
  const double f1sq = (-a * c * e1x * e1x) / (a * c * e1z * e1z + b * d);
  const double f2sq = (-a * b * e2x * e2x) / (a * b * e2z * e2z + c * d);
  if (f1sq < 0 || f2sq < 0) return false;
  *f1 = std::sqrt(f1sq);
  *f2 = std::sqrt(f2sq);
  return true;
}


// Error (:205-221): the Sampson sum over all matches in match order, F row-major
double sampson_sum(const double* F, const double* x1, const double* x2, int n) {
  double total = 0.0;
  for (int i = 0; i < n; i++) {
    const double ax = x1[2 * i], ay = x1[2 * i + 1];
    const double bx = x2[2 * i], by = x2[2 * i + 1];
    const double l0 = F[0] * ax + F[1] * ay + F[2] * 1.0, l1 = F[3] * ax + F[4] * ay + F[5] * 1.0, l2 = F[6] * ax + F[7] * ay + F[8] * 1.0;
    const double num = bx * l0 + by * l1 + 1.0 * l2;
    const double d0 = bx * F[0] + by * F[3] + 1.0 * F[6], d1 = bx * F[1] + by * F[4] + 1.0 * F[7];
    const double den = d0 * d0 + d1 * d1 + l0 * l0 + l1 * l1;
    total += num * num / den;
  }
  return total;
}

// ReltivePoseFromEMatrix (relative_pose_from_essential_matrix.cc:33-104) on pts / f1, pts / f2: E column-major in, R
// row-major out; the first hypothesis with the most votes.
void pose_from_E(const double* E, int N, const double* pts_ref, const double* pts_cur, double f1, double f2, double* Rout, double* tout) {
  double s_R[4][9], s_t[4][3];
  int s_votes[4] = {0, 0, 0, 0};
  {
    double Ut[9], W[3], Vt[9], U[3][3], V[3][3];
    for (int i = 0; i < 3; i++)
      for (int k = 0; k < 3; k++) Ut[i * 3 + k] = E[k + 3 * i];
    pose_jsvd<3, 3, true>(Ut, W, Vt);
    for (int i = 0; i < 3; i++)
      for (int j = 0; j < 3; j++) { U[i][j] = Ut[j * 3 + i]; V[i][j] = Vt[j * 3 + i]; }
    const double detU = U[0][0] * (U[1][1] * U[2][2] - U[1][2] * U[2][1]) - U[0][1] * (U[1][0] * U[2][2] - U[1][2] * U[2][0]) +
                        U[0][2] * (U[1][0] * U[2][1] - U[1][1] * U[2][0]);
    if (detU < 0) for (int i = 0; i < 3; i++) U[i][2] *= -1.0;
    const double detV = V[0][0] * (V[1][1] * V[2][2] - V[1][2] * V[2][1]) - V[0][1] * (V[1][0] * V[2][2] - V[1][2] * V[2][0]) +
                        V[0][2] * (V[1][0] * V[2][1] - V[1][1] * V[2][0]);
    if (detV < 0) for (int i = 0; i < 3; i++) V[i][2] *= -1.0;
    for (int i = 0; i < 3; i++)
      for (int j = 0; j < 3; j++) {
        const double r1 = -U[i][1] * V[j][0] + U[i][0] * V[j][1] + U[i][2] * V[j][2];
        const double r2 = U[i][1] * V[j][0] + -U[i][0] * V[j][1] + U[i][2] * V[j][2];
        s_R[0][3 * i + j] = r1; s_R[1][3 * i + j] = r1; s_R[2][3 * i + j] = r2; s_R[3][3 * i + j] = r2;
      }
    const double tn = std::sqrt(U[0][2] * U[0][2] + U[1][2] * U[1][2] + U[2][2] * U[2][2]);
    double t[3];
    for (int i = 0; i < 3; i++) t[i] = U[i][2] / tn;
    for (int h = 0; h < 4; h++) {
      const double sg = (h & 1) ? -1.0 : 1.0;
      for (int i = 0; i < 3; i++) s_t[h][i] = -(s_R[h][i] * (sg * t[0]) + s_R[h][3 + i] * (sg * t[1]) + s_R[h][6 + i] * (sg * t[2]));
    }
  }
  for (int i = 0; i < N; i++) {
    const double d1[3] = {pts_ref[2 * (size_t)i] / f1, pts_ref[2 * (size_t)i + 1] / f1, 1.0};
    const double q[3] = {pts_cur[2 * (size_t)i] / f2, pts_cur[2 * (size_t)i + 1] / f2, 1.0};
    for (int h = 0; h < 4; h++) {
      const double* R = s_R[h];
      const double* tt = s_t[h];
      double c[3], d2[3];
      for (int k = 0; k < 3; k++) {
        c[k] = -(R[k] * tt[0] + R[3 + k] * tt[1] + R[6 + k] * tt[2]);
        d2[k] = R[k] * q[0] + R[3 + k] * q[1] + R[6 + k] * q[2];
      }
      const double d1sq = d1[0] * d1[0] + d1[1] * d1[1] + d1[2] * d1[2], d2sq = d2[0] * d2[0] + d2[1] * d2[1] + d2[2] * d2[2];
      const double d12 = d1[0] * d2[0] + d1[1] * d2[1] + d1[2] * d2[2];
      const double d1p = d1[0] * c[0] + d1[1] * c[1] + d1[2] * c[2], d2p = d2[0] * c[0] + d2[1] * c[1] + d2[2] * c[2];
      if (d2sq * d1p - d12 * d2p > 0 && d12 * d1p - d1sq * d2p > 0) { s_votes[h]++; break; }
    }
  }
  int mx = s_votes[0];
  for (int h = 1; h < 4; h++) mx = s_votes[h] > mx ? s_votes[h] : mx;
  int h = 0;
  while (s_votes[h] != mx) h++;
  for (int i = 0; i < 9; i++) Rout[i] = s_R[h][i];
  for (int i = 0; i < 3; i++) tout[i] = s_t[h][i];
}

}  // namespace

#define RF_API extern "C" __attribute__((visibility("default")))

// sample `it` of pair `problem` with n matches: 8 distinct indices
RF_API void rf_sample8(uint64_t seed, int problem, int it, int n, int* idx) { pose_sample<8>(seed, F8_SALT, problem, it, n, idx); }

// the single-sample fit on n in [8, 15] matches; F row-major; 1 = a fit
RF_API int rf_fit(const double* x1, const double* x2, int n, double* F) {
  if (n < 8 || n > F8_MAXN) return 0;
  return f8_fit(x1, x2, n, F) ? 1 : 0;
}

// focal lengths and the two epipoles (e1, e2 may be null) from a row-major F; 1 = extracted
RF_API int rf_focal_from_F(const double* F, double* f1, double* f2, double* e1, double* e2) {
  double e1b[3], e2b[3];
  *f1 = 0.0; *f2 = 0.0;
  const bool good = f8_focal(F, f1, f2, e1b, e2b);
  if (e1) for (int i = 0; i < 3; i++) e1[i] = e1b[i];
  if (e2) for (int i = 0; i < 3; i++) e2[i] = e2b[i];
  return good ? 1 : 0;
}

// pose from a row-major E with x_cur^T E x_ref = 0 on (pts / f, 1)
RF_API void rf_pose_from_E(const double* E, int n, const double* pts_ref, const double* pts_cur, double f1, double f2, double* R, double* t) {
  double Ec[9];
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) Ec[i + 3 * j] = E[3 * i + j];
  pose_from_E(Ec, n, pts_ref, pts_cur, f1, f2, R, t);
}

RF_API int rf_relpose_8pt_batch(int n_pairs, const int* off, const double* pts_ref, const double* pts_cur, int ransac_times, uint64_t seed,
                                double* Fout, double* f1out, double* f2out, double* Eout, double* Rout, double* tout, uint8_t* ok,
                                int* best_iter, double* best_error, int* n_candidates) {
  for (int p = 0; p < n_pairs; p++) {
    const int o = off[p], N = off[p + 1] - o;
    const double* x1 = pts_ref + 2 * (size_t)o;
    const double* x2 = pts_cur + 2 * (size_t)o;
    for (int k = 0; k < 9; k++) { Fout[9 * (size_t)p + k] = 0.0; Eout[9 * (size_t)p + k] = 0.0; Rout[9 * (size_t)p + k] = 0.0; }
    for (int k = 0; k < 3; k++) tout[3 * (size_t)p + k] = 0.0;
    f1out[p] = 0.0; f2out[p] = 0.0;
    ok[p] = 0;
    int bi = -1, nC = 0;
    double be = 1000000.0;
    std::vector<double> Fs;   // the candidates, 9 each
    std::vector<int> its;     // and the sample each came from
    if (N >= 8) {
      const int T = N < 16 ? 1 : ransac_times;
      for (int it = 0; it < T; it++) {
        int idx[F8_MAXN];
        int n = 8;
        if (N < 16) { n = N; for (int k = 0; k < N; k++) idx[k] = k; }
        else pose_sample<8>(seed, F8_SALT, p, it, N, idx);
        double a[2 * F8_MAXN], b[2 * F8_MAXN], F[9];
        for (int k = 0; k < n; k++) {
          a[2 * k] = x1[2 * (size_t)idx[k]]; a[2 * k + 1] = x1[2 * (size_t)idx[k] + 1];
          b[2 * k] = x2[2 * (size_t)idx[k]]; b[2 * k + 1] = x2[2 * (size_t)idx[k] + 1];
        }
        if (!f8_fit(a, b, n, F)) continue;
        Fs.insert(Fs.end(), F, F + 9);
        its.push_back(it);
      }
    }
    nC = (int)its.size();
    if (nC > 0) {
      int idx_min = 0;
      for (int i = 0; i < nC; i++) {
        const double e = sampson_sum(&Fs[9 * (size_t)i], x1, x2, N);
        if (e < be) { be = e; idx_min = i; }
      }
      bi = its[idx_min];
      const double* F = &Fs[9 * (size_t)idx_min];
      for (int k = 0; k < 9; k++) Fout[9 * (size_t)p + k] = F[k];
      double f1, f2;
      if (f8_focal(F, &f1, &f2, nullptr, nullptr)) {
        const double d1[3] = {f1, f1, 1.0}, d2[3] = {f2, f2, 1.0};
        double Ec[9];
        for (int i = 0; i < 3; i++)
          for (int j = 0; j < 3; j++) {
            const double e = d2[i] * F[3 * i + j] * d1[j];
            Eout[9 * (size_t)p + 3 * i + j] = e;
            Ec[i + 3 * j] = e;
          }
        f1out[p] = f1; f2out[p] = f2;
        ok[p] = 1;
        pose_from_E(Ec, N, x1, x2, f1, f2, Rout + 9 * (size_t)p, tout + 3 * (size_t)p);
      }
    }
    if (best_iter) best_iter[p] = bi;
    if (best_error) best_error[p] = be;
    if (n_candidates) n_candidates[p] = nC;
  }
  return 0;
}
