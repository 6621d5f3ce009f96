// Registering the SLAM model on its GPS track: what SLAMGPS::Run does between Triangulation and the end of
// FullBundleAdjustment (SfM/src/slam_gps.cc:98-119) beside the bundle adjustment itself.
//   msfm_gps_orient_global     AbsoluteOrientationWithGPSGlobal (:1596-1674) with SimilarityTransformation
//                              (utils/transformation.cpp:142-216) and Camera::Transformation (camera.cc:79-87).  Host only: the
//                              weights need acos and tan, a 3x3 SVD of one matrix is no device work.
//   msfm_point_accuracy_batch  GetAccuracy (:1573-1594) = AccuracyAssessment::ErrorReprojectionPts / Pti
//                              (accuracy_accessment.cc:38-113) and the flags of :1584-1593
//   msfm_gps_register_points   the point loop of GPSRegistration2 (:933-978)
// The two device steps are walks over CSR tracks whose per-track sums keep row order.  Both were built in two forms that give
// the same bits, and measured at config 5's track shape ("Registering the SLAM model"); each keeps the faster:
//   accuracy  the row form.  A workgroup owns the tracks whose first row lies in its 256-row slice of the row array - the slice
//             is found from track_off on the device, which is the scan of the track lengths already.  One lane per row forms
//             the row's error (a 3x4 product, two divisions, the distortion polynomial) from coalesced loads of track_cam / xy
//             and parks it in LDS; one lane per track then adds its rows' errors in row order and walks them a second time for
//             e_mse.  A track that reaches past the LDS window is summed by its lane from global memory with the same row
//             function.
//   shift     one thread per track, k_tri_dlt's shape: a row's term is two square roots and a division, too little to pay for
//             the slice search, the LDS round trip and the barrier.
// + - * / sqrt only and no fused multiply-adds: tests/gpsreg_ref.cpp built with -ffp-contract=off agrees bit for bit.
#include <cmath>
#include <limits>

#include "common.h"

#pragma clang fp contract(off)
#include "point3d_device.h"   // p3d_camera_point, p3d_project

namespace gpr {

constexpr int ROWS = 256;      // rows of a workgroup's slice
constexpr int WINDOW = 320;    // rows its LDS window holds: a track of the slice may run WINDOW - ROWS rows past the slice's end

// first track t in [0, n] with off[t] >= x  (off[n] = rows in all; n when none)
__device__ static inline int first_track_at(const int* __restrict__ off, int n, int x) {
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (off[mid] < x) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// the tracks [t_lo, t_hi) of workgroup w: those whose first row lies in [w * ROWS, (w + 1) * ROWS); the last workgroup also
// takes the empty tracks at the end
__device__ static inline void slice_tracks(const int* __restrict__ off, int n_tracks, int& t_lo, int& t_hi) {
  t_lo = first_track_at(off, n_tracks, (int)blockIdx.x * ROWS);
  t_hi = blockIdx.x + 1 == gridDim.x ? n_tracks : first_track_at(off, n_tracks, ((int)blockIdx.x + 1) * ROWS);
}

// ---- accuracy ----
// accuracy_accessment.cc:47-57: the squared reprojection error of row i for the point X, -1.0 when the depth is not positive
// (e itself is a sum of two squares: never negative).  std::pow(d, 2) is d * d.
__device__ __forceinline__ double acc_row(const AccuracyPtrs& P, int i, double X0, double X1, double X2) {
  const int c = P.cam[i];
  const double X[3] = {X0, X1, X2};
  double pc[3], uv[2];
  p3d_camera_point(P.R + 9 * (size_t)c, P.t + 3 * (size_t)c, X, pc);
  if (!(pc[2] > 0)) return -1.0;   // (not Reprojection's strict rule: a zero or NaN depth drops the row here)
  p3d_project(P.fk + 3 * (size_t)c, pc, uv);
  const double dcx = P.dc ? P.dc[2 * (size_t)c] : 0.0, dcy = P.dc ? P.dc[2 * (size_t)c + 1] : 0.0;
  const double u = uv[0] + dcx, v = uv[1] + dcy;
  const double du = u - P.xy[2 * (size_t)i], dv = v - P.xy[2 * (size_t)i + 1];
  return du * du + dv * dv;
}

// ErrorReprojectionPti :63-82 and ErrorReprojectionPts :94-103 for track t, whose row terms are term(i), i in [b, e);
// returns whether the point counts as an outlier of slam_gps.cc:1587
template <class Term>
__device__ __forceinline__ bool acc_track(const AccuracyPtrs& P, int t, int b, int e, Term term) {
  double e_avg = 1000.0, e_mse = 0.0;
  int m = 0;
  const bool live = P.ok_in[t] != 0 && e - b >= P.min_views;
  if (live) {
    double sum = 0.0;
    for (int i = b; i < e; i++) {
      const double v = term(i);
      if (v != -1.0) { sum += v; m++; }
    }
    if (m > 1) {
      e_avg = sum / (double)m;
      double sq = 0.0;
      for (int i = b; i < e; i++) {
        const double v = term(i);
        if (v != -1.0) sq += (v - e_avg) * (v - e_avg);
      }
      e_mse = sqrt(sq / (double)(m - 1));
    } else {
      m = 0;
    }
  }
  const bool outlier = e_avg > P.th_outlier;
  P.e_avg[t] = e_avg; P.e_mse[t] = e_mse; P.n_used[t] = m;
  P.ok_out[t] = live && !outlier;
  return outlier;
}

// the outliers of the workgroup into *n_outliers: an integer sum, one atomic per workgroup
__device__ __forceinline__ void count_outliers(int mine, int* wave_tot /*[4] LDS*/, int* __restrict__ n_outliers) {
  const int w = wave_sum_int(mine);
  if ((threadIdx.x & 63) == 0) wave_tot[threadIdx.x >> 6] = w;
  __syncthreads();
  if (threadIdx.x == 0) {
    const int tot = wave_tot[0] + wave_tot[1] + wave_tot[2] + wave_tot[3];
    if (tot) atomicAdd(n_outliers, tot);
  }
}

__global__ __launch_bounds__(256) void k_accuracy(AccuracyPtrs P, int* __restrict__ n_outliers) {
  __shared__ double term[WINDOW];
  __shared__ int wt[4];
  int t_lo, t_hi;
  slice_tracks(P.off, P.n_tracks, t_lo, t_hi);
  const int r0 = P.off[t_lo], r1 = min(P.off[t_hi], r0 + WINDOW);   // (t_lo <= n_tracks: off has n_tracks + 1 entries)
  // lane = row
  for (int i = r0 + (int)threadIdx.x; i < r1; i += 256) {
    const int t = t_lo + csr_segment_of(P.off + t_lo, t_hi - t_lo, i);
    term[i - r0] = acc_row(P, i, P.X[3 * (size_t)t], P.X[3 * (size_t)t + 1], P.X[3 * (size_t)t + 2]);
  }
  __syncthreads();
  // lane = track
  int mine = 0;
  for (int t = t_lo + (int)threadIdx.x; t < t_hi; t += 256) {
    const int b = P.off[t], e = P.off[t + 1];
    if (e <= r1) {
      mine += acc_track(P, t, b, e, [&](int i) { return term[i - r0]; });
    } else {
      const double X0 = P.X[3 * (size_t)t], X1 = P.X[3 * (size_t)t + 1], X2 = P.X[3 * (size_t)t + 2];
      mine += acc_track(P, t, b, e, [&](int i) { return acc_row(P, i, X0, X1, X2); });
    }
  }
  count_outliers(mine, wt, n_outliers);
}

// ---- the shift of GPSRegistration2 ----
// slam_gps.cc:940-977, one thread per track
__global__ __launch_bounds__(256) void k_register(RegisterPtrs P) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= P.n_tracks || !P.ok[t]) return;
  const double X0 = P.X[3 * (size_t)t], X1 = P.X[3 * (size_t)t + 1], X2 = P.X[3 * (size_t)t + 2];
  double ox = 0.0, oy = 0.0, oz = 0.0, weight = 0.0;
  for (int i = P.off[t]; i < P.off[t + 1]; i++) {
    const int c = P.cam[i];
    const double* cc = P.cam_c + 3 * (size_t)c;
    const double* o = P.cam_offset + 3 * (size_t)c;
    const double dx = X0 - cc[0], dy = X1 - cc[1], dz = X2 - cc[2];
    const double dis = sqrt(dx * dx + dy * dy + dz * dz);
    const double w = 1.0 / (sqrt(dis) + 5.0);
    weight += w;
    ox += w * o[0]; oy += w * o[1]; oz += w * o[2];
  }
  ox /= weight; oy /= weight; oz /= weight;
  P.X[3 * (size_t)t] = X0 + ox; P.X[3 * (size_t)t + 1] = X1 + oy; P.X[3 * (size_t)t + 2] = X2 + oz;
}

// the adjusted points of a bundle adjustment back into the tracks they were gathered from (adj::k_scatter_points' shape)
__global__ __launch_bounds__(256) void k_store_points(int n, const int* __restrict__ track_of_point, const double* __restrict__ point, double* __restrict__ X) {
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= n) return;
  const size_t t = (size_t)track_of_point[p];
  X[3 * t] = point[3 * (size_t)p]; X[3 * t + 1] = point[3 * (size_t)p + 1]; X[3 * t + 2] = point[3 * (size_t)p + 2];
}

static int slices(int n_rows) { return std::max(1, cdiv(n_rows, ROWS)); }

}  // namespace gpr

// ---- device-array cores (chain.hip calls them on its resident arrays) ----
int gps_accuracy_dev(msfm_ctx* ctx, const AccuracyPtrs& P, int n_rows, int* d_n_outliers) {
  hipStream_t s = ctx->stream;
  HIP_TRY(ctx, hipMemsetAsync(d_n_outliers, 0, sizeof(int), s));
  if (P.n_tracks == 0) return MSFM_OK;
  KTimer t(ctx, "gps_accuracy");
  hipLaunchKernelGGL(gpr::k_accuracy, dim3(gpr::slices(n_rows)), dim3(256), 0, s, P, d_n_outliers);
  HIP_TRY(ctx, hipGetLastError());
  return MSFM_OK;
}

int gps_register_dev(msfm_ctx* ctx, const RegisterPtrs& P) {
  if (P.n_tracks == 0) return MSFM_OK;
  KTimer t(ctx, "gps_register");
  hipLaunchKernelGGL(gpr::k_register, dim3(cdiv(P.n_tracks, 256)), dim3(256), 0, ctx->stream, P);
  HIP_TRY(ctx, hipGetLastError());
  return MSFM_OK;
}

int gps_store_points_dev(msfm_ctx* ctx, int n_points, const int* d_track_of_point, const double* d_point, double* dX) {
  if (n_points == 0) return MSFM_OK;
  KTimer t(ctx, "gps_store_points");
  hipLaunchKernelGGL(gpr::k_store_points, dim3(cdiv(n_points, 256)), dim3(256), 0, ctx->stream, n_points, d_track_of_point, d_point, dX);
  HIP_TRY(ctx, hipGetLastError());
  return MSFM_OK;
}

// cam_offset of slam_gps.cc:920-924, once per camera
std::vector<double> gps_cam_offsets(int n_cams, const double* cam_c, const double* gps) {
  std::vector<double> o(3 * (size_t)n_cams);
  for (size_t k = 0; k < o.size(); k++) o[k] = gps[k] - cam_c[k];
  return o;
}

// ---- exports on host arrays ----
static int check_csr(msfm_ctx* ctx, const char* who, int n_tracks, const int32_t* off, const int32_t* cam, int n_cams) {
  if (n_tracks < 0 || n_cams <= 0 || !off) return msfm_set_error(ctx, MSFM_E_INVAL, "%s: null arrays", who);
  MSFM_TRY(msfm_check_offsets(ctx, who, n_tracks, off));
  const int no = off[n_tracks];
  if (no > 0 && !cam) return msfm_set_error(ctx, MSFM_E_INVAL, "%s: null track_cam", who);
  for (int i = 0; i < no; i++) if (cam[i] < 0 || cam[i] >= n_cams) return msfm_set_error(ctx, MSFM_E_INVAL, "%s: track_cam[%d] out of range", who, i);
  return MSFM_OK;
}

MSFM_API int msfm_point_accuracy_batch(msfm_ctx* ctx, const msfm_tracks* T, const double* cam_dc, const double* X, const uint8_t* ok_in, int min_views,
                                       double th_outlier, double* e_avg, double* e_mse, int32_t* n_used, uint8_t* ok_out, int* n_outliers, int* n_inliers) {
  if (!ctx) return MSFM_E_INVAL;
  if (!T || !T->cam_R || !T->cam_t || !T->cam_fk || (T->n_tracks > 0 && (!X || !ok_in || !e_avg || !e_mse || !n_used || !ok_out)))
    return msfm_set_error(ctx, MSFM_E_INVAL, "msfm_point_accuracy_batch: null argument");
  if (!(th_outlier == th_outlier)) return msfm_set_error(ctx, MSFM_E_INVAL, "msfm_point_accuracy_batch: th_outlier is NaN");
  MSFM_TRY(check_csr(ctx, "msfm_point_accuracy_batch", T->n_tracks, T->track_off, T->track_cam, T->n_cams));
  const int n = T->n_tracks, no = T->track_off[n];
  if (no > 0 && !T->track_xy) return msfm_set_error(ctx, MSFM_E_INVAL, "msfm_point_accuracy_batch: null track_xy");
  if (n_outliers) *n_outliers = 0;
  if (n_inliers) *n_inliers = 0;
  if (n == 0) return MSFM_OK;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  const size_t nc = (size_t)T->n_cams;
  DevBuf<int> off, cam, dn, dcount;
  DevBuf<double> xy, R, t, fk, dc, dX, davg, dmse;
  DevBuf<uint8_t> dok, dout;
  DevScope sc(ctx);
  HIP_TRY(ctx, sc.up(off, T->track_off, (size_t)n + 1)); HIP_TRY(ctx, sc.up(cam, T->track_cam, (size_t)no)); HIP_TRY(ctx, sc.up(xy, T->track_xy, 2 * (size_t)no));
  HIP_TRY(ctx, sc.up(R, T->cam_R, 9 * nc)); HIP_TRY(ctx, sc.up(t, T->cam_t, 3 * nc)); HIP_TRY(ctx, sc.up(fk, T->cam_fk, 3 * nc));
  if (cam_dc) HIP_TRY(ctx, sc.up(dc, cam_dc, 2 * nc));
  HIP_TRY(ctx, sc.up(dX, X, 3 * (size_t)n)); HIP_TRY(ctx, sc.up(dok, ok_in, (size_t)n));
  HIP_TRY(ctx, davg.alloc(n)); HIP_TRY(ctx, dmse.alloc(n)); HIP_TRY(ctx, dn.alloc(n)); HIP_TRY(ctx, dout.alloc(n)); HIP_TRY(ctx, dcount.alloc(1));
  const AccuracyPtrs P{n, off.p, cam.p, xy.p, R.p, t.p, fk.p, cam_dc ? dc.p : nullptr, dX.p, dok.p, min_views, th_outlier, davg.p, dmse.p, dn.p, dout.p};
  MSFM_TRY(gps_accuracy_dev(ctx, P, no, dcount.p));
  int outl = 0;
  HIP_TRY(ctx, sc.down(e_avg, davg.p, (size_t)n)); HIP_TRY(ctx, sc.down(e_mse, dmse.p, (size_t)n)); HIP_TRY(ctx, sc.down(n_used, dn.p, (size_t)n));
  HIP_TRY(ctx, sc.down(ok_out, dout.p, (size_t)n)); HIP_TRY(ctx, sc.down(&outl, dcount.p, 1));
  HIP_TRY(ctx, sc.finish());
  if (n_outliers) *n_outliers = outl;
  if (n_inliers) *n_inliers = n - outl;
  return MSFM_OK;
}

MSFM_API int msfm_gps_register_points(msfm_ctx* ctx, int n_tracks, const int32_t* track_off, const int32_t* track_cam, const uint8_t* ok, int n_cams,
                                      const double* cam_c, const double* gps, double* X) {
  if (!ctx) return MSFM_E_INVAL;
  if (!cam_c || !gps || (n_tracks > 0 && (!ok || !X))) return msfm_set_error(ctx, MSFM_E_INVAL, "msfm_gps_register_points: null argument");
  MSFM_TRY(check_csr(ctx, "msfm_gps_register_points", n_tracks, track_off, track_cam, n_cams));
  if (n_tracks == 0) return MSFM_OK;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  const int n = n_tracks, no = track_off[n];
  const std::vector<double> offs = gps_cam_offsets(n_cams, cam_c, gps);
  DevBuf<int> off, cam;
  DevBuf<double> dc, doff, dX;
  DevBuf<uint8_t> dok;
  DevScope sc(ctx);
  HIP_TRY(ctx, sc.up(off, track_off, (size_t)n + 1)); HIP_TRY(ctx, sc.up(cam, track_cam, (size_t)no));
  HIP_TRY(ctx, sc.up(dc, cam_c, 3 * (size_t)n_cams)); HIP_TRY(ctx, sc.up(doff, offs));
  HIP_TRY(ctx, sc.up(dX, X, 3 * (size_t)n)); HIP_TRY(ctx, sc.up(dok, ok, (size_t)n));
  const RegisterPtrs P{n, off.p, cam.p, dok.p, dc.p, doff.p, dX.p};
  MSFM_TRY(gps_register_dev(ctx, P));
  HIP_TRY(ctx, sc.down(X, dX.p, 3 * (size_t)n));
  HIP_TRY(ctx, sc.finish());
  return MSFM_OK;
}

// ---- msfm_gps_orient_global (host) ----
namespace gpr {

struct Rot2 { double c, s; };   // a plane rotation [c s; -s c]

// rows p, q of the 3x3 M (row-major): x' = c x + s y, y' = -s x + c y
static void rot_rows(double* M, int p, int q, Rot2 j) {
  for (int k = 0; k < 3; k++) {
    const double x = M[3 * p + k], y = M[3 * q + k];
    M[3 * p + k] = j.c * x + j.s * y;
    M[3 * q + k] = -j.s * x + j.c * y;
  }
}
// columns p, q of M: x' = c x + s y, y' = -s x + c y  (M <- M j^T)
static void rot_cols(double* M, int p, int q, Rot2 j) {
  for (int k = 0; k < 3; k++) {
    const double x = M[3 * k + p], y = M[3 * k + q];
    M[3 * k + p] = j.c * x + j.s * y;
    M[3 * k + q] = -j.s * x + j.c * y;
  }
}

// The two-sided Jacobi SVD of a real 3x3 matrix as Eigen 3's JacobiSVD documents it: the input scaled by its largest
// magnitude; per pivot pair (p, q), q < p, a 2x2 real SVD - a rotation that makes the block symmetric, then the Jacobi
// rotation that diagonalises it; a pair is skipped while both off-diagonal entries are below 2 eps times the largest diagonal
// entry seen so far; sweeps until no pair rotates; singular values made non-negative (the column of U negated), then sorted
// descending with the column swaps applied to U and V.  A = U diag(S) V^T, all row-major.
static void svd3(const double* A, double* U, double* S, double* V) {
  const double tiny = std::numeric_limits<double>::min(), precision = 2.0 * std::numeric_limits<double>::epsilon();
  double scale = 0.0;
  for (int k = 0; k < 9; k++) scale = std::max(scale, std::fabs(A[k]));
  if (scale == 0.0) scale = 1.0;
  double W[9];
  for (int k = 0; k < 9; k++) { W[k] = A[k] / scale; U[k] = V[k] = (k % 4 == 0) ? 1.0 : 0.0; }
  double max_diag = std::max(std::fabs(W[0]), std::max(std::fabs(W[4]), std::fabs(W[8])));
  bool finished = false;
  while (!finished) {
    finished = true;
    for (int p = 1; p < 3; p++)
      for (int q = 0; q < p; q++) {
        const double threshold = std::max(tiny, precision * max_diag);
        if (!(std::fabs(W[3 * p + q]) > threshold || std::fabs(W[3 * q + p]) > threshold)) continue;
        finished = false;
        // the 2x2 block [[W(p,p), W(p,q)], [W(q,p), W(q,q)]]
        double m00 = W[3 * p + p], m01 = W[3 * p + q], m10 = W[3 * q + p], m11 = W[3 * q + q];
        Rot2 rot1;
        const double t = m00 + m11, d = m10 - m01;
        if (std::fabs(d) < tiny) {
          rot1 = Rot2{1.0, 0.0};
        } else {
          const double u = t / d, tmp = std::sqrt(1.0 + u * u);
          rot1 = Rot2{u / tmp, 1.0 / tmp};
        }
        {   // rot1 on the block's rows
          const double a0 = rot1.c * m00 + rot1.s * m10, a1 = rot1.c * m01 + rot1.s * m11;
          const double b1 = -rot1.s * m01 + rot1.c * m11;
          m00 = a0; m01 = a1; m11 = b1;
        }
        Rot2 jr;
        const double deno = 2.0 * std::fabs(m01);
        if (deno < tiny) {
          jr = Rot2{1.0, 0.0};
        } else {
          const double tau = (m00 - m11) / deno, w = std::sqrt(tau * tau + 1.0);
          const double tt = tau > 0.0 ? 1.0 / (tau + w) : 1.0 / (tau - w);
          const double sign_t = tt > 0.0 ? 1.0 : -1.0, n = 1.0 / std::sqrt(tt * tt + 1.0);
          jr = Rot2{n, -sign_t * (m01 / std::fabs(m01)) * std::fabs(tt) * n};
        }
        const Rot2 jl{rot1.c * jr.c + rot1.s * jr.s, rot1.s * jr.c - rot1.c * jr.s};   // rot1 * jr^T
        rot_rows(W, p, q, jl);
        rot_cols(U, p, q, jl);                    // U <- U jl^T
        rot_cols(W, p, q, Rot2{jr.c, -jr.s});     // W <- W jr
        rot_cols(V, p, q, Rot2{jr.c, -jr.s});     // V <- V jr
        max_diag = std::max(max_diag, std::max(std::fabs(W[3 * p + p]), std::fabs(W[3 * q + q])));
      }
  }
  for (int i = 0; i < 3; i++) {
    const double a = W[4 * i];
    S[i] = std::fabs(a);
    if (a < 0.0) for (int k = 0; k < 3; k++) U[3 * k + i] = -U[3 * k + i];
  }
  for (int i = 0; i < 3; i++) S[i] *= scale;
  for (int i = 0; i < 3; i++) {
    int pos = i;
    for (int k = i + 1; k < 3; k++) if (S[k] > S[pos]) pos = k;
    if (S[pos] == 0.0) break;
    if (pos != i) {
      std::swap(S[i], S[pos]);
      for (int k = 0; k < 3; k++) { std::swap(U[3 * k + i], U[3 * k + pos]); std::swap(V[3 * k + i], V[3 * k + pos]); }
    }
  }
}

static void mul33(const double* A, const double* B, double* C) {
  for (int r = 0; r < 3; r++)
    for (int c = 0; c < 3; c++) C[3 * r + c] = A[3 * r] * B[c] + A[3 * r + 1] * B[3 + c] + A[3 * r + 2] * B[6 + c];
}
static void mul31(const double* A, const double* x, double* y) {
  for (int r = 0; r < 3; r++) y[r] = A[3 * r] * x[0] + A[3 * r + 1] * x[1] + A[3 * r + 2] * x[2];
}
static double det33(const double* A) {
  return A[0] * (A[4] * A[8] - A[5] * A[7]) - A[1] * (A[3] * A[8] - A[5] * A[6]) + A[2] * (A[3] * A[7] - A[4] * A[6]);
}
// cofactors times 1 / det
static void inv33(const double* A, double* I) {
  const double c00 = A[4] * A[8] - A[5] * A[7], c01 = A[5] * A[6] - A[3] * A[8], c02 = A[3] * A[7] - A[4] * A[6];
  const double invdet = 1.0 / (A[0] * c00 + A[1] * c01 + A[2] * c02);
  I[0] = c00 * invdet; I[1] = (A[2] * A[7] - A[1] * A[8]) * invdet; I[2] = (A[1] * A[5] - A[2] * A[4]) * invdet;
  I[3] = c01 * invdet; I[4] = (A[0] * A[8] - A[2] * A[6]) * invdet; I[5] = (A[2] * A[3] - A[0] * A[5]) * invdet;
  I[6] = c02 * invdet; I[7] = (A[1] * A[6] - A[0] * A[7]) * invdet; I[8] = (A[0] * A[4] - A[1] * A[3]) * invdet;
}

// rotation::RotationMatrixToAngleAxis (SfM/src/utils/basic_funcs.cc), the statement of host/objectsfm.cc on a row-major R
static void rot_to_aa(const double* R, double* axis) {
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

// Camera::Transformation (camera.cc:79-87)
static void cam_transform(double* R, double* t, double* c, double* aa, const double* Rg, const double* tg, double scale) {
  double Ri[9], Rn[9], sR[9], rc[3];
  inv33(Rg, Ri);
  mul33(R, Ri, Rn);
  for (int k = 0; k < 9; k++) { R[k] = Rn[k]; sR[k] = scale * Rg[k]; }
  mul31(sR, c, rc);
  for (int k = 0; k < 3; k++) c[k] = rc[k] + tg[k];
  mul31(R, c, rc);
  for (int k = 0; k < 3; k++) t[k] = -rc[k];
  rot_to_aa(R, aa);
}

}  // namespace gpr

MSFM_API void msfm_gpsreg_default_options(msfm_gpsreg_options* o) {
  if (!o) return;
  o->window = 20; o->min_views = 3; o->clip_deg = 80.0; o->th_outlier = 3.0;
}

MSFM_API int msfm_gps_orient_global(int n_cams, const double* cam_R, const double* cam_c, const double* gps_in, const msfm_gpsreg_options* opt,
                                    msfm_gps_orient_result* out) {
  using namespace gpr;
  if (n_cams < 3 || !cam_R || !cam_c || !gps_in || !out || !out->cam_R || !out->cam_t || !out->cam_c || !out->cam_aa || !out->gps || !out->weight)
    return MSFM_E_INVAL;
  msfm_gpsreg_options o;
  msfm_gpsreg_default_options(&o);
  if (opt) o = *opt;
  if (o.window < 0 || !(o.clip_deg >= 0.0 && o.clip_deg < 90.0)) return MSFM_E_INVAL;
  const int n = n_cams;
  const double pi = 3.1415926535897932384626433832795;   // CV_PI
  // ---- the weights, slam_gps.cc:1606-1624 ----
  for (int i = 0; i < n; i++) {
    const int ids = std::max(0, i - o.window), ide = std::min(n - 1, i + o.window);
    const double dxs = gps_in[3 * ids] - gps_in[3 * i], dys = gps_in[3 * ids + 1] - gps_in[3 * i + 1];
    const double dxe = gps_in[3 * ide] - gps_in[3 * i], dye = gps_in[3 * ide + 1] - gps_in[3 * i + 1];
    double angle = std::acos((dxs * dxe + dys * dye) / std::sqrt(dxs * dxs + dys * dys + 0.1) / std::sqrt(dxe * dxe + dye * dye + 0.1));
    angle = std::fabs(angle - pi);
    if (angle >= pi * o.clip_deg / 180.0) angle = pi * o.clip_deg / 180.0;
    out->weight[i] = std::tan(angle);
  }
  // ---- SimilarityTransformation, utils/transformation.cpp:155-213 (src = centres, dst = GPS) ----
  double sc[3] = {0, 0, 0}, dc[3] = {0, 0, 0};
  for (int i = 0; i < n; i++) for (int k = 0; k < 3; k++) { sc[k] += cam_c[3 * i + k]; dc[k] += gps_in[3 * i + k]; }
  for (int k = 0; k < 3; k++) { sc[k] /= n; dc[k] /= n; }
  double cov[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, s_mv = 0.0;
  for (int i = 0; i < n; i++) {
    double ds[3], dd[3];
    for (int k = 0; k < 3; k++) { ds[k] = cam_c[3 * i + k] - sc[k]; dd[k] = gps_in[3 * i + k] - dc[k]; }
    s_mv += (ds[0] * ds[0] + ds[1] * ds[1] + ds[2] * ds[2]) * out->weight[i];
    for (int r = 0; r < 3; r++) for (int c = 0; c < 3; c++) cov[3 * r + c] += ds[r] * dd[c] * out->weight[i];
  }
  s_mv /= n;
  for (int k = 0; k < 9; k++) cov[k] /= n;
  double U[9], S[3], V[9], Ut[9], VUt[9], VZ[9];
  svd3(cov, U, S, V);
  for (int r = 0; r < 3; r++) for (int c = 0; c < 3; c++) Ut[3 * r + c] = U[3 * c + r];
  mul33(V, Ut, VUt);
  const double Z[3] = {1.0, 1.0, det33(VUt)};
  for (int r = 0; r < 3; r++) for (int c = 0; c < 3; c++) VZ[3 * r + c] = V[3 * r + c] * Z[c];
  double* Rg = out->Rg;
  mul33(VZ, Ut, Rg);
  const double scale = (S[0] * Z[0] + S[1] * Z[1] + S[2] * Z[2]) / s_mv;
  double sR[9], v[3];
  for (int k = 0; k < 9; k++) sR[k] = -scale * Rg[k];
  mul31(sR, sc, v);
  for (int k = 0; k < 3; k++) out->tg[k] = v[k] + dc[k];
  for (int k = 0; k < 9; k++) sR[k] = scale * Rg[k];
  double sum_err = 0.0;
  for (int i = 0; i < n; i++) {
    mul31(sR, cam_c + 3 * i, v);
    const double d0 = v[0] + out->tg[0] - gps_in[3 * i], d1 = v[1] + out->tg[1] - gps_in[3 * i + 1], d2 = v[2] + out->tg[2] - gps_in[3 * i + 2];
    sum_err += std::sqrt(d0 * d0 + d1 * d1 + d2 * d2);
  }
  out->scale = scale;
  out->err = sum_err / n;
  // ---- the cameras into the GPS frame, then everything re-centred on gps_offset_ (slam_gps.cc:1638-1673) ----
  for (int i = 0; i < n; i++) {
    for (int k = 0; k < 9; k++) out->cam_R[9 * (size_t)i + k] = cam_R[9 * (size_t)i + k];
    for (int k = 0; k < 3; k++) out->cam_c[3 * (size_t)i + k] = cam_c[3 * (size_t)i + k];
    cam_transform(out->cam_R + 9 * (size_t)i, out->cam_t + 3 * (size_t)i, out->cam_c + 3 * (size_t)i, out->cam_aa + 3 * (size_t)i, Rg, out->tg, scale);
  }
  double off[3] = {0, 0, 0};
  for (int i = 0; i < n; i++) for (int k = 0; k < 3; k++) off[k] += out->cam_c[3 * (size_t)i + k];
  for (int k = 0; k < 3; k++) { off[k] /= n; out->offset[k] = off[k]; }
  const double eye[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, neg[3] = {-off[0], -off[1], -off[2]};
  for (int i = 0; i < n; i++)
    cam_transform(out->cam_R + 9 * (size_t)i, out->cam_t + 3 * (size_t)i, out->cam_c + 3 * (size_t)i, out->cam_aa + 3 * (size_t)i, eye, neg, 1.0);
  for (int i = 0; i < n; i++) for (int k = 0; k < 3; k++) out->gps[3 * (size_t)i + k] = gps_in[3 * (size_t)i + k] - off[k];
  return MSFM_OK;
}
