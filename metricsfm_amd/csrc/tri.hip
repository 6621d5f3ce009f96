// Batched triangulation / reprojection / epipolar filter (FP64).
// Round 4: the midpoint triangulation and the reprojection run in two kinds of phases inside one workgroup of 64 tracks - what
// belongs to ONE observation (its ray, its reprojection error, its ray for the angle gate: all the loads, divisions and square
// roots) is computed with lane = observation from coalesced reads and parked in LDS; what the reference SUMS over a track's
// observations in their order is then done by one thread per track from LDS.  Both forms call the same functions of
// point3d_device.h - a ray, a row error, the ordered sum are each stated there once - so every number is formed by the same
// operations in the same order as in the thread-per-track form (which remains: DLT, and workgroups whose observations do not
// fit the LDS area); tests/test_gpu_tri.py::test_both_workgroup_forms_give_the_same_bits holds the two to the same bits.
// The kernel no longer waits for a chain of dependent loads per observation.
// Reference: Point3D::Trianglate2 SfM/src/structure.cc:211-265, Point3D::Trianglate (DLT)
// :163-209, Point3D::Reprojection :267-300, Point3D::SufficientTriangulationAngle :325-355,
// GeoVerification::GeoVerificationFundamental (closed form) SfM/src/utils/geo_verification.cc:60-79.
#include "common.h"
#include "point3d_device.h"   // contracted here, as the compiler's default has it

// the squared reprojection error of observation i for the point X, -1.0 at negative depth
__device__ __forceinline__ double obs_error(const TrackPtrs& T, int i, const double* X) {
  const size_t c = (size_t)T.cam[i];
  return p3d_row_error(T.R + 9 * c, T.t + 3 * c, T.fk + 3 * c, X, T.xy[2 * (size_t)i], T.xy[2 * (size_t)i + 1]);
}

// structure.cc:267-300
__device__ double track_mse(const TrackPtrs& T, int b, int e, const double* X) {
  return p3d_ordered_mse(b, e, [&](int i) { return obs_error(T, i, X); });
}

// structure.cc:325-355
__device__ bool track_angle_ok(const TrackPtrs& T, int b, int e, const double* X, double cos_min) {
  for (int i = b; i + 1 < e; i++) {
    double a[3];
    p3d_direction(T.c + 3 * (size_t)T.cam[i], X, a);
    for (int j = i + 1; j < e; j++) {
      double d[3];
      p3d_direction(T.c + 3 * (size_t)T.cam[j], X, d);
      if (p3d_pair_wide(a, d, cos_min)) return true;
    }
  }
  return false;
}

// what every thread-per-track form ends in: the point, its Reprojection, the verdict
__device__ __forceinline__ void track_finish(const TrackPtrs& T, int t, int b, int e, const double* X, double th_error, double cos_min,
                                             double* __restrict__ Xo, double* __restrict__ mse, uint8_t* __restrict__ ok) {
  Xo[3 * (size_t)t] = X[0]; Xo[3 * (size_t)t + 1] = X[1]; Xo[3 * (size_t)t + 2] = X[2];
  const double m = track_mse(T, b, e, X);
  mse[t] = m;
  ok[t] = p3d_accepted(m, th_error, track_angle_ok(T, b, e, X, cos_min));
}

__device__ __forceinline__ void tri_midpoint_track(const TrackPtrs& T, int t, double th_error, double cos_min, double* __restrict__ Xo,
                                                   double* __restrict__ mse, uint8_t* __restrict__ ok) {
  const int b = T.off[t], e = T.off[t + 1];
  double A[16], bv[4] = {0, 0, 0, 0};
#pragma unroll
  for (int k = 0; k < 16; k++) A[k] = 0.0;
  for (int i = b; i < e; i++) {
    const size_t c = (size_t)T.cam[i];
    double d[3];
    p3d_ray(T.R + 9 * c, T.fk[3 * c], T.xy[2 * (size_t)i], T.xy[2 * (size_t)i + 1], d);
    p3d_accumulate(d, T.c + 3 * c, A, bv);
  }
  ok[t] = 0;
  mse[t] = 0.0;
  double X[3];
  if (p3d_solve(A, bv, X)) track_finish(T, t, b, e, X, th_error, cos_min, Xo, mse, ok);
}

// ---- the staged form: 64 tracks per workgroup, observations through LDS ----
#define TRI_TPB 64      // tracks per workgroup
#define TRI_CAP 768     // observations per workgroup that fit the LDS area (else: thread per track)
#define TRI_REC 7       // doubles per observation: ray (3), centre (3), squared reprojection error
__global__ __launch_bounds__(256) void k_tri_midpoint_staged(TrackPtrs T, double th_error, double cos_min, double* __restrict__ Xo,
                                                              double* __restrict__ mse, uint8_t* __restrict__ ok) {
  __shared__ double sd[TRI_CAP * TRI_REC];
  __shared__ double Xs[TRI_TPB * 3];
  __shared__ int offs[TRI_TPB + 1];
  __shared__ short tk[TRI_CAP];
  __shared__ unsigned char alive[TRI_TPB];
  const int tid = threadIdx.x, t0 = blockIdx.x * TRI_TPB;
  const int nt = min(TRI_TPB, T.n_tracks - t0);
  if (tid <= nt) offs[tid] = T.off[t0 + tid];
  __syncthreads();
  const int ob = offs[0], nobs = offs[nt] - ob;
  if (nobs > TRI_CAP) {   // (uniform) long tracks: the thread-per-track form for this workgroup
    if (tid < nt) tri_midpoint_track(T, t0 + tid, th_error, cos_min, Xo, mse, ok);
    return;
  }
  // -- per observation: the unit ray through the image point in world coordinates, the camera centre (structure.cc:224-236)
  for (int j = tid; j < nobs; j += 256) {
    const int i = ob + j;
    const size_t c = (size_t)T.cam[i];
    const double* o = T.c + 3 * c;
    double d[3];
    p3d_ray(T.R + 9 * c, T.fk[3 * c], T.xy[2 * (size_t)i], T.xy[2 * (size_t)i + 1], d);
    double* rec = sd + (size_t)j * TRI_REC;
    rec[0] = d[0]; rec[1] = d[1]; rec[2] = d[2]; rec[3] = o[0]; rec[4] = o[1]; rec[5] = o[2];
  }
  __syncthreads();
  // -- per track: the sums over its observations in their order, the 4 x 4 LLT (structure.cc:237-258)
  if (tid < nt) {
    const int t = t0 + tid, b = offs[tid] - ob, e = offs[tid + 1] - ob;
    double A[16], bv[4] = {0, 0, 0, 0};
#pragma unroll
    for (int k = 0; k < 16; k++) A[k] = 0.0;
    for (int j = b; j < e; j++) {
      const double* rec = sd + (size_t)j * TRI_REC;
      tk[j] = (short)tid;
      p3d_accumulate(rec, rec + 3, A, bv);
    }
    ok[t] = 0;
    mse[t] = 0.0;
    double X[3];
    const bool pd = p3d_solve(A, bv, X);
    alive[tid] = pd ? 1 : 0;
    if (pd) {
      Xo[3 * (size_t)t] = X[0]; Xo[3 * (size_t)t + 1] = X[1]; Xo[3 * (size_t)t + 2] = X[2];
      Xs[3 * tid] = X[0]; Xs[3 * tid + 1] = X[1]; Xs[3 * tid + 2] = X[2];
    }
  }
  __syncthreads();
  // -- per observation: squared reprojection error (structure.cc:267-300; negative depth is flagged) and the unit ray from the
  //    camera centre to the point (:325-355)
  for (int j = tid; j < nobs; j += 256) {
    const int trk = tk[j];
    if (!alive[trk]) continue;
    const double X[3] = {Xs[3 * trk], Xs[3 * trk + 1], Xs[3 * trk + 2]};
    double* rec = sd + (size_t)j * TRI_REC;
    const double err = obs_error(T, ob + j, X);
    double a[3];
    p3d_direction(rec + 3, X, a);
    rec[0] = a[0]; rec[1] = a[1]; rec[2] = a[2]; rec[6] = err;
  }
  __syncthreads();
  // -- per track: the error sum in observation order, the angle gate over the pairs of rays
  if (tid < nt && alive[tid]) {
    const int t = t0 + tid, b = offs[tid] - ob, e = offs[tid + 1] - ob;
    const double m = p3d_ordered_mse(b, e, [&](int j) { return sd[(size_t)j * TRI_REC + 6]; });
    mse[t] = m;
    bool wide = false;
    for (int i = b; i + 1 < e && !wide; i++)
      for (int j = i + 1; j < e; j++)
        if (p3d_pair_wide(sd + (size_t)i * TRI_REC, sd + (size_t)j * TRI_REC, cos_min)) { wide = true; break; }
    ok[t] = p3d_accepted(m, th_error, wide);
  }
}

// Reprojection only (RemovePointOutliers, sfm_incremental.cc:1831-1863): the errors with lane = observation, the sums per track.
__global__ __launch_bounds__(256) void k_reproject_staged(TrackPtrs T, const double* __restrict__ X, double* __restrict__ mse) {
  __shared__ double er_s[TRI_CAP];
  __shared__ int offs[TRI_TPB + 1];
  const int tid = threadIdx.x, t0 = blockIdx.x * TRI_TPB;
  const int nt = min(TRI_TPB, T.n_tracks - t0);
  if (tid <= nt) offs[tid] = T.off[t0 + tid];
  __syncthreads();
  const int ob = offs[0], nobs = offs[nt] - ob;
  if (nobs > TRI_CAP) {
    if (tid < nt) {
      const int t = t0 + tid;
      const double Xt[3] = {X[3 * (size_t)t], X[3 * (size_t)t + 1], X[3 * (size_t)t + 2]};
      mse[t] = track_mse(T, T.off[t], T.off[t + 1], Xt);
    }
    return;
  }
  for (int j = tid; j < nobs; j += 256) {
    const int i = ob + j;
    int lo = 0, hi = nt - 1;   // the track of observation i: the last one whose first observation is <= i
    while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (offs[mid] <= i) lo = mid; else hi = mid - 1; }
    er_s[j] = obs_error(T, i, X + 3 * (size_t)(t0 + lo));
  }
  __syncthreads();
  if (tid < nt) {
    const int b = offs[tid] - ob, e = offs[tid + 1] - ob;
    mse[t0 + tid] = p3d_ordered_mse(b, e, [&](int j) { return er_s[j]; });
  }
}

// DLT: streaming Givens QR of the 2k x 4 design matrix, one-sided Jacobi SVD of the 4x4 factor.
__global__ __launch_bounds__(256) void k_tri_dlt(TrackPtrs T, double th_error, double cos_min, double* __restrict__ Xo,
                                                  double* __restrict__ mse, uint8_t* __restrict__ ok) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= T.n_tracks) return;
  const int b = T.off[t], e = T.off[t + 1];
  ok[t] = 0;
  mse[t] = 0.0;
  if (e - b < 2) return;
  double Rf[16];
#pragma unroll
  for (int k = 0; k < 16; k++) Rf[k] = 0.0;
  for (int i = b; i < e; i++) {
    const int c = T.cam[i];
    const double* R = T.R + 9 * (size_t)c;
    const double* tt = T.t + 3 * (size_t)c;
    const double f = T.fk[3 * (size_t)c];
    const double x = T.xy[2 * (size_t)i], y = T.xy[2 * (size_t)i + 1];
    const double M0[4] = {R[0], R[1], R[2], tt[0]}, M1[4] = {R[3], R[4], R[5], tt[1]}, M2[4] = {R[6], R[7], R[8], tt[2]};
#pragma unroll
    for (int rr = 0; rr < 2; rr++) {
      double v[4];
#pragma unroll
      for (int q = 0; q < 4; q++) v[q] = rr == 0 ? (-M1[q] * f + M2[q] * y) : (M0[q] * f - M2[q] * x);
#pragma unroll
      for (int j = 0; j < 4; j++) {
        if (v[j] != 0.0) {
          const double a = Rf[j * 4 + j], bb = v[j];
          const double h = hypot(a, bb);
          const double cs = a / h, sn = bb / h;
#pragma unroll
          for (int q = j; q < 4; q++) {
            const double rj = Rf[j * 4 + q], vq = v[q];
            Rf[j * 4 + q] = cs * rj + sn * vq;
            v[q] = -sn * rj + cs * vq;
          }
        }
      }
    }
  }
  double V[16];
#pragma unroll
  for (int k = 0; k < 16; k++) V[k] = (k % 5 == 0) ? 1.0 : 0.0;
  for (int sweep = 0; sweep < 30; sweep++) {
    bool rotated = false;
#pragma unroll
    for (int p = 0; p < 3; p++)
#pragma unroll
      for (int q = p + 1; q < 4; q++) {
        double alpha = 0, beta = 0, gamma = 0;
#pragma unroll
        for (int r = 0; r < 4; r++) {
          alpha += Rf[r * 4 + p] * Rf[r * 4 + p];
          beta += Rf[r * 4 + q] * Rf[r * 4 + q];
          gamma += Rf[r * 4 + p] * Rf[r * 4 + q];
        }
        if (!(fabs(gamma) <= 1e-15 * sqrt(alpha * beta) || gamma == 0.0)) {
          rotated = true;
          const double zeta = (beta - alpha) / (2.0 * gamma);
          const double tn = (zeta >= 0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
          const double cs = 1.0 / sqrt(1.0 + tn * tn), sn = cs * tn;
#pragma unroll
          for (int r = 0; r < 4; r++) {
            const double rp = Rf[r * 4 + p], rq = Rf[r * 4 + q];
            Rf[r * 4 + p] = cs * rp - sn * rq;
            Rf[r * 4 + q] = sn * rp + cs * rq;
            const double vp = V[r * 4 + p], vq = V[r * 4 + q];
            V[r * 4 + p] = cs * vp - sn * vq;
            V[r * 4 + q] = sn * vp + cs * vq;
          }
        }
      }
    if (!rotated) break;
  }
  double bn = 0.0, v0 = 0, v1 = 0, v2 = 0, v3 = 1;
#pragma unroll
  for (int q = 0; q < 4; q++) {
    double nn = 0;
#pragma unroll
    for (int r = 0; r < 4; r++) nn += Rf[r * 4 + q] * Rf[r * 4 + q];
    if (q == 0 || nn < bn) { bn = nn; v0 = V[q]; v1 = V[4 + q]; v2 = V[8 + q]; v3 = V[12 + q]; }
  }
  const double X[3] = {v0 / v3, v1 / v3, v2 / v3};
  track_finish(T, t, b, e, X, th_error, cos_min, Xo, mse, ok);
}

struct F9 { double f[9]; };
__global__ __launch_bounds__(256) void k_epipolar(const float* __restrict__ pt1, const float* __restrict__ pt2, int n, F9 F, double th,
                                                   uint8_t* __restrict__ inlier) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const double x1 = pt1[2 * (size_t)i], y1 = pt1[2 * (size_t)i + 1], x2 = pt2[2 * (size_t)i], y2 = pt2[2 * (size_t)i + 1];
  double l0 = F.f[0] * x1 + F.f[1] * y1 + F.f[2], l1 = F.f[3] * x1 + F.f[4] * y1 + F.f[5], l2 = F.f[6] * x1 + F.f[7] * y1 + F.f[8];
  const double nn = sqrt(l0 * l0 + l1 * l1);
  l0 /= nn; l1 /= nn; l2 /= nn;
  inlier[i] = fabs(l0 * x2 + l1 * y2 + l2) < th;
}

// ---- host ----
struct TrackDev {
  DevBuf<int> off, cam;
  DevBuf<double> xy, R, t, c, fk;
  TrackPtrs ptrs;
};

static int upload_tracks(msfm_ctx* ctx, const msfm_tracks* T, TrackDev& D, DevScope& sc) {   // (D lives in front of the caller's scope)
  if (!ctx || !T || T->n_tracks < 0 || T->n_cams <= 0 || !T->track_off || !T->cam_R || !T->cam_t || !T->cam_c || !T->cam_fk)
    return msfm_set_error(ctx, MSFM_E_INVAL, "tracks: null arrays");
  const int n = T->n_tracks;
  if (T->track_off[0] != 0) return msfm_set_error(ctx, MSFM_E_INVAL, "track_off[0] != 0");
  for (int i = 0; i < n; i++) if (T->track_off[i + 1] < T->track_off[i]) return msfm_set_error(ctx, MSFM_E_INVAL, "track_off not monotone");
  const int no = T->track_off[n];
  for (int i = 0; i < no; i++) if (T->track_cam[i] < 0 || T->track_cam[i] >= T->n_cams) return msfm_set_error(ctx, MSFM_E_INVAL, "track_cam[%d] out of range", i);
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  const size_t nc = (size_t)T->n_cams;
  HIP_TRY(ctx, sc.up(D.off, T->track_off, (size_t)n + 1)); HIP_TRY(ctx, sc.up(D.cam, T->track_cam, (size_t)no));
  HIP_TRY(ctx, sc.up(D.xy, T->track_xy, 2 * (size_t)no));
  HIP_TRY(ctx, sc.up(D.R, T->cam_R, 9 * nc)); HIP_TRY(ctx, sc.up(D.t, T->cam_t, 3 * nc)); HIP_TRY(ctx, sc.up(D.c, T->cam_c, 3 * nc));
  HIP_TRY(ctx, sc.up(D.fk, T->cam_fk, 3 * nc));
  D.ptrs = TrackPtrs{n, D.off.p, D.cam.p, D.xy.p, D.R.p, D.t.p, D.c.p, D.fk.p};
  return MSFM_OK;
}

static int triangulate(msfm_ctx* ctx, const msfm_tracks* T, double th_error, double th_angle, double* X, double* mse, uint8_t* ok,
                       bool dlt) {
  if (!X || !mse || !ok) return MSFM_E_INVAL;
  TrackDev D;
  DevBuf<double> dX, dm;
  DevBuf<uint8_t> dok;
  DevScope sc(ctx);
  MSFM_TRY(upload_tracks(ctx, T, D, sc));
  const int n = T->n_tracks;
  if (n == 0) return MSFM_OK;   // (the scope waits for the uploads)
  hipStream_t s = ctx->stream;
  HIP_TRY(ctx, dm.alloc(n)); HIP_TRY(ctx, dok.alloc(n));
  HIP_TRY(ctx, sc.up(dX, X, 3 * (size_t)n));  // X is in/out: untouched on LLT failure
  {
    KTimer t(ctx, dlt ? "tri_dlt" : "tri_midpoint");
    if (dlt) hipLaunchKernelGGL(k_tri_dlt, dim3(cdiv(n, 256)), dim3(256), 0, s, D.ptrs, th_error, cos(th_angle), dX.p, dm.p, dok.p);
    else hipLaunchKernelGGL(k_tri_midpoint_staged, dim3(cdiv(n, TRI_TPB)), dim3(256), 0, s, D.ptrs, th_error, cos(th_angle), dX.p, dm.p, dok.p);
  }
  HIP_TRY(ctx, hipGetLastError());
  HIP_TRY(ctx, sc.down(X, dX.p, 3 * (size_t)n)); HIP_TRY(ctx, sc.down(mse, dm.p, (size_t)n)); HIP_TRY(ctx, sc.down(ok, dok.p, (size_t)n));
  HIP_TRY(ctx, sc.finish());
  return MSFM_OK;
}

// Point3D::Trianglate2 + Reprojection + the angle gate on tracks that are already resident (all pointers device memory);
// X is in/out.  msfm_chain_triangulate (chain.hip) calls it on the tracks it built.
int tri_midpoint_dev(msfm_ctx* ctx, const TrackPtrs& T, double th_error, double th_angle, double* dX, double* dmse, uint8_t* dok) {
  if (T.n_tracks == 0) return MSFM_OK;
  KTimer t(ctx, "tri_midpoint");
  hipLaunchKernelGGL(k_tri_midpoint_staged, dim3(cdiv(T.n_tracks, TRI_TPB)), dim3(256), 0, ctx->stream, T, th_error, cos(th_angle), dX, dmse, dok);
  HIP_TRY(ctx, hipGetLastError());
  return MSFM_OK;
}

MSFM_API int msfm_triangulate_midpoint_batch(msfm_ctx* ctx, const msfm_tracks* T, double th_error, double th_angle, double* X,
                                             double* mse, uint8_t* ok) {
  if (!ctx) return MSFM_E_INVAL;
  return triangulate(ctx, T, th_error, th_angle, X, mse, ok, false);
}

MSFM_API int msfm_triangulate_dlt_batch(msfm_ctx* ctx, const msfm_tracks* T, double th_error, double th_angle, double* X,
                                        double* mse, uint8_t* ok) {
  if (!ctx) return MSFM_E_INVAL;
  return triangulate(ctx, T, th_error, th_angle, X, mse, ok, true);
}

MSFM_API int msfm_reproject_mse_batch(msfm_ctx* ctx, const msfm_tracks* T, const double* X, double* mse) {
  if (!ctx || !X || !mse) return MSFM_E_INVAL;
  TrackDev D;
  DevBuf<double> dX, dm;
  DevScope sc(ctx);
  MSFM_TRY(upload_tracks(ctx, T, D, sc));
  const int n = T->n_tracks;
  if (n == 0) return MSFM_OK;   // (the scope waits for the uploads)
  hipStream_t s = ctx->stream;
  HIP_TRY(ctx, dm.alloc(n));
  HIP_TRY(ctx, sc.up(dX, X, 3 * (size_t)n));
  {
    KTimer t(ctx, "tri_reproject");
    hipLaunchKernelGGL(k_reproject_staged, dim3(cdiv(n, TRI_TPB)), dim3(256), 0, s, D.ptrs, dX.p, dm.p);
  }
  HIP_TRY(ctx, hipGetLastError());
  HIP_TRY(ctx, sc.down(mse, dm.p, (size_t)n));
  HIP_TRY(ctx, sc.finish());
  return MSFM_OK;
}

MSFM_API int msfm_epipolar_filter(msfm_ctx* ctx, const float* pt1, const float* pt2, int n, const double F[9], double th,
                                  uint8_t* inlier) {
  if (!ctx || n < 0 || (n > 0 && (!pt1 || !pt2 || !inlier)) || !F) return MSFM_E_INVAL;
  if (n == 0) return MSFM_OK;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  DevBuf<float> d1, d2;
  DevBuf<uint8_t> di;
  DevScope sc(ctx);
  HIP_TRY(ctx, sc.up(d1, pt1, 2 * (size_t)n)); HIP_TRY(ctx, sc.up(d2, pt2, 2 * (size_t)n)); HIP_TRY(ctx, di.alloc(n));
  F9 f;
  for (int k = 0; k < 9; k++) f.f[k] = F[k];
  hipLaunchKernelGGL(k_epipolar, dim3(cdiv(n, 256)), dim3(256), 0, s, d1.p, d2.p, n, f, th, di.p);
  HIP_TRY(ctx, hipGetLastError());
  HIP_TRY(ctx, sc.down(inlier, di.p, (size_t)n));
  HIP_TRY(ctx, sc.finish());
  return MSFM_OK;
}
