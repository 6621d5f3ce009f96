// The second half of a round of IncrementalSfM::Run (SfM/src/sfm_incremental.cc:172-186) on the flat state, in one call:
//   PartialBundleAdjustment(new_cam)   :917-1014     FullBundleAdjustment   :1016-1026     RemovePointOutliers   :1831-1863
// The state keeps both sides of the object graph: feat_point is Camera::pts_ (the masks walk it, :1865-1893, :922-945), the
// obs_* rows are Point3D::cams_ / pts2d_ (the solver's gather walks them, optimizer.cc:80-82, and so does
// Point3D::Reprojection, structure.cc:267-300).
//
//   host        O(cameras): image ranks, the free cameras of the partial stage, the camera tables
//   k_check     feat_point and the obs_* rows against their arrays (the first read-back carries the answer; every kernel in
//               front of it steps over what k_check reports), and the 64-bit key of a row: point << 32 | image rank << b_f | feature
//   sort        ONE rocPRIM radix sort of the keys: a point's rows in std::map order of cams_ (structure.cc:134)
//   k_first     the first row of every distinct key (std::map::insert keeps one), views per point; k_segments: every point's rows
//   k_attach    over feat_point: attached points, and points a free camera frees; k_pt_mutable combines them with the incoming flag
//   k_keep      row and point predicates of the compact problem, two exclusive scans (the shape of chain.hip's k_keep / k_ba_arrays)
//   k_emit      obs_cam, obs_pt, obs_xy, pt_weight, point, pt_mutable, kept
//   solve       ba_create_impl(bulk_on_device) + msfm_ba_run, as msfm_chain_ba_create; k_scatter_points puts the result back
//   k_outliers  one thread per point over its sorted segment: Reprojection and the flags of RemovePointOutliers
// The host waits where it needs a count - the sizes of a stage's problem, what the solve does itself - and at the end.
// The call is three parts: round_tables (the checks that need no bulk array, the O(cameras) tables), round_adjust_dev (everything on
// device arrays, written in place) and the export, which uploads the bulk arrays in front of the core and reads the points back
// behind it.  recon.hip calls the first two on the arrays a msfm_recon keeps resident.
// k_outliers is Reprojection as point3d_device.h states it, compiled without fused multiply-adds, + - * / sqrt only (the
// discipline of newpoints.hip and seed.hip): tests/round_ref.py, a sequential restatement in doubles, agrees bit for bit.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>
#include <memory>
#include <numeric>

#include "prim_device.h"

#pragma clang fp contract(off)
#include "point3d_device.h"   // p3d_row_error, p3d_ordered_mse

namespace adj {

#define ADJ_CAM 15    // R (9), t (3), fk (3)
#define ADJ_BIG 0x7fffffff

__global__ __launch_bounds__(256) void k_check_points(int FP, int n_points, const int* __restrict__ fp, int* __restrict__ err) {
  const int x = blockIdx.x * 256 + threadIdx.x;
  if (x < FP && fp[x] >= n_points) atomicMin(err, x);
}

// the key of row i; a row with an index outside its array is reported and gets the key of "point n_points", behind every point
__global__ __launch_bounds__(256) void k_key(int n_obs, int n_points, int n_cams, const int* __restrict__ obs_point, const int* __restrict__ obs_cam,
                                              const int* __restrict__ obs_feat, const int* __restrict__ cam_fo, const int* __restrict__ rank, int bf,
                                              unsigned long long* __restrict__ key, int* __restrict__ err) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n_obs) return;
  const int p = obs_point[i], c = obs_cam[i], f = obs_feat[i];
  bool ok = p >= 0 && p < n_points && c >= 0 && c < n_cams && f >= 0;
  if (ok) ok = f < cam_fo[c + 1] - cam_fo[c];
  if (!ok) { atomicMin(err, i); key[i] = (unsigned long long)(unsigned)n_points << 32; return; }
  key[i] = ((unsigned long long)(unsigned)p << 32) | ((unsigned long long)(unsigned)rank[c] << bf) | (unsigned)f;
}

// first[i] = 1 where sorted row i opens a distinct key; views[p] counts them (p = n_points: the reported rows)
__global__ __launch_bounds__(256) void k_first(int n_obs, const unsigned long long* __restrict__ key_s, uint8_t* __restrict__ first,
                                                int* __restrict__ views) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n_obs) return;
  const unsigned long long k = key_s[i];
  const bool head = i == 0 || key_s[i - 1] != k;
  first[i] = head ? 1 : 0;
  if (head) atomicAdd(&views[(int)(k >> 32)], 1);
}

// seg[p] = the first sorted row whose point is >= p, for p = 0 .. n_points + 1: seg[p] .. seg[p + 1] are the rows of point p
__global__ __launch_bounds__(256) void k_segments(int n_obs, int n_points, const unsigned long long* __restrict__ key_s, int* __restrict__ seg) {
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p > n_points + 1) return;
  int lo = 0, hi = n_obs;   // (key_s[i] >> 32) < p for i < lo, >= p for i >= hi
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if ((unsigned)(key_s[mid] >> 32) < (unsigned)p) lo = mid + 1; else hi = mid;
  }
  seg[p] = lo;
}

// ImmutableCamsPoints / MutableCamsPoints / PartialBundleAdjustment walk Camera::pts_: att[p] = some camera holds p,
// freed[p] = a free camera holds p and p is not bad (:926-931).  Idempotent byte stores: no atomics.
__global__ __launch_bounds__(256) void k_attach(int FP, int n_cams, int n_points, const int* __restrict__ cam_fo, const int* __restrict__ fp,
                                                 const uint8_t* __restrict__ cam_free, const uint8_t* __restrict__ pt_bad, uint8_t* __restrict__ att,
                                                 uint8_t* __restrict__ freed) {
  const int x = blockIdx.x * 256 + threadIdx.x;
  if (x >= FP) return;
  const int p = fp[x];
  if (p < 0 || p >= n_points) return;
  att[p] = 1;
  if (cam_free && !pt_bad[p] && cam_free[csr_segment_of(cam_fo, n_cams, x)]) freed[p] = 1;
}

// full = 0: frozen where attached, then freed (:919-945); full = 1: free where attached (:1880-1893); a point no camera holds
// keeps its incoming flag.  count[0] += the free points ("adjust pts", :955-963).
__global__ __launch_bounds__(256) void k_pt_mutable(int n_points, int full, const uint8_t* __restrict__ att, const uint8_t* __restrict__ freed,
                                                     const uint8_t* __restrict__ in, uint8_t* __restrict__ out, int* __restrict__ count) {
  const int p = blockIdx.x * 256 + threadIdx.x;
  int m = 0;
  if (p < n_points) {
    m = att[p] ? (full ? 1 : (freed[p] ? 1 : 0)) : (in[p] ? 1 : 0);
    out[p] = (uint8_t)m;
  }
  const int s = wave_sum_int(m);
  if ((threadIdx.x & 63) == 0 && s) atomicAdd(count, s);
}

// optimizer.cc:64, :86-125: the rows of a point that is not bad whose camera or point is free; a point with such a row
__global__ __launch_bounds__(256) void k_keep(int n_obs, int n_points, const unsigned long long* __restrict__ key_s, const uint8_t* __restrict__ first,
                                               const int* __restrict__ cam_of_rank, int bf, const uint8_t* __restrict__ cam_mut,
                                               const uint8_t* __restrict__ pt_mut, const uint8_t* __restrict__ pt_bad, int* __restrict__ keep_row,
                                               int* __restrict__ keep_pt) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i > n_obs) return;
  int k = 0;
  if (i < n_obs && first[i]) {
    const unsigned long long key = key_s[i];
    const int p = (int)(key >> 32);
    if (p < n_points && !pt_bad[p]) {
      const int c = cam_of_rank[((unsigned)key) >> bf];
      if (cam_mut[c] || pt_mut[p]) { k = 1; keep_pt[p] = 1; }
    }
  }
  keep_row[i] = k;
}

// thread i: sorted row i of the problem, and point i of the problem
__global__ __launch_bounds__(256) void k_emit(int n_obs, int n_points, const unsigned long long* __restrict__ key_s, const int* __restrict__ keep_row,
                                               const int* __restrict__ new_row, const int* __restrict__ keep_pt, const int* __restrict__ new_pt,
                                               const int* __restrict__ cam_of_rank, int bf, const int* __restrict__ kp_base, const float* __restrict__ kp,
                                               const int* __restrict__ views, double weight_ge3, const double* __restrict__ point_xyz,
                                               const uint8_t* __restrict__ pt_mut, int* __restrict__ obs_cam, int* __restrict__ obs_pt,
                                               double* __restrict__ obs_xy, double* __restrict__ pt_weight, double* __restrict__ point,
                                               uint8_t* __restrict__ out_mut, int* __restrict__ kept) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n_obs && keep_row[i]) {
    const unsigned long long key = key_s[i];
    const unsigned lo = (unsigned)key;
    const int c = cam_of_rank[lo >> bf], f = (int)(lo & ((1u << bf) - 1u));
    const size_t o = (size_t)new_row[i], r = (size_t)kp_base[c] + f;
    obs_cam[o] = c;
    obs_pt[o] = new_pt[(int)(key >> 32)];
    obs_xy[2 * o] = (double)kp[2 * r]; obs_xy[2 * o + 1] = (double)kp[2 * r + 1];   // :592-600, :810-821: float -> double
  }
  if (i < n_points && keep_pt[i]) {
    const size_t q = (size_t)new_pt[i];
    pt_weight[q] = views[i] >= 3 ? weight_ge3 : 1.0;   // optimizer.cc:69-78
    point[3 * q] = point_xyz[3 * (size_t)i]; point[3 * q + 1] = point_xyz[3 * (size_t)i + 1]; point[3 * q + 2] = point_xyz[3 * (size_t)i + 2];
    out_mut[q] = pt_mut[i];
    kept[q] = i;
  }
}

// BundleAdjuster::UpdateParameters for the points: problem point q is state point kept[q]
__global__ __launch_bounds__(256) void k_scatter_points(int n, const int* __restrict__ kept, const double* __restrict__ point, double* __restrict__ point_xyz) {
  const int q = blockIdx.x * 256 + threadIdx.x;
  if (q >= n) return;
  const size_t p = (size_t)kept[q];
  point_xyz[3 * p] = point[3 * (size_t)q]; point_xyz[3 * p + 1] = point[3 * (size_t)q + 1]; point_xyz[3 * p + 2] = point[3 * (size_t)q + 2];
}

// RemovePointOutliers (:1831-1863) with Point3D::Reprojection (structure.cc:267-300), one thread per point.  The sum over a
// point's rows is sequential by definition and a track is a handful of rows.  count: outliers, new added, new added outliers.
__global__ __launch_bounds__(256) void k_outliers(int n_points, const int* __restrict__ seg, const unsigned long long* __restrict__ key_s,
                                                   const uint8_t* __restrict__ first, const int* __restrict__ cam_of_rank, int bf,
                                                   const int* __restrict__ kp_base, const float* __restrict__ kp, const double* __restrict__ cam,
                                                   const double* __restrict__ point_xyz, double th, uint8_t* __restrict__ pt_bad,
                                                   double* __restrict__ pt_mse, uint8_t* __restrict__ pt_new_added, int* __restrict__ count) {
  const int p = blockIdx.x * 256 + threadIdx.x;
  int n_out = 0, n_new = 0, n_out_new = 0;
  if (p < n_points && !pt_bad[p]) {
    const double X[3] = {point_xyz[3 * (size_t)p], point_xyz[3 * (size_t)p + 1], point_xyz[3 * (size_t)p + 2]};
    const double m = p3d_ordered_mse(seg[p], seg[p + 1], [&](int i) {
      const unsigned lo = (unsigned)key_s[i];
      const int c = cam_of_rank[lo >> bf], f = (int)(lo & ((1u << bf) - 1u));
      const double* R = cam + ADJ_CAM * (size_t)c;
      const size_t r = (size_t)kp_base[c] + f;
      return p3d_row_error(R, R + 9, R + 12, X, (double)kp[2 * r], (double)kp[2 * r + 1]);
    }, [&](int i) { return first[i] != 0; });   // (std::map::insert kept one row per key)
    const int added = pt_new_added[p] ? 1 : 0;
    n_new = added;
    pt_mse[p] = m;
    if (sqrt(m) > th) { pt_bad[p] = 1; n_out = 1; n_out_new = added; }
    pt_new_added[p] = 0;
  }
  n_out = wave_sum_int(n_out); n_new = wave_sum_int(n_new); n_out_new = wave_sum_int(n_out_new);
  if ((threadIdx.x & 63) == 0) {
    if (n_out) atomicAdd(&count[0], n_out);
    if (n_new) atomicAdd(&count[1], n_new);
    if (n_out_new) atomicAdd(&count[2], n_out_new);
  }
}

// Camera::UpdatePoseFromData (camera.cc:113-137): rotation::AngleAxisToRotationMatrix with the C library's sin / cos, then
// c = -(R^T t), the products summed in row order
static void pose_to_camera(const double* pose, double* R, double* t, double* c) {
  const double a0 = pose[0], a1 = pose[1], a2 = pose[2];
  const double theta2 = a0 * a0 + a1 * a1 + a2 * a2;
  if (theta2 > std::numeric_limits<double>::epsilon()) {
    const double theta = std::sqrt(theta2);
    const double wx = a0 / theta, wy = a1 / theta, wz = a2 / theta;
    const double co = std::cos(theta), si = std::sin(theta);
    R[0] = co + wx * wx * (1 - co);       R[3] = wz * si + wx * wy * (1 - co);  R[6] = -wy * si + wx * wz * (1 - co);
    R[1] = wx * wy * (1 - co) - wz * si;  R[4] = co + wy * wy * (1 - co);       R[7] = wx * si + wy * wz * (1 - co);
    R[2] = wy * si + wx * wz * (1 - co);  R[5] = -wx * si + wy * wz * (1 - co); R[8] = co + wz * wz * (1 - co);
  } else {
    R[0] = 1; R[3] = a2; R[6] = -a1;
    R[1] = -a2; R[4] = 1; R[7] = a0;
    R[2] = a1; R[5] = -a0; R[8] = 1;
  }
  t[0] = pose[3]; t[1] = pose[4]; t[2] = pose[5];
  for (int k = 0; k < 3; k++) c[k] = -((R[k] * t[0] + R[3 + k] * t[1]) + R[6 + k] * t[2]);
}

}  // namespace adj

#define AJ_TRY(e) HIP_TRY(ctx, (e))

MSFM_API void msfm_round_default_options(msfm_round_options* o) {
  if (!o) return;
  msfm_ba_options_default(&o->partial);
  msfm_ba_options_default(&o->full);
  o->partial.max_num_iterations = 100;   // basic_structs.h:181-182
  o->full.max_num_iterations = 100;
  o->weight_partial = 2.0;               // sfm_incremental.cc:1012
  o->weight_full = 1.0;                  // :1024
  o->th_mse_outliers = 1.0;              // basic_structs.h:188
  o->keep_problem = 0;
}

// The checks that need no bulk array, and O(cameras) on the host: feat_point rows, image ranks, keypoint rows
int round_tables(msfm_ctx* ctx, const char* who, const msfm_match_store* S, const RoundArgs& A, bool packed_kp, const msfm_round_options& opt,
                 RoundTables* T) {
  const int ni = S->n_images, nc = A.n_cams, nm = A.n_models;
  if (!(opt.th_mse_outliers >= 0.0)) return msfm_set_error(ctx, MSFM_E_INVAL, "%s: th_mse_outliers = %g is NaN or negative", who, opt.th_mse_outliers);
  if (!(opt.weight_partial >= 0.0) || !(opt.weight_full >= 0.0))
    return msfm_set_error(ctx, MSFM_E_INVAL, "%s: a weight is NaN or negative", who);
  if (A.do_partial && A.new_cam < 0) return msfm_set_error(ctx, MSFM_E_INVAL, "%s: do_partial without new_cam", who);
  if (A.new_cam >= nc || A.new_cam < -1) return msfm_set_error(ctx, MSFM_E_INVAL, "%s: new_cam = %d outside n_cams = %d", who, A.new_cam, nc);
  for (int q = 0; q < A.n_visible; q++)
    if (A.visible[q] < 0 || A.visible[q] >= nc)
      return msfm_set_error(ctx, MSFM_E_INVAL, "%s: visible[%d] = %d outside n_cams = %d", who, q, A.visible[q], nc);
  for (int c = 0; c < nc; c++)
    if (A.cam_model_of_cam[c] < 0 || A.cam_model_of_cam[c] >= nm)
      return msfm_set_error(ctx, MSFM_E_INVAL, "%s: cam_model_of_cam[%d] = %d outside n_models = %d", who, c, A.cam_model_of_cam[c], nm);
  T->cam_fo.assign(nc + 1, 0); T->rank.assign(std::max(1, nc), 0); T->cam_of_rank.assign(std::max(1, nc), 0); T->kp_base.assign(std::max(1, nc), 0);
  T->max_feat = 1;
  T->kp_rows = 0;
  T->all_kp = true;
  {
    std::vector<uint8_t> seen(std::max(1, ni), 0);
    for (int c = 0; c < nc; c++) {
      const int im = A.cam_img[c];
      if (im < 0 || im >= ni) return msfm_set_error(ctx, MSFM_E_INVAL, "%s: cam_img[%d] = %d is no image of the store", who, c, im);
      if (seen[im]) return msfm_set_error(ctx, MSFM_E_INVAL, "%s: image %d has two cameras", who, im);
      seen[im] = 1;
      if ((long)T->cam_fo[c] + S->n_features[im] > 0x7fffffffL) return msfm_set_error(ctx, MSFM_E_INVAL, "%s: more than 2^31 registered features", who);
      T->cam_fo[c + 1] = T->cam_fo[c] + S->n_features[im];
      T->max_feat = std::max(T->max_feat, S->n_features[im]);
      if (packed_kp) { T->kp_base[c] = (int)T->kp_rows; T->kp_rows += S->n_features[im]; }
      else { T->kp_base[c] = S->feat_off[im]; T->all_kp = T->all_kp && S->has_kp[im]; }
    }
    std::iota(T->cam_of_rank.begin(), T->cam_of_rank.begin() + nc, 0);
    std::sort(T->cam_of_rank.begin(), T->cam_of_rank.begin() + nc, [&](int a, int b) { return A.cam_img[a] < A.cam_img[b]; });
    for (int r = 0; r < nc; r++) T->rank[T->cam_of_rank[r]] = r;
  }
  T->bf = bits_for((unsigned)(T->max_feat - 1));
  // the free cameras of the partial stage (:922-945): the new camera's model, and its visible cameras
  T->cam_free.assign(std::max(1, nc), 0); T->cam_all.assign(std::max(1, nc), 1);
  if (A.do_partial) {
    const int m = A.cam_model_of_cam[A.new_cam];
    for (int c = 0; c < nc; c++) T->cam_free[c] = A.cam_model_of_cam[c] == m ? 1 : 0;
    for (int q = 0; q < A.n_visible; q++) T->cam_free[A.visible[q]] = 1;
  }
  return MSFM_OK;
}

int round_fp_error(msfm_ctx* ctx, const char* who, const std::vector<int>& cam_fo, int n_cams, int n_points, int x) {
  int c = 0;
  while (c + 1 < n_cams && cam_fo[c + 1] <= x) c++;
  return msfm_set_error(ctx, MSFM_E_INVAL, "%s: feat_point of camera %d, feature %d is no point (n_points = %d)", who, c, x - cam_fo[c], n_points);
}

int round_row_error(msfm_ctx* ctx, const char* who, int row, int point, int cam, int feat) {
  return msfm_set_error(ctx, MSFM_E_INVAL, "%s: observation %d = (point %d, camera %d, feature %d) names an index outside its array", who, row, point, cam,
                        feat);
}

int round_key_check(msfm_ctx* ctx, const char* who, int n_cams, const RoundTables& T) {
  const int br = bits_for((unsigned)std::max(0, n_cams - 1));
  if (T.bf + br > 32)
    return msfm_set_error(ctx, MSFM_E_INVAL, "%s: %d cameras and %d features in an image need %d + %d bits: the sort key holds image rank and feature in 32", who,
                          n_cams, T.max_feat, br, T.bf);
  return MSFM_OK;
}

// The call behind its bulk uploads: the camera tables go up, every kernel and both solves run on the arrays of D, which are
// written in place.  R arrives with cam_pose / cam_model set and leaves with everything but h2d_bytes; with fetch_points the
// one read-back at the end carries the point arrays into it, without it the last solve's pt_mutable goes into D.pt_mutable.
int round_adjust_dev(msfm_ctx* ctx, const char* who, const RoundArgs& A, const RoundTables& T, const RoundDev& D, const msfm_round_options& opt,
                     int64_t* h2d_bytes, msfm_round_set* R, bool fetch_points) {
  using namespace adj;
  const int nc = A.n_cams, nm = A.n_models, np = A.n_points, no = A.n_obs, FP = T.cam_fo[nc], bf = T.bf;
  const bool solve = A.do_partial || A.do_full;
  const std::vector<int>& cam_fo = T.cam_fo;
  hipStream_t s = ctx->stream;
  const size_t npx = (size_t)np, nox = (size_t)no;
  DevBuf<int> d_fo, d_rank, d_cor, d_kpb, d_err, d_cnt, d_views, d_seg, keep_row, keep_pt, new_row, new_pt;
  DevBuf<double> d_cam;
  DevBuf<uint8_t> d_free, d_call, d_first, d_att, d_freed, d_mut;
  DevBuf<unsigned long long> d_key, d_key_s;
  PrimTmp tmp;
  DevScope sc(ctx);
  AJ_TRY(sc.up(d_fo, cam_fo.data(), (size_t)nc + 1));
  AJ_TRY(sc.up(d_rank, T.rank.data(), (size_t)nc)); AJ_TRY(sc.up(d_cor, T.cam_of_rank.data(), (size_t)nc)); AJ_TRY(sc.up(d_kpb, T.kp_base.data(), (size_t)nc));
  AJ_TRY(sc.up(d_free, T.cam_free.data(), (size_t)nc)); AJ_TRY(sc.up(d_call, T.cam_all.data(), (size_t)nc));
  const float* d_kp = D.kp;
  // err: feat_point entry, obs row; cnt: free points of the partial / the full stage, the three counts of the outlier stage
  AJ_TRY(d_err.alloc(2)); AJ_TRY(d_cnt.alloc(8));
  AJ_TRY(hipMemsetD32Async((hipDeviceptr_t)d_err.p, ADJ_BIG, 2, s));
  AJ_TRY(hipMemsetAsync(d_cnt.p, 0, sizeof(int) * 8, s));
  // ---- the point side in std::map order ----
  AJ_TRY(d_key.alloc(std::max<size_t>(1, nox))); AJ_TRY(d_key_s.alloc(std::max<size_t>(1, nox))); AJ_TRY(d_first.alloc(std::max<size_t>(1, nox)));
  AJ_TRY(d_views.alloc(npx + 1)); AJ_TRY(d_seg.alloc(npx + 2));
  AJ_TRY(d_att.alloc(std::max<size_t>(1, npx))); AJ_TRY(d_freed.alloc(std::max<size_t>(1, npx))); AJ_TRY(d_mut.alloc(std::max<size_t>(1, npx)));
  AJ_TRY(hipMemsetAsync(d_views.p, 0, sizeof(int) * (npx + 1), s));
  AJ_TRY(hipMemsetAsync(d_seg.p, 0, sizeof(int) * (npx + 2), s));   // (n_obs = 0: every segment is empty)
  AJ_TRY(hipMemsetAsync(d_att.p, 0, std::max<size_t>(1, npx), s)); AJ_TRY(hipMemsetAsync(d_freed.p, 0, std::max<size_t>(1, npx), s));
  {
    KTimer tm(ctx, "round_keys");
    tm.count = (FP ? 1 : 0) + (no ? 1 : 0);
    if (FP) hipLaunchKernelGGL(k_check_points, dim3(cdiv(FP, 256)), dim3(256), 0, s, FP, np, D.feat_point, d_err.p);
    if (no) hipLaunchKernelGGL(k_key, dim3(cdiv(no, 256)), dim3(256), 0, s, no, np, nc, D.obs_point, D.obs_cam, D.obs_feat, d_fo.p, d_rank.p, bf, d_key.p,
                               d_err.p + 1);
  }
  AJ_TRY(hipGetLastError());
  if (no) {
    const unsigned end_bit = 32u + (unsigned)bits_for((unsigned)np);
    {
      KTimer tm(ctx, "round_sort");
      AJ_TRY(prim_sort_keys(tmp, d_key.p, d_key_s.p, nox, 0u, end_bit, s));
    }
    KTimer tm(ctx, "round_first");
    tm.count = 2;
    hipLaunchKernelGGL(k_first, dim3(cdiv(no, 256)), dim3(256), 0, s, no, d_key_s.p, d_first.p, d_views.p);
    hipLaunchKernelGGL(k_segments, dim3(cdiv(np + 2, 256)), dim3(256), 0, s, no, np, d_key_s.p, d_seg.p);
  }
  if (FP && np) {
    KTimer tm(ctx, "round_attach");
    hipLaunchKernelGGL(k_attach, dim3(cdiv(FP, 256)), dim3(256), 0, s, FP, nc, np, d_fo.p, D.feat_point, A.do_partial ? d_free.p : (const uint8_t*)nullptr,
                       D.pt_bad, d_att.p, d_freed.p);
  }
  AJ_TRY(hipGetLastError());
  int err[2] = {ADJ_BIG, ADJ_BIG};
  bool err_read = false;
  auto index_error = [&]() -> int {   // after a synchronisation that carried d_err
    err_read = true;
    if (err[0] != ADJ_BIG) return round_fp_error(ctx, who, cam_fo, nc, np, err[0]);
    if (err[1] != ADJ_BIG) {
      int row[3] = {0, 0, 0};
      if (A.h_obs_point) { row[0] = A.h_obs_point[err[1]]; row[1] = A.h_obs_cam[err[1]]; row[2] = A.h_obs_feat[err[1]]; }
      else {   // the rows live on the device only
        AJ_TRY(hipMemcpyAsync(&row[0], D.obs_point + err[1], sizeof(int), hipMemcpyDeviceToHost, s));
        AJ_TRY(hipMemcpyAsync(&row[1], D.obs_cam + err[1], sizeof(int), hipMemcpyDeviceToHost, s));
        AJ_TRY(hipMemcpyAsync(&row[2], D.obs_feat + err[1], sizeof(int), hipMemcpyDeviceToHost, s));
        AJ_TRY(hipStreamSynchronize(s));
      }
      return round_row_error(ctx, who, err[1], row[0], row[1], row[2]);
    }
    return MSFM_OK;
  };
  // ---- the two solves ----
  if (solve) {
    AJ_TRY(keep_row.alloc(nox + 1)); AJ_TRY(keep_pt.alloc(npx + 1)); AJ_TRY(new_row.alloc(nox + 1)); AJ_TRY(new_pt.alloc(npx + 1));
  }
  bool mut_done = false;
  for (int stage = 0; stage < 2; stage++) {
    if (!(stage == 0 ? A.do_partial : A.do_full)) continue;
    const std::vector<uint8_t>& cam_mut = stage == 0 ? T.cam_free : T.cam_all;
    const uint8_t* d_cam_mut = stage == 0 ? d_free.p : d_call.p;
    const msfm_ba_options& bo = stage == 0 ? opt.partial : opt.full;
    AJ_TRY(hipMemsetAsync(keep_pt.p, 0, sizeof(int) * (npx + 1), s));
    {
      KTimer tm(ctx, "round_keep");
      tm.count = (np ? 1 : 0) + 1;
      if (np) hipLaunchKernelGGL(k_pt_mutable, dim3(cdiv(np, 256)), dim3(256), 0, s, np, stage, d_att.p, d_freed.p, D.pt_mutable, d_mut.p, d_cnt.p + stage);
      hipLaunchKernelGGL(k_keep, dim3(cdiv(no + 1, 256)), dim3(256), 0, s, no, np, d_key_s.p, d_first.p, d_cor.p, bf, d_cam_mut, d_mut.p, D.pt_bad, keep_row.p,
                         keep_pt.p);
    }
    mut_done = true;
    AJ_TRY(prim_scan_excl(tmp, keep_row.p, new_row.p, nox + 1, s));
    AJ_TRY(prim_scan_excl(tmp, keep_pt.p, new_pt.p, npx + 1, s));
    int npk = 0, nok = 0, free_pts = 0;
    AJ_TRY(hipMemcpyAsync(&nok, new_row.p + no, sizeof(int), hipMemcpyDeviceToHost, s));
    AJ_TRY(hipMemcpyAsync(&npk, new_pt.p + np, sizeof(int), hipMemcpyDeviceToHost, s));
    AJ_TRY(hipMemcpyAsync(&free_pts, d_cnt.p + stage, sizeof(int), hipMemcpyDeviceToHost, s));
    if (!err_read) AJ_TRY(hipMemcpyAsync(err, d_err.p, sizeof err, hipMemcpyDeviceToHost, s));
    AJ_TRY(hipStreamSynchronize(s));
    if (!err_read) MSFM_TRY(index_error());
    R->adjust[stage][0] = (int)std::count(cam_mut.begin(), cam_mut.begin() + nc, (uint8_t)1);
    R->adjust[stage][1] = free_pts;
    msfm_round_set::Problem& Q = R->problem[stage];
    Q.n_points = npk; Q.n_obs = nok;
    if (R->keep_problem) Q.cam_mutable.assign(cam_mut.begin(), cam_mut.begin() + nc);
    if (nok == 0) continue;   // nothing to adjust: the stage is skipped, solved[stage] stays 0
    DevBuf<int> obs_cam, obs_pt, kept;
    DevBuf<double> obs_xy, point, ptw;
    DevBuf<uint8_t> pmut;
    DevScope stage_sc(ctx);   // the problem's blocks: the solve below reads them
    AJ_TRY(obs_cam.alloc(nok)); AJ_TRY(obs_pt.alloc(nok)); AJ_TRY(obs_xy.alloc(2 * (size_t)nok));
    AJ_TRY(point.alloc(3 * (size_t)npk)); AJ_TRY(ptw.alloc(npk)); AJ_TRY(pmut.alloc(npk)); AJ_TRY(kept.alloc(npk));
    {
      KTimer tm(ctx, "round_emit");
      hipLaunchKernelGGL(k_emit, dim3(cdiv(std::max(no, np), 256)), dim3(256), 0, s, no, np, d_key_s.p, keep_row.p, new_row.p, keep_pt.p, new_pt.p, d_cor.p, bf,
                         d_kpb.p, d_kp, d_views.p, stage == 0 ? opt.weight_partial : opt.weight_full, D.point_xyz, d_mut.p, obs_cam.p, obs_pt.p, obs_xy.p, ptw.p,
                         point.p, pmut.p, kept.p);
    }
    AJ_TRY(hipGetLastError());
    if (R->keep_problem) {
      Q.kept.resize(npk); Q.obs_cam.resize(nok); Q.obs_pt.resize(nok); Q.obs_xy.resize(2 * (size_t)nok); Q.pt_weight.resize(npk); Q.pt_mutable.resize(npk);
      AJ_TRY(hipMemcpyAsync(Q.kept.data(), kept.p, sizeof(int) * (size_t)npk, hipMemcpyDeviceToHost, s));
      AJ_TRY(hipMemcpyAsync(Q.obs_cam.data(), obs_cam.p, sizeof(int) * (size_t)nok, hipMemcpyDeviceToHost, s));
      AJ_TRY(hipMemcpyAsync(Q.obs_pt.data(), obs_pt.p, sizeof(int) * (size_t)nok, hipMemcpyDeviceToHost, s));
      AJ_TRY(hipMemcpyAsync(Q.obs_xy.data(), obs_xy.p, sizeof(double) * 2 * (size_t)nok, hipMemcpyDeviceToHost, s));
      AJ_TRY(hipMemcpyAsync(Q.pt_weight.data(), ptw.p, sizeof(double) * (size_t)npk, hipMemcpyDeviceToHost, s));
      AJ_TRY(hipMemcpyAsync(Q.pt_mutable.data(), pmut.p, (size_t)npk, hipMemcpyDeviceToHost, s));
      AJ_TRY(hipStreamSynchronize(s));
    }
    msfm_ba_problem B;
    memset(&B, 0, sizeof B);
    B.n_cams = nc; B.n_models = nm; B.n_points = npk; B.n_obs = nok;
    B.cam_pose = R->cam_pose.data(); B.cam_model = R->cam_model.data(); B.cam_model_of_cam = A.cam_model_of_cam;
    B.point = point.p; B.obs_cam = obs_cam.p; B.obs_pt = obs_pt.p; B.obs_xy = obs_xy.p; B.pt_weight = ptw.p;
    B.cam_mutable = cam_mut.data(); B.model_mutable = A.model_mutable; B.pt_mutable = pmut.p;
    msfm_ba* ba = nullptr;
    MSFM_TRY(ba_create_impl(ctx, &B, /*bulk_on_device=*/true, &ba));
    struct Guard { msfm_ba* p; ~Guard() { if (p) msfm_ba_destroy(p); } } guard{ba};
    R->rows[stage].assign((size_t)std::max(0, bo.max_num_iterations) + 2, msfm_ba_iteration());
    msfm_ba_summary& sum = R->summary[stage];
    sum.iterations = R->rows[stage].data();
    sum.iterations_capacity = (int)R->rows[stage].size();
    MSFM_TRY(msfm_ba_run(ba, &bo, &sum));
    // BundleAdjuster::UpdateParameters: the points on the device, cameras and models through the host copy the next stage starts from
    {
      KTimer tm(ctx, "round_scatter_points");
      hipLaunchKernelGGL(k_scatter_points, dim3(cdiv(npk, 256)), dim3(256), 0, s, npk, kept.p, ba_device_points(ba), D.point_xyz);
    }
    AJ_TRY(hipGetLastError());
    MSFM_TRY(msfm_ba_download_params(ba, R->cam_pose.data(), R->cam_model.data(), nullptr));   // (synchronises: the scatter has run)
    stage_sc.dismiss();
    R->solved[stage] = 1;
  }
  // ---- Camera::UpdatePoseFromData / UpdataModelFromData ----
  R->cam_R.resize(9 * (size_t)nc); R->cam_t.resize(3 * (size_t)nc); R->cam_c.resize(3 * (size_t)nc); R->cam_fk.resize(3 * (size_t)nc);
  std::vector<double> cam(ADJ_CAM * (size_t)std::max(1, nc));
  for (int c = 0; c < nc; c++) {
    const size_t cx = (size_t)c;
    pose_to_camera(R->cam_pose.data() + 6 * cx, R->cam_R.data() + 9 * cx, R->cam_t.data() + 3 * cx, R->cam_c.data() + 3 * cx);
    std::copy(R->cam_model.begin() + 3 * (size_t)A.cam_model_of_cam[c], R->cam_model.begin() + 3 * (size_t)A.cam_model_of_cam[c] + 3, R->cam_fk.begin() + 3 * cx);
    double* C = cam.data() + ADJ_CAM * cx;
    std::copy(R->cam_R.begin() + 9 * cx, R->cam_R.begin() + 9 * cx + 9, C);
    std::copy(R->cam_t.begin() + 3 * cx, R->cam_t.begin() + 3 * cx + 3, C + 9);
    std::copy(R->cam_fk.begin() + 3 * cx, R->cam_fk.begin() + 3 * cx + 3, C + 12);
  }
  if (A.do_outliers && np) {
    AJ_TRY(sc.up(d_cam, cam.data(), ADJ_CAM * (size_t)nc));
    KTimer tm(ctx, "round_outliers");
    hipLaunchKernelGGL(k_outliers, dim3(cdiv(np, 256)), dim3(256), 0, s, np, d_seg.p, d_key_s.p, d_first.p, d_cor.p, bf, d_kpb.p, d_kp, d_cam.p, D.point_xyz,
                       opt.th_mse_outliers, D.pt_bad, D.pt_mse, D.pt_new_added, d_cnt.p + 2);
  }
  AJ_TRY(hipGetLastError());
  // ---- one read-back ----
  if (fetch_points) {
    R->point_xyz.resize(3 * npx); R->pt_mse.resize(npx); R->pt_mutable.resize(npx); R->pt_bad.resize(npx); R->pt_new_added.resize(npx); R->pt_views.resize(npx);
    if (np) {
      AJ_TRY(hipMemcpyAsync(R->point_xyz.data(), D.point_xyz, sizeof(double) * 3 * npx, hipMemcpyDeviceToHost, s));
      AJ_TRY(hipMemcpyAsync(R->pt_mse.data(), D.pt_mse, sizeof(double) * npx, hipMemcpyDeviceToHost, s));
      AJ_TRY(hipMemcpyAsync(R->pt_mutable.data(), mut_done ? d_mut.p : D.pt_mutable, npx, hipMemcpyDeviceToHost, s));
      AJ_TRY(hipMemcpyAsync(R->pt_bad.data(), D.pt_bad, npx, hipMemcpyDeviceToHost, s));
      AJ_TRY(hipMemcpyAsync(R->pt_new_added.data(), D.pt_new_added, npx, hipMemcpyDeviceToHost, s));
      AJ_TRY(hipMemcpyAsync(R->pt_views.data(), d_views.p, sizeof(int) * npx, hipMemcpyDeviceToHost, s));
    }
  } else if (mut_done && np) {   // the resident caller keeps the flag where it keeps the rest
    AJ_TRY(hipMemcpyAsync(D.pt_mutable, d_mut.p, npx, hipMemcpyDeviceToDevice, s));
  }
  AJ_TRY(hipMemcpyAsync(R->counts, d_cnt.p + 2, sizeof(int) * 3, hipMemcpyDeviceToHost, s));
  if (!err_read) AJ_TRY(hipMemcpyAsync(err, d_err.p, sizeof err, hipMemcpyDeviceToHost, s));
  AJ_TRY(sc.finish());   // the scratch above is released on return
  if (!err_read) MSFM_TRY(index_error());
  *h2d_bytes += sc.h2d;
  return MSFM_OK;
}

MSFM_API int msfm_round_adjust(msfm_ctx* ctx, const msfm_match_store* S, const msfm_round_problem* P, const msfm_round_options* opt_in,
                               msfm_round_set** out) {
  const char* who = "msfm_round_adjust";
  if (!ctx) return MSFM_E_INVAL;
  if (!S || !P || !out) return msfm_set_error(ctx, MSFM_E_INVAL, "%s: null argument", who);
  *out = nullptr;
  if (S->ctx != ctx) return msfm_set_error(ctx, MSFM_E_INVAL, "%s: the store belongs to another context", who);
  msfm_round_options opt;
  if (opt_in) opt = *opt_in; else msfm_round_default_options(&opt);
  const int nc = P->n_cams, nm = P->n_models, np = P->n_points, no = P->n_obs;
  if (nc < 0 || nm < 0 || np < 0 || no < 0 || P->n_visible < 0) return msfm_set_error(ctx, MSFM_E_INVAL, "%s: negative count", who);
  if ((nc && (!P->cam_img || !P->cam_pose || !P->cam_model_of_cam)) || (nm && !P->cam_model) || (no && (!P->obs_point || !P->obs_cam || !P->obs_feat)) ||
      (np && (!P->point_xyz || !P->pt_bad || !P->pt_mse || !P->pt_mutable)) || (P->n_visible && !P->visible))
    return msfm_set_error(ctx, MSFM_E_INVAL, "%s: null array", who);
  RoundArgs A;
  A.n_cams = nc; A.n_models = nm; A.n_points = np; A.n_obs = no;
  A.cam_img = P->cam_img; A.cam_model_of_cam = P->cam_model_of_cam; A.model_mutable = P->model_mutable;
  A.h_obs_point = P->obs_point; A.h_obs_cam = P->obs_cam; A.h_obs_feat = P->obs_feat;
  A.new_cam = P->new_cam; A.n_visible = P->n_visible; A.visible = P->visible;
  A.do_partial = P->do_partial != 0; A.do_full = P->do_full != 0; A.do_outliers = P->do_outliers != 0;
  RoundTables T;
  MSFM_TRY(round_tables(ctx, who, S, A, P->keypoints != nullptr, opt, &T));
  if (!T.all_kp)   // a store without some image's keypoints: that image must have no observation (a walk over obs_cam)
    for (int i = 0; i < no; i++) {
      const int c = P->obs_cam[i];
      if (c >= 0 && c < nc && !S->has_kp[P->cam_img[c]])
        return msfm_set_error(ctx, MSFM_E_INVAL, "%s: no keypoints of image %d (argument or chain)", who, P->cam_img[c]);
    }
  const int FP = T.cam_fo[nc];
  if (FP && !P->feat_point) return msfm_set_error(ctx, MSFM_E_INVAL, "%s: null feat_point", who);
  MSFM_TRY(round_key_check(ctx, who, nc, T));
  Child<msfm_round_set> R = child_new<msfm_round_set>(ctx);
  R->n_cams = nc; R->n_models = nm; R->n_points = np;
  R->keep_problem = opt.keep_problem != 0;
  R->cam_pose.assign(P->cam_pose, P->cam_pose + 6 * (size_t)nc);
  R->cam_model.assign(P->cam_model, P->cam_model + 3 * (size_t)nm);
  memset(R->summary, 0, sizeof R->summary);
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  const size_t npx = (size_t)np, nox = (size_t)no;
  // ---- one batch of uploads: the bulk arrays here, the camera tables in the core ----
  DevBuf<int> d_fp, d_op, d_oc, d_of;
  DevBuf<double> d_xyz, d_mse;
  DevBuf<uint8_t> d_bad, d_mut_in, d_added;
  DevBuf<float> d_kp_up;
  DevScope sc(ctx);
  AJ_TRY(sc.up(d_fp, P->feat_point, (size_t)FP));
  AJ_TRY(sc.up(d_op, P->obs_point, nox)); AJ_TRY(sc.up(d_oc, P->obs_cam, nox)); AJ_TRY(sc.up(d_of, P->obs_feat, nox));
  AJ_TRY(sc.up(d_xyz, P->point_xyz, 3 * npx)); AJ_TRY(sc.up(d_mse, P->pt_mse, npx));
  AJ_TRY(sc.up(d_bad, P->pt_bad, npx)); AJ_TRY(sc.up(d_mut_in, P->pt_mutable, npx));
  if (P->pt_new_added) AJ_TRY(sc.up(d_added, P->pt_new_added, npx));
  else { AJ_TRY(d_added.alloc(std::max<size_t>(1, npx))); AJ_TRY(hipMemsetAsync(d_added.p, 0, std::max<size_t>(1, npx), s)); }
  std::vector<float> h_kp;   // (lives to the final wait)
  if (P->keypoints) {   // the rows of the cameras' images only, packed in camera order
    h_kp.resize(2 * (size_t)T.kp_rows);
    for (int c = 0; c < nc; c++) {
      const int im = P->cam_img[c];
      std::copy(P->keypoints + 2 * (size_t)S->feat_off[im], P->keypoints + 2 * ((size_t)S->feat_off[im] + S->n_features[im]), h_kp.begin() + 2 * (size_t)T.kp_base[c]);
    }
    AJ_TRY(sc.up(d_kp_up, h_kp.data(), h_kp.size()));
  }
  RoundDev D;
  D.feat_point = d_fp.p; D.obs_point = d_op.p; D.obs_cam = d_oc.p; D.obs_feat = d_of.p;
  D.point_xyz = d_xyz.p; D.pt_mse = d_mse.p; D.pt_bad = d_bad.p; D.pt_mutable = d_mut_in.p; D.pt_new_added = d_added.p;
  D.kp = P->keypoints ? d_kp_up.p : S->d_kp.p;
  MSFM_TRY(round_adjust_dev(ctx, who, A, T, D, opt, &sc.h2d, R.get(), /*fetch_points=*/true));
  sc.dismiss();   // (the core's finish())
  R->h2d_bytes = sc.h2d;
  *out = R.release();
  return MSFM_OK;
}

MSFM_API int msfm_round_set_size(const msfm_round_set* R, int* n_cams, int* n_models, int* n_points, int64_t* h2d_bytes) {
  if (!R) return MSFM_E_INVAL;
  if (n_cams) *n_cams = R->n_cams;
  if (n_models) *n_models = R->n_models;
  if (n_points) *n_points = R->n_points;
  if (h2d_bytes) *h2d_bytes = R->h2d_bytes;
  return MSFM_OK;
}

MSFM_API int msfm_round_set_fetch(const msfm_round_set* R, double* cam_pose, double* cam_model, double* cam_R, double* cam_t, double* cam_c,
                                  double* cam_fk, double* point_xyz, uint8_t* pt_mutable, uint8_t* pt_bad, double* pt_mse, uint8_t* pt_new_added,
                                  int32_t* pt_views, int32_t* counts, int32_t* adjust, int32_t* solved, msfm_ba_summary* summary) {
  if (!R) return MSFM_E_INVAL;
  if (cam_pose) std::copy(R->cam_pose.begin(), R->cam_pose.end(), cam_pose);
  if (cam_model) std::copy(R->cam_model.begin(), R->cam_model.end(), cam_model);
  if (cam_R) std::copy(R->cam_R.begin(), R->cam_R.end(), cam_R);
  if (cam_t) std::copy(R->cam_t.begin(), R->cam_t.end(), cam_t);
  if (cam_c) std::copy(R->cam_c.begin(), R->cam_c.end(), cam_c);
  if (cam_fk) std::copy(R->cam_fk.begin(), R->cam_fk.end(), cam_fk);
  if (point_xyz) std::copy(R->point_xyz.begin(), R->point_xyz.end(), point_xyz);
  if (pt_mutable) std::copy(R->pt_mutable.begin(), R->pt_mutable.end(), pt_mutable);
  if (pt_bad) std::copy(R->pt_bad.begin(), R->pt_bad.end(), pt_bad);
  if (pt_mse) std::copy(R->pt_mse.begin(), R->pt_mse.end(), pt_mse);
  if (pt_new_added) std::copy(R->pt_new_added.begin(), R->pt_new_added.end(), pt_new_added);
  if (pt_views) std::copy(R->pt_views.begin(), R->pt_views.end(), pt_views);
  if (counts) std::copy(R->counts, R->counts + 3, counts);
  if (adjust) std::copy(&R->adjust[0][0], &R->adjust[0][0] + 4, adjust);
  if (solved) std::copy(R->solved, R->solved + 2, solved);
  if (summary)
    for (int k = 0; k < 2; k++) {   // the caller's iteration buffer stays the caller's
      msfm_ba_iteration* rows = summary[k].iterations;
      const int cap = rows ? summary[k].iterations_capacity : 0;
      summary[k] = R->summary[k];
      summary[k].iterations = rows;
      summary[k].iterations_capacity = cap;
      if (R->solved[k] && cap > 0) {
        const int n = std::min({cap, R->summary[k].num_iterations + 1, (int)R->rows[k].size()});
        std::copy(R->rows[k].begin(), R->rows[k].begin() + std::max(0, n), rows);
      }
    }
  return MSFM_OK;
}

MSFM_API int msfm_round_set_fetch_problem(const msfm_round_set* R, int stage, int* n_points, int* n_obs, int32_t* kept, int32_t* obs_cam,
                                          int32_t* obs_pt, double* obs_xy, double* pt_weight, uint8_t* cam_mutable, uint8_t* pt_mutable) {
  if (!R) return MSFM_E_INVAL;
  if (stage < 0 || stage > 1) return msfm_set_error(R->ctx, MSFM_E_INVAL, "msfm_round_set_fetch_problem: stage = %d is neither 0 (partial) nor 1 (full)", stage);
  if (!R->keep_problem) return msfm_set_error(R->ctx, MSFM_E_INVAL, "msfm_round_set_fetch_problem: the set was made without keep_problem");
  const msfm_round_set::Problem& Q = R->problem[stage];
  if (n_points) *n_points = Q.n_points;
  if (n_obs) *n_obs = Q.n_obs;
  if (kept) std::copy(Q.kept.begin(), Q.kept.end(), kept);
  if (obs_cam) std::copy(Q.obs_cam.begin(), Q.obs_cam.end(), obs_cam);
  if (obs_pt) std::copy(Q.obs_pt.begin(), Q.obs_pt.end(), obs_pt);
  if (obs_xy) std::copy(Q.obs_xy.begin(), Q.obs_xy.end(), obs_xy);
  if (pt_weight) std::copy(Q.pt_weight.begin(), Q.pt_weight.end(), pt_weight);
  if (cam_mutable) std::copy(Q.cam_mutable.begin(), Q.cam_mutable.end(), cam_mutable);
  if (pt_mutable) std::copy(Q.pt_mutable.begin(), Q.pt_mutable.end(), pt_mutable);
  return MSFM_OK;
}

MSFM_API void msfm_round_set_destroy(msfm_round_set* R) { msfm_child_destroy(R); }
