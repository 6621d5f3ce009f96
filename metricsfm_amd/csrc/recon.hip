// The reconstruction state of a model, resident: the flat state of the round calls (feat_point = Camera::pts_, the obs_* rows =
// Point3D::cams_ / pts2d_, the point arrays and flags, the keypoints of a host-made store) uploaded once, at msfm_recon_create,
// read by msfm_recon_localize (the cores of the two localize calls; the winner's row stays pending on the device), given a
// camera by msfm_recon_commit_camera (k_commit_flags, a scan, k_commit),
// made from a seed set's winner by msfm_recon_create_from_seed (k_seed_state on the points the set keeps on the device), normalised
// by msfm_recon_normalize (k_normalize_sums: the ordered sums of BundleAdjuster::Normalize; k_normalize_write),
// extended by msfm_recon_new_points - the kernels of msfm_new_points (newpoints.hip: newpoints_dev) on the resident feat_point and
// keypoints, then k_append_points - and adjusted in place by msfm_recon_adjust - the core of msfm_round_adjust (adjust.hip:
// round_adjust_dev) on these buffers.
//
//   device      feat_point [sum of n_features of the store]   (an image has at most one camera: the capacity never grows)
//               obs_point / obs_cam / obs_feat [cap_obs], point_xyz, pt_bad, pt_mse, pt_views, pt_mutable, pt_new_added [cap_points]
//               keypoints [sum of n_features][2] of a host-made store; a store made from a chain has them already
//   host        O(cameras): cam_img, cam_pose, cam_model, cam_model_of_cam, model_mutable, cam_R / cam_t / cam_c / cam_fk
//
// Capacity and length are kept apart: the state only grows at its ends, so an append writes behind them, and arrays that are
// too short move into blocks of twice the need first (recon_reserve).
// Every index of the state is checked once, on the device, before the object exists (k_check_fp, k_check_rows): the calls on
// the object may then index by it.  The kernels here compare and copy; the unit keeps the no-contraction discipline of
// adjust.hip all the same.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <memory>

#include "prim_device.h"

#pragma clang fp contract(off)

struct msfm_recon {
  msfm_ctx* ctx = nullptr;
  const msfm_match_store* store = nullptr;
  int n_cams = 0, n_models = 0, n_points = 0, n_obs = 0;
  size_t cap_points = 0, cap_obs = 0;
  std::vector<int> cam_img, cam_model_of_cam;
  std::vector<uint8_t> model_mutable;   // empty: none given
  std::vector<double> cam_pose, cam_model, cam_R, cam_t, cam_c, cam_fk;
  DevBuf<int> d_fp, d_op, d_oc, d_of, d_views;
  DevBuf<double> d_xyz, d_mse;
  DevBuf<uint8_t> d_bad, d_mut, d_added;
  DevBuf<float> d_kp;                   // empty: the store's
  DevBuf<double> d_noise;               // the last msfm_recon_normalize's noise: its write kernel is not waited for
  bool own_kp = false;
  int64_t h2d_bytes = 0;
  bool poisoned = false;                // a solve failed behind a stage that had written: the state is mixed
  // the last msfm_recon_localize: its lists, and the winner's row as a pending localisation (device) until it is committed
  std::vector<int> ranked, failed, visible;
  msfm_recon_winner winner;
  bool pending = false;
  DevBuf<int> pend_feat, pend_point;
  DevBuf<uint8_t> pend_state;
};

namespace rec {

#define REC_BIG 0x7fffffff

__global__ __launch_bounds__(256) void k_check_fp(int FP, int n_points, const int* __restrict__ fp, int* __restrict__ err) {
  const int x = blockIdx.x * 256 + threadIdx.x;
  if (x < FP && fp[x] >= n_points) atomicMin(err, x);
}

// a row names a point, a camera and a feature of that camera's image (cam_fo: the feat_point row offsets)
__global__ __launch_bounds__(256) void k_check_rows(int n_obs, int n_points, int n_cams, const int* __restrict__ obs_point, const int* __restrict__ obs_cam,
                                                     const int* __restrict__ obs_feat, const int* __restrict__ cam_fo, int* __restrict__ err) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n_obs) return;
  const int p = obs_point[i], c = obs_cam[i], f = obs_feat[i];
  bool ok = p >= 0 && p < n_points && c >= 0 && c < n_cams && f >= 0;
  if (ok) ok = f < cam_fo[c + 1] - cam_fo[c];
  if (!ok) atomicMin(err, i);
}

// sfm_incremental.cc:899-910 for the n points k_emit of newpoints.hip left in sorted order (one new camera: they are the
// first n positions): point p becomes id n_points + p with two views, its mse, not bad, new, mutable; its two rows
// (id, c1, feat1), (id, cam2, feat2) go to 2p, 2p + 1 behind the existing rows; feat_point gets the inserts that took.
// No atomics: takes1 / takes2 name one writer per (camera, feature) slot (k_claim), everything else is indexed by p.
__global__ __launch_bounds__(256) void k_append_points(int n, int E, int c1, int n_points, int n_obs, const int* __restrict__ off_all,
                                                        const NewPointsEnt* __restrict__ ent, const int* __restrict__ cam_of_row, const int* __restrict__ w,
                                                        const int* __restrict__ feat1, const int* __restrict__ feat2, const double* __restrict__ X,
                                                        const double* __restrict__ mse, const uint8_t* __restrict__ takes1,
                                                        const uint8_t* __restrict__ takes2, int* __restrict__ fp, int* __restrict__ obs_point,
                                                        int* __restrict__ obs_cam, int* __restrict__ obs_feat, double* __restrict__ point_xyz,
                                                        double* __restrict__ pt_mse, int* __restrict__ pt_views, uint8_t* __restrict__ pt_bad,
                                                        uint8_t* __restrict__ pt_mutable, uint8_t* __restrict__ pt_new_added) {
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= n) return;
  const NewPointsEnt e = ent[csr_segment_of(off_all, E, w[p])];
  const int id = n_points + p, f1 = feat1[p], f2 = feat2[p];
  const size_t i = (size_t)id, r = (size_t)n_obs + 2 * (size_t)p;
  point_xyz[3 * i] = X[3 * (size_t)p]; point_xyz[3 * i + 1] = X[3 * (size_t)p + 1]; point_xyz[3 * i + 2] = X[3 * (size_t)p + 2];
  pt_mse[i] = mse[p];
  pt_views[i] = 2; pt_bad[i] = 0; pt_new_added[i] = 1; pt_mutable[i] = 1;
  obs_point[r] = id; obs_cam[r] = c1; obs_feat[r] = f1;
  obs_point[r + 1] = id; obs_cam[r + 1] = cam_of_row[e.cam2]; obs_feat[r + 1] = f2;
  if (takes1[p]) fp[(size_t)e.fp1 + f1] = id;
  if (takes2[p]) fp[(size_t)e.fp2 + f2] = id;
}

// LocalizeImage :705-748 for the pending row, in two launches around an exclusive scan of (state == 2).
// k_commit_flags: flag[i] = the correspondence is state 2 (n entries and a closing 0).
__global__ __launch_bounds__(256) void k_commit_flags(int n, const uint8_t* __restrict__ state, int* __restrict__ flag) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i <= n) flag[i] = i < n && state[i] == 2 ? 1 : 0;
}
// k_commit: state 1 marks its point bad (:715); state 2 puts the point into the new camera's feat_point row (:725), gives it a
// view and is_new_added_ (:723-724) and appends its row at n_obs + pos[i], in correspondence order.  No atomics: the features
// of a row are distinct, a point is state 2 at most once per row, and the state-1 store is idempotent.  A point that is state 1
// through one feature and state 2 through another keeps both effects.
__global__ __launch_bounds__(256) void k_commit(int n, int new_cam, int fp_off, int n_obs, const int* __restrict__ feat, const int* __restrict__ point,
                                                 const uint8_t* __restrict__ state, const int* __restrict__ pos, int* __restrict__ fp,
                                                 uint8_t* __restrict__ pt_bad, int* __restrict__ pt_views, uint8_t* __restrict__ pt_new_added,
                                                 int* __restrict__ obs_point, int* __restrict__ obs_cam, int* __restrict__ obs_feat) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int st = state[i], p = point[i], f = feat[i];
  if (st == 1) pt_bad[p] = 1;
  if (st == 2) {
    fp[(size_t)fp_off + f] = p;
    pt_views[p] += 1;
    pt_new_added[p] = 1;
    const size_t r = (size_t)n_obs + pos[i];
    obs_point[r] = p; obs_cam[r] = new_cam; obs_feat[r] = f;
  }
}

// sfm_incremental.cc:344-374 for the P accepted points of a seed set's winner, in the set's order: point p is the set's X / mse
// with two views, not bad, mutable, new (structure.cc:30-37); its rows (p, 0, feat1), (p, 1, feat2) go to 2p, 2p + 1, the
// features read from the store's matches through pt_match.  Camera::AddPoints is a std::map::insert - the first point of a
// feature keeps it: fp (nf1 + nf2 entries of -1 on entry) takes the unsigned minimum of the ids, which is the lowest id whatever
// the scheduling (-1 is the largest unsigned value).  The store's matches name features inside their images (checked when
// the store was made).
__global__ __launch_bounds__(256) void k_seed_state(int P, int m0, int nf1, const int* __restrict__ pt_match, const int* __restrict__ matches,
                                                     const double* __restrict__ X, const double* __restrict__ mse, int* __restrict__ fp,
                                                     int* __restrict__ obs_point, int* __restrict__ obs_cam, int* __restrict__ obs_feat,
                                                     double* __restrict__ point_xyz, double* __restrict__ pt_mse, int* __restrict__ pt_views,
                                                     uint8_t* __restrict__ pt_bad, uint8_t* __restrict__ pt_mutable, uint8_t* __restrict__ pt_new_added) {
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= P) return;
  const size_t i = (size_t)p, m = (size_t)m0 + pt_match[p];
  const int f1 = matches[2 * m], f2 = matches[2 * m + 1];
  point_xyz[3 * i] = X[3 * i]; point_xyz[3 * i + 1] = X[3 * i + 1]; point_xyz[3 * i + 2] = X[3 * i + 2];
  pt_mse[i] = mse[i];
  pt_views[i] = 2; pt_bad[i] = 0; pt_mutable[i] = 1; pt_new_added[i] = 1;
  obs_point[2 * i] = p; obs_cam[2 * i] = 0; obs_feat[2 * i] = f1;
  obs_point[2 * i + 1] = p; obs_cam[2 * i + 1] = 1; obs_feat[2 * i + 1] = f2;
  atomicMin((unsigned*)fp + f1, (unsigned)p);
  atomicMin((unsigned*)fp + (size_t)nf1 + f2, (unsigned)p);
}

// BundleAdjuster::Normalize's two sums (optimizer.cc:160-179), in the order of its loops: the definition is the left-to-right
// sum, so one wave does it.  Chunks of NORM_CHUNK points are staged through LDS by all 64 lanes (coalesced); lanes 0-2 carry
// the three chains of mid, then every lane forms the deviations d_i of its points and lane 0 carries the chain of mad.
// out [5]: mid (3), mad, scale = target / mad.
#define NORM_CHUNK 1024
__global__ __launch_bounds__(64) void k_normalize_sums(int n, const double* __restrict__ x, double target, double* __restrict__ out) {
  __shared__ double s_x[3 * NORM_CHUNK];
  __shared__ double s_mid[3];
  const int lane = threadIdx.x;
  double acc = 0.0;
  for (int c0 = 0; c0 < n; c0 += NORM_CHUNK) {
    const int cnt = min(NORM_CHUNK, n - c0);
    for (int k = lane; k < 3 * cnt; k += 64) s_x[k] = x[3 * (size_t)c0 + k];
    __syncthreads();
    if (lane < 3)
      for (int j = 0; j < cnt; j++) acc += s_x[3 * j + lane];
    __syncthreads();
  }
  if (lane < 3) s_mid[lane] = acc / n;
  __syncthreads();
  const double m0 = s_mid[0], m1 = s_mid[1], m2 = s_mid[2];
  double mad = 0.0;
  for (int c0 = 0; c0 < n; c0 += NORM_CHUNK) {
    const int cnt = min(NORM_CHUNK, n - c0);
    for (int j = lane; j < cnt; j += 64) {
      const double* q = x + 3 * ((size_t)c0 + j);
      s_x[j] = (fabs(q[0] - m0) + fabs(q[1] - m1)) + fabs(q[2] - m2);
    }
    __syncthreads();
    if (lane == 0)
      for (int j = 0; j < cnt; j++) mad += s_x[j];
    __syncthreads();
  }
  if (lane == 0) {
    mad = mad / n;
    out[0] = m0; out[1] = m1; out[2] = m2; out[3] = mad; out[4] = target / mad;
  }
}

// x = scale * (x - mid), then x = x + noise * sigma (optimizer.cc:183-188, :204-209); one thread per coordinate
__global__ __launch_bounds__(256) void k_normalize_write(long n3, double m0, double m1, double m2, double scale, const double* __restrict__ noise,
                                                          double sigma, double* __restrict__ x) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n3) return;
  const int k = (int)(i % 3);
  const double mid = k == 0 ? m0 : (k == 1 ? m1 : m2);
  double v = scale * (x[i] - mid);
  if (noise) v = v + noise[i] * sigma;
  x[i] = v;
}

static RoundArgs args_of(const msfm_recon* Q) {
  RoundArgs A;
  A.n_cams = Q->n_cams; A.n_models = Q->n_models; A.n_points = Q->n_points; A.n_obs = Q->n_obs;
  A.cam_img = Q->cam_img.data(); A.cam_model_of_cam = Q->cam_model_of_cam.data();
  A.model_mutable = Q->model_mutable.empty() ? nullptr : Q->model_mutable.data();
  return A;
}

// the refusal of every call but fetch and destroy once a solve has failed behind a stage that had written
static int poisoned_error(msfm_ctx* ctx, const char* who) {
  return msfm_set_error(ctx, MSFM_E_INVAL, "%s: an earlier msfm_recon_adjust failed inside a solve: the object can only be fetched or destroyed", who);
}

}  // namespace rec

#define RC_TRY(e) HIP_TRY(ctx, (e))

MSFM_API int msfm_recon_create(msfm_ctx* ctx, const msfm_match_store* S, const msfm_recon_init* P, msfm_recon** out) {
  using namespace rec;
  const char* who = "msfm_recon_create";
  if (!ctx) return MSFM_E_INVAL;
  if (!S || !P || !out) return msfm_set_error(ctx, MSFM_E_INVAL, "%s: null argument", who);
  *out = nullptr;
  if (S->ctx != ctx) return msfm_set_error(ctx, MSFM_E_INVAL, "%s: the store belongs to another context", who);
  const int nc = P->n_cams, nm = P->n_models, np = P->n_points, no = P->n_obs;
  if (nc < 0 || nm < 0 || np < 0 || no < 0 || P->reserve_points < 0 || P->reserve_obs < 0) return msfm_set_error(ctx, MSFM_E_INVAL, "%s: negative count", who);
  if ((nc && (!P->cam_img || !P->cam_pose || !P->cam_model_of_cam || !P->cam_R || !P->cam_t || !P->cam_c || !P->cam_fk)) || (nm && !P->cam_model) ||
      (no && (!P->obs_point || !P->obs_cam || !P->obs_feat)) || (np && (!P->point_xyz || !P->pt_bad || !P->pt_mse || !P->pt_views || !P->pt_mutable)))
    return msfm_set_error(ctx, MSFM_E_INVAL, "%s: null array", who);
  RoundArgs A;
  A.n_cams = nc; A.n_models = nm; A.n_points = np; A.n_obs = no;
  A.cam_img = P->cam_img; A.cam_model_of_cam = P->cam_model_of_cam;
  msfm_round_options opt;
  msfm_round_default_options(&opt);
  RoundTables T;
  MSFM_TRY(round_tables(ctx, who, S, A, /*packed_kp=*/false, opt, &T));
  if (!P->keypoints && !T.all_kp)   // as msfm_round_adjust: an image without keypoints must have no observation
    for (int i = 0; i < no; i++) {
      const int c = P->obs_cam[i];
      if (c >= 0 && c < nc && !S->has_kp[P->cam_img[c]])
        return msfm_set_error(ctx, MSFM_E_INVAL, "%s: no keypoints of image %d (argument or chain)", who, P->cam_img[c]);
    }
  const int FP = T.cam_fo[nc];
  if (FP && !P->feat_point) return msfm_set_error(ctx, MSFM_E_INVAL, "%s: null feat_point", who);
  MSFM_TRY(round_key_check(ctx, who, nc, T));
  Child<msfm_recon> Q = child_new<msfm_recon>(ctx);
  Q->store = S;
  Q->n_cams = nc; Q->n_models = nm; Q->n_points = np; Q->n_obs = no;
  Q->cap_points = std::max<size_t>(1, std::max((size_t)np, (size_t)P->reserve_points));
  Q->cap_obs = std::max<size_t>(1, std::max((size_t)no, (size_t)P->reserve_obs));
  const size_t ncx = (size_t)nc, npx = (size_t)np, nox = (size_t)no, total = (size_t)S->feat_off[S->n_images];
  Q->cam_img.assign(P->cam_img, P->cam_img + ncx);
  Q->cam_model_of_cam.assign(P->cam_model_of_cam, P->cam_model_of_cam + ncx);
  if (P->model_mutable) Q->model_mutable.assign(P->model_mutable, P->model_mutable + (size_t)nm);
  Q->cam_pose.assign(P->cam_pose, P->cam_pose + 6 * ncx); Q->cam_model.assign(P->cam_model, P->cam_model + 3 * (size_t)nm);
  Q->cam_R.assign(P->cam_R, P->cam_R + 9 * ncx); Q->cam_t.assign(P->cam_t, P->cam_t + 3 * ncx);
  Q->cam_c.assign(P->cam_c, P->cam_c + 3 * ncx); Q->cam_fk.assign(P->cam_fk, P->cam_fk + 3 * ncx);
  RC_TRY(hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  DevBuf<int> d_fo, d_err;
  DevScope sc(ctx);
  RC_TRY(sc.up(Q->d_fp, P->feat_point, (size_t)FP, total));
  RC_TRY(sc.up(Q->d_op, P->obs_point, nox, Q->cap_obs)); RC_TRY(sc.up(Q->d_oc, P->obs_cam, nox, Q->cap_obs)); RC_TRY(sc.up(Q->d_of, P->obs_feat, nox, Q->cap_obs));
  RC_TRY(sc.up(Q->d_xyz, P->point_xyz, 3 * npx, 3 * Q->cap_points)); RC_TRY(sc.up(Q->d_mse, P->pt_mse, npx, Q->cap_points));
  RC_TRY(sc.up(Q->d_views, P->pt_views, npx, Q->cap_points));
  RC_TRY(sc.up(Q->d_bad, P->pt_bad, npx, Q->cap_points)); RC_TRY(sc.up(Q->d_mut, P->pt_mutable, npx, Q->cap_points));
  if (P->pt_new_added) RC_TRY(sc.up(Q->d_added, P->pt_new_added, npx, Q->cap_points));
  else { RC_TRY(Q->d_added.alloc(Q->cap_points)); RC_TRY(hipMemsetAsync(Q->d_added.p, 0, Q->cap_points, s)); }
  if (P->keypoints) {   // every image's rows, in the store's order: camera c reads from feat_off[cam_img[c]], now and after any append
    RC_TRY(sc.up(Q->d_kp, P->keypoints, 2 * total, 2 * total));
    Q->own_kp = true;
  }
  RC_TRY(sc.up(d_fo, T.cam_fo.data(), ncx + 1, ncx + 1));
  RC_TRY(d_err.alloc(2));
  RC_TRY(hipMemsetD32Async((hipDeviceptr_t)d_err.p, REC_BIG, 2, s));
  {
    KTimer tm(ctx, "recon_check");
    tm.count = (FP ? 1 : 0) + (no ? 1 : 0);
    if (FP) hipLaunchKernelGGL(k_check_fp, dim3(cdiv(FP, 256)), dim3(256), 0, s, FP, np, Q->d_fp.p, d_err.p);
    if (no) hipLaunchKernelGGL(k_check_rows, dim3(cdiv(no, 256)), dim3(256), 0, s, no, np, nc, Q->d_op.p, Q->d_oc.p, Q->d_of.p, d_fo.p, d_err.p + 1);
  }
  RC_TRY(hipGetLastError());
  int err[2] = {REC_BIG, REC_BIG};
  RC_TRY(hipMemcpyAsync(err, d_err.p, sizeof err, hipMemcpyDeviceToHost, s));
  RC_TRY(sc.finish());
  if (err[0] != REC_BIG) return round_fp_error(ctx, who, T.cam_fo, nc, np, err[0]);
  if (err[1] != REC_BIG) return round_row_error(ctx, who, err[1], P->obs_point[err[1]], P->obs_cam[err[1]], P->obs_feat[err[1]]);
  Q->h2d_bytes = sc.h2d;
  *out = Q.release();
  return MSFM_OK;
}

MSFM_API int msfm_recon_create_from_seed(msfm_ctx* ctx, const msfm_match_store* S, const msfm_seed_set* W, const double* cam_pose, int nm,
                                         const double* cam_model, const int32_t* cam_model_of_cam, const uint8_t* model_mutable,
                                         const float* keypoints, int reserve_points, int reserve_obs, msfm_recon** out) {
  using namespace rec;
  const char* who = "msfm_recon_create_from_seed";
  if (!ctx) return MSFM_E_INVAL;
  if (!S || !W || !out) return msfm_set_error(ctx, MSFM_E_INVAL, "%s: null argument", who);
  *out = nullptr;
  if (S->ctx != ctx) return msfm_set_error(ctx, MSFM_E_INVAL, "%s: the store belongs to another context", who);
  if (W->store != S || W->ctx != ctx) return msfm_set_error(ctx, MSFM_E_INVAL, "%s: the seed set was made on another store", who);
  if (W->winner < 0) return msfm_set_error(ctx, MSFM_E_INVAL, "%s: the seed set has no winner", who);
  if (nm != 1 && nm != 2) return msfm_set_error(ctx, MSFM_E_INVAL, "%s: n_models = %d outside {1, 2}", who, nm);
  if (!cam_pose || !cam_model || !cam_model_of_cam) return msfm_set_error(ctx, MSFM_E_INVAL, "%s: null array", who);
  if (reserve_points < 0 || reserve_obs < 0) return msfm_set_error(ctx, MSFM_E_INVAL, "%s: negative count", who);
  for (int c = 0; c < 2; c++) {
    if (cam_model_of_cam[c] < 0 || cam_model_of_cam[c] >= nm)
      return msfm_set_error(ctx, MSFM_E_INVAL, "%s: cam_model_of_cam[%d] = %d outside n_models = %d", who, c, cam_model_of_cam[c], nm);
    if (!keypoints && !S->has_kp[W->win_img[c]])
      return msfm_set_error(ctx, MSFM_E_INVAL, "%s: no keypoints of image %d (argument or chain)", who, W->win_img[c]);
  }
  const int w = W->winner, i1 = W->win_img[0], i2 = W->win_img[1];
  const int np = W->pt_off[w + 1] - W->pt_off[w], no = 2 * np;
  const int nf1 = S->n_features[i1], nf2 = S->n_features[i2];
  Child<msfm_recon> Q = child_new<msfm_recon>(ctx);
  Q->store = S;
  Q->n_cams = 2; Q->n_models = nm; Q->n_points = np; Q->n_obs = no;
  Q->cap_points = std::max<size_t>(1, std::max((size_t)np, (size_t)reserve_points));
  Q->cap_obs = std::max<size_t>(1, std::max((size_t)no, (size_t)reserve_obs));
  const size_t total = (size_t)S->feat_off[S->n_images];
  // the host tables: camera 0 is [I|0] (:290), camera 1 the set's pose; fk = (the set's f, the model's k1, k2)
  Q->cam_img = {i1, i2};
  Q->cam_model_of_cam.assign(cam_model_of_cam, cam_model_of_cam + 2);
  if (model_mutable) Q->model_mutable.assign(model_mutable, model_mutable + (size_t)nm);
  Q->cam_pose.assign(cam_pose, cam_pose + 12); Q->cam_model.assign(cam_model, cam_model + 3 * (size_t)nm);
  Q->cam_R = {1, 0, 0, 0, 1, 0, 0, 0, 1}; Q->cam_t.assign(3, 0.0); Q->cam_c.assign(3, 0.0);
  Q->cam_R.insert(Q->cam_R.end(), W->R.begin() + 9 * (size_t)w, W->R.begin() + 9 * (size_t)w + 9);
  Q->cam_t.insert(Q->cam_t.end(), W->t.begin() + 3 * (size_t)w, W->t.begin() + 3 * (size_t)w + 3);
  Q->cam_c.insert(Q->cam_c.end(), W->c.begin() + 3 * (size_t)w, W->c.begin() + 3 * (size_t)w + 3);
  for (int c = 0; c < 2; c++) {
    const double* M = cam_model + 3 * (size_t)cam_model_of_cam[c];
    Q->cam_fk.push_back(W->f[2 * (size_t)w + c]); Q->cam_fk.push_back(M[1]); Q->cam_fk.push_back(M[2]);
  }
  RC_TRY(hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  DevScope sc(ctx);
  RC_TRY(Q->d_fp.alloc(std::max<size_t>(1, total)));
  RC_TRY(Q->d_op.alloc(Q->cap_obs)); RC_TRY(Q->d_oc.alloc(Q->cap_obs)); RC_TRY(Q->d_of.alloc(Q->cap_obs));
  RC_TRY(Q->d_xyz.alloc(3 * Q->cap_points)); RC_TRY(Q->d_mse.alloc(Q->cap_points)); RC_TRY(Q->d_views.alloc(Q->cap_points));
  RC_TRY(Q->d_bad.alloc(Q->cap_points)); RC_TRY(Q->d_mut.alloc(Q->cap_points)); RC_TRY(Q->d_added.alloc(Q->cap_points));
  if (keypoints) {   // every image's rows, as msfm_recon_create keeps them
    RC_TRY(sc.up(Q->d_kp, keypoints, 2 * total, 2 * total));
    Q->own_kp = true;
  }
  if (nf1 + nf2) RC_TRY(hipMemsetD32Async((hipDeviceptr_t)Q->d_fp.p, -1, (size_t)nf1 + (size_t)nf2, s));   // Camera::pts_ of two new cameras
  if (np) {
    KTimer tm(ctx, "recon_from_seed");
    hipLaunchKernelGGL(k_seed_state, dim3(cdiv(np, 256)), dim3(256), 0, s, np, W->win_m0, nf1, W->d_ptm.p, S->d_match.p, W->d_X.p, W->d_mse.p, Q->d_fp.p,
                       Q->d_op.p, Q->d_oc.p, Q->d_of.p, Q->d_xyz.p, Q->d_mse.p, Q->d_views.p, Q->d_bad.p, Q->d_mut.p, Q->d_added.p);
  }
  RC_TRY(hipGetLastError());
  RC_TRY(sc.finish());   // the one wait: the set may be destroyed behind the call
  Q->h2d_bytes = sc.h2d;
  *out = Q.release();
  return MSFM_OK;
}

MSFM_API int msfm_recon_normalize(msfm_recon* Q, const double* noise, double target_deviation, double point_sigma, double mid[3], double* scale) {
  using namespace rec;
  const char* who = "msfm_recon_normalize";
  if (!Q) return MSFM_E_INVAL;
  msfm_ctx* ctx = Q->ctx;
  if (Q->poisoned) return rec::poisoned_error(ctx, who);
  if (target_deviation != target_deviation || point_sigma != point_sigma)
    return msfm_set_error(ctx, MSFM_E_INVAL, "%s: an option is NaN", who);
  const int n = Q->n_points;
  if (n == 0) return msfm_set_error(ctx, MSFM_E_INVAL, "%s: the state has no point", who);
  RC_TRY(hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  DevBuf<double> d_out, d_noise;
  DevScope sc(ctx);
  RC_TRY(d_out.alloc(5));
  if (noise) RC_TRY(sc.up(d_noise, noise, 3 * (size_t)n));
  {
    KTimer tm(ctx, "recon_normalize_sums");
    hipLaunchKernelGGL(k_normalize_sums, dim3(1), dim3(64), 0, s, n, Q->d_xyz.p, target_deviation, d_out.p);
  }
  RC_TRY(hipGetLastError());
  double h[5] = {0, 0, 0, 0, 0};
  RC_TRY(sc.down(h, (const double*)d_out.p, 5));
  RC_TRY(sc.finish());   // the one wait
  if (!std::isfinite(h[4]) || !std::isfinite(h[0]) || !std::isfinite(h[1]) || !std::isfinite(h[2]))
    return msfm_set_error(ctx, MSFM_E_NUMERIC, "%s: scale = %g / %g is not finite", who, target_deviation, h[3]);
  {
    KTimer tm(ctx, "recon_normalize_write");
    hipLaunchKernelGGL(k_normalize_write, dim3(cdiv(3 * (long)n, 256)), dim3(256), 0, s, 3 * (long)n, h[0], h[1], h[2], h[4], noise ? d_noise.p : nullptr,
                       point_sigma, Q->d_xyz.p);
  }
  RC_TRY(hipGetLastError());
  // the write kernel reads the noise behind this return: the object keeps the block; the one it held has been waited for above
  Q->d_noise.swap(d_noise);
  Q->h2d_bytes += sc.h2d;
  if (mid) { mid[0] = h[0]; mid[1] = h[1]; mid[2] = h[2]; }
  if (scale) *scale = h[4];
  return MSFM_OK;
}

MSFM_API int msfm_recon_set_cameras(msfm_recon* Q, const double* cam_pose, const double* cam_R, const double* cam_t, const double* cam_c) {
  if (!Q) return MSFM_E_INVAL;
  if (Q->poisoned) return rec::poisoned_error(Q->ctx, "msfm_recon_set_cameras");
  const size_t nc = (size_t)Q->n_cams;
  if (cam_pose) Q->cam_pose.assign(cam_pose, cam_pose + 6 * nc);
  if (cam_R) Q->cam_R.assign(cam_R, cam_R + 9 * nc);
  if (cam_t) Q->cam_t.assign(cam_t, cam_t + 3 * nc);
  if (cam_c) Q->cam_c.assign(cam_c, cam_c + 3 * nc);
  return MSFM_OK;
}

MSFM_API int msfm_recon_size(const msfm_recon* Q, int* n_cams, int* n_models, int* n_points, int* n_obs, int64_t* cap_points, int64_t* cap_obs,
                             int64_t* h2d_bytes) {
  if (!Q) return MSFM_E_INVAL;
  if (n_cams) *n_cams = Q->n_cams;
  if (n_models) *n_models = Q->n_models;
  if (n_points) *n_points = Q->n_points;
  if (n_obs) *n_obs = Q->n_obs;
  if (cap_points) *cap_points = (int64_t)Q->cap_points;
  if (cap_obs) *cap_obs = (int64_t)Q->cap_obs;
  if (h2d_bytes) *h2d_bytes = Q->h2d_bytes;
  return MSFM_OK;
}

MSFM_API int msfm_recon_fetch(msfm_recon* Q, int32_t* cam_img, int32_t* feat_point, int32_t* obs_point, int32_t* obs_cam, int32_t* obs_feat,
                              double* point_xyz, uint8_t* pt_bad, double* pt_mse, int32_t* pt_views, uint8_t* pt_mutable, uint8_t* pt_new_added,
                              double* cam_pose, double* cam_model, int32_t* cam_model_of_cam, double* cam_R, double* cam_t, double* cam_c,
                              double* cam_fk) {
  if (!Q) return MSFM_E_INVAL;
  msfm_ctx* ctx = Q->ctx;
  if (cam_img) std::copy(Q->cam_img.begin(), Q->cam_img.end(), cam_img);
  if (cam_pose) std::copy(Q->cam_pose.begin(), Q->cam_pose.end(), cam_pose);
  if (cam_model) std::copy(Q->cam_model.begin(), Q->cam_model.end(), cam_model);
  if (cam_model_of_cam) std::copy(Q->cam_model_of_cam.begin(), Q->cam_model_of_cam.end(), cam_model_of_cam);
  if (cam_R) std::copy(Q->cam_R.begin(), Q->cam_R.end(), cam_R);
  if (cam_t) std::copy(Q->cam_t.begin(), Q->cam_t.end(), cam_t);
  if (cam_c) std::copy(Q->cam_c.begin(), Q->cam_c.end(), cam_c);
  if (cam_fk) std::copy(Q->cam_fk.begin(), Q->cam_fk.end(), cam_fk);
  RC_TRY(hipSetDevice(ctx->device));
  DevScope sc(ctx);
  size_t FP = 0;
  for (int c = 0; c < Q->n_cams; c++) FP += (size_t)Q->store->n_features[Q->cam_img[c]];
  const size_t npx = (size_t)Q->n_points, nox = (size_t)Q->n_obs;
  RC_TRY(sc.down(feat_point, Q->d_fp.p, FP));
  RC_TRY(sc.down(obs_point, Q->d_op.p, nox)); RC_TRY(sc.down(obs_cam, Q->d_oc.p, nox)); RC_TRY(sc.down(obs_feat, Q->d_of.p, nox));
  RC_TRY(sc.down(point_xyz, Q->d_xyz.p, 3 * npx)); RC_TRY(sc.down(pt_bad, Q->d_bad.p, npx)); RC_TRY(sc.down(pt_mse, Q->d_mse.p, npx));
  RC_TRY(sc.down(pt_views, Q->d_views.p, npx)); RC_TRY(sc.down(pt_mutable, Q->d_mut.p, npx)); RC_TRY(sc.down(pt_new_added, Q->d_added.p, npx));
  RC_TRY(sc.finish());
  return MSFM_OK;
}

MSFM_API int msfm_recon_adjust(msfm_recon* Q, int new_cam, int n_visible, const int32_t* visible, int do_partial, int do_full, int do_outliers,
                               const msfm_round_options* opt_in, msfm_round_set** out) {
  const char* who = "msfm_recon_adjust";
  if (!Q) return MSFM_E_INVAL;
  msfm_ctx* ctx = Q->ctx;
  if (!out) return msfm_set_error(ctx, MSFM_E_INVAL, "%s: null argument", who);
  *out = nullptr;
  msfm_round_options opt;
  if (opt_in) opt = *opt_in; else msfm_round_default_options(&opt);
  if (n_visible < 0) return msfm_set_error(ctx, MSFM_E_INVAL, "%s: negative count", who);
  if (n_visible && !visible) return msfm_set_error(ctx, MSFM_E_INVAL, "%s: null array", who);
  // every refusal lies in front of the first write to the state: the checks of msfm_round_adjust that need no bulk array
  // (the indices of the state were checked when it was uploaded)
  if (Q->poisoned) return rec::poisoned_error(ctx, who);
  RoundArgs A = rec::args_of(Q);
  A.new_cam = new_cam; A.n_visible = n_visible; A.visible = visible;
  A.do_partial = do_partial != 0; A.do_full = do_full != 0; A.do_outliers = do_outliers != 0;
  RoundTables T;
  MSFM_TRY(round_tables(ctx, who, Q->store, A, /*packed_kp=*/false, opt, &T));
  MSFM_TRY(round_key_check(ctx, who, Q->n_cams, T));
  Child<msfm_round_set> R = child_new<msfm_round_set>(ctx);
  R->n_cams = Q->n_cams; R->n_models = Q->n_models; R->n_points = 0;   // the points stay where they are
  R->keep_problem = opt.keep_problem != 0;
  R->cam_pose = Q->cam_pose; R->cam_model = Q->cam_model;
  memset(R->summary, 0, sizeof R->summary);
  RC_TRY(hipSetDevice(ctx->device));
  RoundDev D;
  D.feat_point = Q->d_fp.p; D.obs_point = Q->d_op.p; D.obs_cam = Q->d_oc.p; D.obs_feat = Q->d_of.p;
  D.point_xyz = Q->d_xyz.p; D.pt_mse = Q->d_mse.p; D.pt_bad = Q->d_bad.p; D.pt_mutable = Q->d_mut.p; D.pt_new_added = Q->d_added.p;
  D.kp = Q->own_kp ? Q->d_kp.p : Q->store->d_kp.p;
  int64_t h2d = 0;
  if (int rc = round_adjust_dev(ctx, who, A, T, D, opt, &h2d, R.get(), /*fetch_points=*/false)) {
    Q->poisoned = true;   // (a stage may have written while the host tables keep the cameras of before the call)
    return rc;
  }
  // the cameras and models as the solves left them (pt_views is not written: apply_round of the flat state leaves it too)
  Q->cam_pose = R->cam_pose; Q->cam_model = R->cam_model;
  Q->cam_R = R->cam_R; Q->cam_t = R->cam_t; Q->cam_c = R->cam_c; Q->cam_fk = R->cam_fk;
  Q->h2d_bytes += h2d;
  R->h2d_bytes = h2d;
  *out = R.release();
  return MSFM_OK;
}

// Room for `points` points and `obs` rows: the arrays that are too short move into blocks of twice the need, device to device on
// the context's stream; the old blocks go back to the pool only behind the scope's wait for the copies that read them.
static int recon_reserve(msfm_recon* Q, size_t points, size_t obs) {
  msfm_ctx* ctx = Q->ctx;
  hipStream_t s = ctx->stream;
  const bool gp = points > Q->cap_points, go = obs > Q->cap_obs;
  if (!gp && !go) return MSFM_OK;
  const size_t cp = gp ? 2 * points : Q->cap_points, co = go ? 2 * obs : Q->cap_obs;
  if (cp > 0x7fffffffUL || co > 0x7fffffffUL) return msfm_set_error(ctx, MSFM_E_INVAL, "msfm_recon: more than 2^31 points or rows");
  const size_t np = (size_t)Q->n_points, no = (size_t)Q->n_obs;
  DevBuf<int> op, oc, of, views;
  DevBuf<double> xyz, mse;
  DevBuf<uint8_t> bad, mut, added;
  DevScope sc(ctx);
  auto move = [&](auto& fresh, auto& old, size_t cap, size_t cnt) -> hipError_t {
    hipError_t e = fresh.alloc(cap);
    if (e != hipSuccess) return e;
    if (cnt) e = hipMemcpyAsync(fresh.p, old.p, cnt * sizeof(*old.p), hipMemcpyDeviceToDevice, s);
    return e;
  };
  if (go) { RC_TRY(move(op, Q->d_op, co, no)); RC_TRY(move(oc, Q->d_oc, co, no)); RC_TRY(move(of, Q->d_of, co, no)); }
  if (gp) {
    RC_TRY(move(xyz, Q->d_xyz, 3 * cp, 3 * np)); RC_TRY(move(mse, Q->d_mse, cp, np)); RC_TRY(move(views, Q->d_views, cp, np));
    RC_TRY(move(bad, Q->d_bad, cp, np)); RC_TRY(move(mut, Q->d_mut, cp, np)); RC_TRY(move(added, Q->d_added, cp, np));
  }
  RC_TRY(sc.finish());   // the copies have read the old blocks
  if (go) { Q->d_op.swap(op); Q->d_oc.swap(oc); Q->d_of.swap(of); Q->cap_obs = co; }
  if (gp) { Q->d_xyz.swap(xyz); Q->d_mse.swap(mse); Q->d_views.swap(views); Q->d_bad.swap(bad); Q->d_mut.swap(mut); Q->d_added.swap(added); Q->cap_points = cp; }
  return MSFM_OK;
}

MSFM_API int msfm_recon_new_points(msfm_recon* Q, int new_cam, int n_visible, const int32_t* visible, const msfm_new_points_options* opt_in, int* n_new,
                                   msfm_new_points_set** stats) {
  using namespace rec;
  const char* who = "msfm_recon_new_points";
  if (!Q) return MSFM_E_INVAL;
  msfm_ctx* ctx = Q->ctx;
  const msfm_match_store* S = Q->store;
  if (stats) *stats = nullptr;
  if (!n_new) return msfm_set_error(ctx, MSFM_E_INVAL, "%s: null argument", who);
  *n_new = 0;
  if (n_visible < 0) return msfm_set_error(ctx, MSFM_E_INVAL, "%s: negative count", who);
  if (n_visible && !visible) return msfm_set_error(ctx, MSFM_E_INVAL, "%s: null array", who);
  msfm_new_points_options opt;
  if (opt_in) opt = *opt_in; else msfm_new_points_default_options(&opt);
  if (Q->poisoned) return rec::poisoned_error(ctx, who);
  const int vis_off[2] = {0, n_visible};
  NewPointsArgs A;
  A.n_cams = Q->n_cams; A.cam_img = Q->cam_img.data();
  A.cam_R = Q->cam_R.data(); A.cam_t = Q->cam_t.data(); A.cam_c = Q->cam_c.data(); A.cam_fk = Q->cam_fk.data();
  A.n_new = 1; A.new_cam = &new_cam; A.vis_off = vis_off; A.vis_cam = visible;
  // every refusal lies in front of the first write to the state: msfm_new_points' checks of the cameras, lists and thresholds
  std::unique_ptr<msfm_new_points_set> R(new msfm_new_points_set());
  NewPointsPlan L;
  MSFM_TRY(newpoints_plan(ctx, who, S, A, opt, /*fp_resident=*/true, Q->own_kp ? NP_KP_ALL : NP_KP_STORE, &L, R.get()));
  if (L.M == 0) {   // no match in the walk: no point
    if (stats) *stats = R.release();
    return MSFM_OK;
  }
  RC_TRY(hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  NewPointsDev W;
  DevBuf<int> d_row_cam;
  DevScope sc(ctx);
  MSFM_TRY(newpoints_dev(ctx, S, A, L, opt, Q->d_fp.p, Q->own_kp ? Q->d_kp.p : S->d_kp.p, sc, &W));
  // what comes back: the accepted count of every visible entry - their sum sizes the append; with `stats` the whole block
  const size_t Ex = (size_t)L.E;
  std::vector<double> h_out;
  std::vector<int> n_acc(Ex, 0);
  if (stats) {
    h_out.resize((W.out_bytes + 7) / 8);
    RC_TRY(hipMemcpyAsync(h_out.data(), W.d_out.p, W.out_bytes, hipMemcpyDeviceToHost, s));
  } else {
    RC_TRY(hipMemcpyAsync(n_acc.data(), W.d_out.p + W.o_na, sizeof(int) * Ex, hipMemcpyDeviceToHost, s));
  }
  RC_TRY(hipStreamSynchronize(s));
  if (stats) {
    newpoints_collect(A, L, W, (const char*)h_out.data(), R.get());
    n_acc = R->n_accepted;
  }
  long total = 0;
  for (size_t q = 0; q < Ex; q++) total += n_acc[q];
  if ((long)Q->n_points + total > 0x7fffffffL || (long)Q->n_obs + 2 * total > 0x7fffffffL)
    return msfm_set_error(ctx, MSFM_E_INVAL, "%s: more than 2^31 points or rows", who);
  const int n = (int)total;
  if (n) {
    MSFM_TRY(recon_reserve(Q, (size_t)Q->n_points + (size_t)n, (size_t)Q->n_obs + 2 * (size_t)n));
    RC_TRY(sc.up(d_row_cam, L.involved));
    {
      KTimer tm(ctx, "recon_append_points");
      hipLaunchKernelGGL(k_append_points, dim3(cdiv(n, 256)), dim3(256), 0, s, n, L.E, new_cam, Q->n_points, Q->n_obs, W.d_offa.p, W.d_ent.p, d_row_cam.p,
                         (const int*)(W.d_out.p + W.o_w), (const int*)(W.d_out.p + W.o_f1), (const int*)(W.d_out.p + W.o_f2), (const double*)W.d_out.p,
                         (const double*)(W.d_out.p + W.o_mse), (const uint8_t*)(W.d_out.p + W.o_t1), (const uint8_t*)(W.d_out.p + W.o_t2), Q->d_fp.p,
                         Q->d_op.p, Q->d_oc.p, Q->d_of.p, Q->d_xyz.p, Q->d_mse.p, Q->d_views.p, Q->d_bad.p, Q->d_mut.p, Q->d_added.p);
    }
    RC_TRY(hipGetLastError());
  }
  RC_TRY(sc.finish());   // the append has read W's blocks
  Q->n_points += n; Q->n_obs += 2 * n;
  Q->h2d_bytes += sc.h2d;
  R->h2d_bytes = sc.h2d;
  *n_new = n;
  if (stats) *stats = R.release();
  return MSFM_OK;
}

MSFM_API int msfm_recon_localize(msfm_recon* Q, int n_cand, const int32_t* cand_img, const int32_t* fail_times, const double* cand_f,
                                 const double* cand_f_init, const msfm_localize_pose_options* opt_in, msfm_recon_winner* out) {
  const char* who = "msfm_recon_localize";
  if (!Q) return MSFM_E_INVAL;
  msfm_ctx* ctx = Q->ctx;
  if (!out) return msfm_set_error(ctx, MSFM_E_INVAL, "%s: null argument", who);
  if (Q->poisoned) return rec::poisoned_error(ctx, who);
  if (n_cand < 0) return msfm_set_error(ctx, MSFM_E_INVAL, "%s: negative count", who);
  if (n_cand && (!cand_img || !fail_times || !cand_f)) return msfm_set_error(ctx, MSFM_E_INVAL, "%s: null array", who);
  msfm_localize_pose_options opt;
  if (opt_in) opt = *opt_in; else msfm_localize_pose_default_options(&opt);
  // a call that is refused leaves the last call's lists and its pending winner as they were; one that succeeds replaces them
  std::vector<int> ranked, failed, visible;
  DevBuf<int> pend_feat, pend_point;
  DevBuf<uint8_t> pend_state;
  bool pending = false;
  int64_t h2d = 0;
  msfm_recon_winner W;
  memset(&W, 0, sizeof W);
  W.image = -1; W.row = -1;
  RC_TRY(hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  DevScope sc(ctx);   // the pending blocks of this call
  msfm_localize_problem P;
  memset(&P, 0, sizeof P);
  P.n_cams = Q->n_cams; P.cam_img = Q->cam_img.data(); P.n_points = Q->n_points; P.n_cand = n_cand; P.cand_img = cand_img; P.fail_times = fail_times;
  LocalizeDev D{Q->d_fp.p, Q->d_bad.p, Q->d_mse.p, Q->d_views.p, Q->d_xyz.p, Q->own_kp ? Q->d_kp.p : nullptr};
  msfm_localize_set* L = nullptr;
  MSFM_TRY(localize_candidates_dev(ctx, who, Q->store, &P, &D, &L));
  struct Guard { msfm_localize_set* p; ~Guard() { msfm_localize_set_destroy(p); } } guard{L};   // (waits for the stream)
  h2d += L->h2d_bytes;
  const int n = (int)L->rank.size();
  for (int r = 0; r < n; r++) ranked.push_back(cand_img[L->rank[r]]);
  W.n_ranked = n;
  std::vector<double> row_f(std::max(1, n)), row_fi(std::max(1, n), 0.0);
  for (int r = 0; r < n; r++) {
    row_f[r] = cand_f[L->rank[r]];
    if (cand_f_init) row_fi[r] = cand_f_init[L->rank[r]];
  }
  // the tries in chunks of max_tries rows, until a row passes or the rows run out (localize.py::localize_next_image)
  int row = opt.first_row;
  while (row >= 0 && n) {
    msfm_localize_pose_options o = opt;
    o.first_row = row;
    msfm_localize_pose_set* R = nullptr;
    DevBuf<uint8_t> d_state;
    DevScope chunk(ctx);   // d_state returns to the pool behind the copies below: never settled, every chunk ends in its wait
    MSFM_TRY(localize_poses_dev(ctx, who, L, row_f.data(), cand_f_init ? row_fi.data() : nullptr, Q->n_points, nullptr, Q->d_added.p, &o, &R, &d_state, &h2d));
    std::unique_ptr<msfm_localize_pose_set> own(R);
    W.n_chunks++;
    const int w = R->winner;
    for (int r = 0; r < n; r++)
      if (R->tried[r] && (w < 0 || r < w)) failed.push_back(ranked[r]);
    if (w >= 0) {
      const int b = L->corr_off[w], cnt = L->corr_off[w + 1] - b;
      RC_TRY(pend_feat.alloc(cnt)); RC_TRY(pend_point.alloc(cnt)); RC_TRY(pend_state.alloc(cnt));
      RC_TRY(hipMemcpyAsync(pend_feat.p, L->d_cf.p + b, sizeof(int) * (size_t)cnt, hipMemcpyDeviceToDevice, s));
      RC_TRY(hipMemcpyAsync(pend_point.p, L->d_cp.p + b, sizeof(int) * (size_t)cnt, hipMemcpyDeviceToDevice, s));
      RC_TRY(hipMemcpyAsync(pend_state.p, d_state.p + b, (size_t)cnt, hipMemcpyDeviceToDevice, s));
      W.image = ranked[w]; W.row = w; W.n_corr = cnt;
      W.f = R->f[w]; W.avg_error = R->avg[w]; W.n_inliers = R->n_in[w]; W.n_outliers = R->n_out[w];
      std::copy(R->R.begin() + 9 * (size_t)w, R->R.begin() + 9 * (size_t)w + 9, W.R);
      std::copy(R->t.begin() + 3 * (size_t)w, R->t.begin() + 3 * (size_t)w + 3, W.t);
      visible.assign(L->vis_cam.begin() + L->vis_off[w], L->vis_cam.begin() + L->vis_off[w + 1]);
      pending = true;
      break;
    }
    row = R->next_row;
  }
  W.n_failed = (int)failed.size();
  W.n_visible = (int)visible.size();
  RC_TRY(sc.finish());   // the old pending blocks return to the pool behind whatever read them
  Q->ranked.swap(ranked); Q->failed.swap(failed); Q->visible.swap(visible);
  Q->pend_feat.swap(pend_feat); Q->pend_point.swap(pend_point); Q->pend_state.swap(pend_state);
  Q->pending = pending;
  Q->h2d_bytes += h2d;
  Q->winner = W;
  *out = W;
  return MSFM_OK;
}

MSFM_API int msfm_recon_localize_fetch(const msfm_recon* Q, int32_t* ranked, int32_t* failed, int32_t* visible) {
  if (!Q) return MSFM_E_INVAL;
  if (ranked) std::copy(Q->ranked.begin(), Q->ranked.end(), ranked);
  if (failed) std::copy(Q->failed.begin(), Q->failed.end(), failed);
  if (visible) std::copy(Q->visible.begin(), Q->visible.end(), visible);
  return MSFM_OK;
}

MSFM_API int msfm_recon_commit_camera(msfm_recon* Q, const double* cam_pose6, int model, const double* cam_model3, int model_mutable, int* new_cam,
                                      int32_t* visible) {
  using namespace rec;
  const char* who = "msfm_recon_commit_camera";
  if (!Q) return MSFM_E_INVAL;
  msfm_ctx* ctx = Q->ctx;
  if (!cam_pose6 || !new_cam) return msfm_set_error(ctx, MSFM_E_INVAL, "%s: null argument", who);
  if (Q->poisoned) return rec::poisoned_error(ctx, who);
  if (!Q->pending) return msfm_set_error(ctx, MSFM_E_INVAL, "%s: no pending localisation (none found, or committed already)", who);
  if (model < 0 || model > Q->n_models) return msfm_set_error(ctx, MSFM_E_INVAL, "%s: model = %d outside n_models = %d", who, model, Q->n_models);
  if (model == Q->n_models && !cam_model3) return msfm_set_error(ctx, MSFM_E_INVAL, "%s: a new model needs cam_model3", who);
  const msfm_recon_winner& W = Q->winner;
  const msfm_match_store* S = Q->store;
  long fp_off = 0;
  for (int c = 0; c < Q->n_cams; c++) fp_off += S->n_features[Q->cam_img[c]];
  const int nf = S->n_features[W.image], n = W.n_corr, n2 = W.n_inliers, c1 = Q->n_cams;
  if (fp_off + nf > 0x7fffffffL || (long)Q->n_obs + n2 > 0x7fffffffL) return msfm_set_error(ctx, MSFM_E_INVAL, "%s: more than 2^31 features or rows", who);
  RC_TRY(hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  MSFM_TRY(recon_reserve(Q, (size_t)Q->n_points, (size_t)Q->n_obs + (size_t)n2));
  DevBuf<int> flag, pos;
  PrimTmp tmp;
  DevScope sc(ctx);
  RC_TRY(flag.alloc((size_t)n + 1)); RC_TRY(pos.alloc((size_t)n + 1));
  if (nf) RC_TRY(hipMemsetD32Async((hipDeviceptr_t)(Q->d_fp.p + fp_off), -1, (size_t)nf, s));   // Camera::pts_ of a new camera: no point anywhere
  {
    KTimer tm(ctx, "recon_commit");
    tm.count = 3;
    hipLaunchKernelGGL(k_commit_flags, dim3(cdiv(n + 1, 256)), dim3(256), 0, s, n, Q->pend_state.p, flag.p);
    RC_TRY(prim_scan_excl(tmp, flag.p, pos.p, (size_t)n + 1, s));
    hipLaunchKernelGGL(k_commit, dim3(cdiv(n, 256)), dim3(256), 0, s, n, c1, (int)fp_off, Q->n_obs, Q->pend_feat.p, Q->pend_point.p, Q->pend_state.p, pos.p,
                       Q->d_fp.p, Q->d_bad.p, Q->d_views.p, Q->d_added.p, Q->d_op.p, Q->d_oc.p, Q->d_of.p);
  }
  RC_TRY(hipGetLastError());
  RC_TRY(sc.finish());
  // the host tables: SetRTPose keeps R, t and c = -(R^T t), the products summed in row order
  if (model == Q->n_models) {
    Q->cam_model.insert(Q->cam_model.end(), cam_model3, cam_model3 + 3);
    if (!Q->model_mutable.empty() || !model_mutable) {
      if (Q->model_mutable.empty()) Q->model_mutable.assign((size_t)Q->n_models, 1);
      Q->model_mutable.push_back(model_mutable ? 1 : 0);
    }
    Q->n_models++;
  }
  Q->cam_img.push_back(W.image);
  Q->cam_model_of_cam.push_back(model);
  Q->cam_pose.insert(Q->cam_pose.end(), cam_pose6, cam_pose6 + 6);
  Q->cam_R.insert(Q->cam_R.end(), W.R, W.R + 9);
  Q->cam_t.insert(Q->cam_t.end(), W.t, W.t + 3);
  for (int k = 0; k < 3; k++) Q->cam_c.push_back(-((W.R[k] * W.t[0] + W.R[3 + k] * W.t[1]) + W.R[6 + k] * W.t[2]));
  // (f, k1, k2) as apply_localized_image keeps it: the localised focal length, the model's distortion (the adjustment refreshes all three)
  Q->cam_fk.push_back(W.f); Q->cam_fk.push_back(Q->cam_model[3 * (size_t)model + 1]); Q->cam_fk.push_back(Q->cam_model[3 * (size_t)model + 2]);
  Q->n_cams++;
  Q->n_obs += n2;
  Q->pending = false;
  *new_cam = c1;
  if (visible) {   // UpdateVisibleGraph (:1895-1903): itself, then the visible cameras
    visible[0] = c1;
    std::copy(Q->visible.begin(), Q->visible.end(), visible + 1);
  }
  return MSFM_OK;
}

MSFM_API void msfm_recon_destroy(msfm_recon* Q) { msfm_child_destroy(Q); }
