// Which images can be localised next, and from which 2D-3D correspondences: the search half of
//   IncrementalSfM::FindImageToLocalize     SfM/src/sfm_incremental.cc:440-562
// for a whole candidate list in one call, on match lists that stay resident (msfm_match_store; the reference re-reads and
// parses `<i>_match` through Graph::QueryMatch, graph.cc:92-137, for every candidate x registered image in every round).
//
// Per candidate image i the reference walks the registered images j in ascending id and the matches of (i, j) in stored
// order (:452-480).  A match (f_i, f_j) qualifies when camera(j) holds a point under f_j that is not badly estimated
// (:486-487); it then does corres_2d3d_i.insert(f_i -> point) and corres_2d3d_info_i.insert(f_i -> mse [+ 3.0 when the point has
// <= 2 views]) (:489-496) - std::map::insert, so the FIRST qualifying match that names f_i wins - and counts (:497) whether the
// insert took or not; camera(j) is visible with more than 5 counted matches (:503).  The correspondences are then ordered by
// that mse (:517-531) and the candidates by n_corr / (5 + fail_times), integer division, zero dropped (:537-562).
//
// Here: the store is sorted by (idx1, idx2), so the position of a match in the walk is monotone in its index -
//   k_resolve   one thread per match of the (candidate, registered) pairs: atomicMin of the walk position into the slot of
//               (candidate, f_i) = "first insert wins"; the per-pair count is a wave ballot + one integer atomicAdd
//   k_count     winners per candidate (the host ranks the candidates from these: n_cand is tens)
//   k_emit      per kept candidate a block scan over its feature slots: winners in f_i order with the order-preserving
//               64-bit image of the mse (NaN last, -0.0 = +0.0)
//   sort        by that key, ties to the lower f_i (= emit order): segments of up to LOC_LDS_MAX in LDS (bitonic on
//               (key, emit index)), longer ones by rocPRIM's stable segmented radix sort - a total order, so both agree
//   k_gather    corr_feat / corr_point in sorted order and, when asked for, pts_w / pts_2d as msfm_epnp_ransac_batch takes them
//               (these three stay on the device inside the set: msfm_localize_poses, localize_pose.hip, reads them there)
// Integer atomics only; nothing depends on the order in which threads run.  Per call the host sends O(registered features +
// points + pairs of the candidates' rows); nothing that scales with the number of matches crosses PCIe.
#include <algorithm>
#include <cstring>
#include <memory>

#include "prim_device.h"

// Longest segment k_sort_lds takes: 4096 x (8-byte key + 4-byte index) = 48 KiB of the CU's 160 KiB LDS, below the 64 KiB a
// workgroup may declare statically, and three such workgroups fit a CU.  MSFM_LOCALIZE_LDS_MAX lowers it (0: everything
// through rocPRIM).
#define LOC_LDS_MAX 4096
#define LOC_BIG 0x7fffffff

namespace loc {

struct WorkPair { int w0, m0, cand, fp0; };   // first walk position, first match in the store, candidate, feat_point base of camera(j)

__global__ __launch_bounds__(256) void k_check_matches(int M, int n_pairs, const int* __restrict__ match_off, const int* __restrict__ pair_img,
                                                        const int* __restrict__ matches, const int* __restrict__ n_features, int* __restrict__ err) {
  const int m = blockIdx.x * 256 + threadIdx.x;
  if (m >= M) return;
  int lo = 0, hi = n_pairs;   // invariant: match_off[lo] <= m < match_off[hi]
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (match_off[mid] <= m) lo = mid; else hi = mid;
  }
  const int f1 = matches[2 * (size_t)m], f2 = matches[2 * (size_t)m + 1];
  if (f1 < 0 || f1 >= n_features[pair_img[2 * lo]] || f2 < 0 || f2 >= n_features[pair_img[2 * lo + 1]]) atomicMin(err, m);
}

__global__ __launch_bounds__(256) void k_check_points(int n, int n_points, const int* __restrict__ feat_point, int* __restrict__ err) {
  const int x = blockIdx.x * 256 + threadIdx.x;
  if (x < n && feat_point[x] >= n_points) atomicMin(err, x);
}

// the work pair of walk position w: last q with wp[q].w0 <= w (only pairs with matches are listed: w0 strictly ascending)
__device__ static inline int pair_of(const WorkPair* __restrict__ wp, int nwp, int w) {
  int lo = 0, hi = nwp;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (wp[mid].w0 <= w) lo = mid; else hi = mid;
  }
  return lo;
}

__global__ __launch_bounds__(256) void k_resolve(int W, int nwp, const WorkPair* __restrict__ wp, const int* __restrict__ matches,
                                                  const int* __restrict__ feat_point, int n_points, const uint8_t* __restrict__ pt_bad,
                                                  const int* __restrict__ slot_off, int* __restrict__ first, int* __restrict__ pcount) {
  const int w = blockIdx.x * 256 + threadIdx.x;
  const bool in = w < W;
  int q = 0;
  bool ok = false;
  if (in) {
    q = pair_of(wp, nwp, w);
    const WorkPair P = wp[q];
    const size_t m = (size_t)P.m0 + (w - P.w0);
    const int fi = matches[2 * m], fj = matches[2 * m + 1];
    const int p = feat_point[(size_t)P.fp0 + fj];
    ok = p >= 0 && p < n_points && !pt_bad[p];                   // :486-487
    if (ok) atomicMin(&first[(size_t)slot_off[P.cand] + fi], w);   // std::map::insert: the earliest position of the walk keeps the key
  }
  // count_2d3d_ij (:497): every qualifying match.  A wave mostly lies inside one pair: one add for all its lanes.
  const int q0 = __shfl(q, 0);
  if (__all(!in || q == q0)) {
    const unsigned long long b = __ballot(ok);
    if ((threadIdx.x & 63) == 0 && b) atomicAdd(&pcount[q0], __popcll(b));
  } else if (ok) {
    atomicAdd(&pcount[q], 1);
  }
}

__global__ __launch_bounds__(256) void k_count(const int* __restrict__ slot_off, const int* __restrict__ first, int* __restrict__ n_corr) {
  __shared__ int part[4];
  const int k = blockIdx.x;
  const int b = slot_off[k], e = slot_off[k + 1];
  int c = 0;
  for (int s = b + threadIdx.x; s < e; s += 256) c += first[s] != LOC_BIG;
  c = wave_sum_int(c);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = c;
  __syncthreads();
  if (threadIdx.x == 0) n_corr[k] = part[0] + part[1] + part[2] + part[3];
}

// order-preserving image of a double: a < b  <=>  key(a) < key(b); -0.0 and +0.0 share a key, every NaN gets the largest
__device__ static inline unsigned long long mse_key(double v) {
  if (v != v) return ~0ull;
  if (v == 0.0) v = 0.0;
  const unsigned long long u = (unsigned long long)__double_as_longlong(v);
  return (u >> 63) ? ~u : (u | (1ull << 63));
}

__global__ __launch_bounds__(256) void k_emit(const int* __restrict__ slot_off, const int* __restrict__ out_off, const int* __restrict__ kp_off,
                                               const int* __restrict__ first, int nwp, const WorkPair* __restrict__ wp,
                                               const int* __restrict__ matches, const int* __restrict__ feat_point, const double* __restrict__ pt_mse,
                                               const int* __restrict__ pt_views, unsigned long long* __restrict__ key, int* __restrict__ idx,
                                               int* __restrict__ feat, int* __restrict__ point, int* __restrict__ kp_row) {
  __shared__ int part[4];
  const int k = blockIdx.x;
  const int o0 = out_off[k];
  if (o0 < 0) return;   // a dropped candidate (score 0)
  const int b = slot_off[k], n = slot_off[k + 1] - b;
  int base = 0;
  for (int c0 = 0; c0 < n; c0 += 256) {
    const int f = c0 + threadIdx.x;
    const int w = f < n ? first[b + f] : LOC_BIG;
    const bool win = w != LOC_BIG;
    int total;
    const int before = wg_rank<4>(win, part, total);
    if (win) {
      const WorkPair P = wp[pair_of(wp, nwp, w)];
      const size_t m = (size_t)P.m0 + (w - P.w0);
      const int p = feat_point[(size_t)P.fp0 + matches[2 * m + 1]];
      const double v = pt_mse[p] + (pt_views[p] <= 2 ? 3.0 : 0.0);   // :491-495
      const int e = o0 + base + before;
      key[e] = mse_key(v); idx[e] = e; feat[e] = f; point[e] = p; kp_row[e] = kp_off[k] + f;
    }
    base += total;
  }
}

// one workgroup per segment of at most LOC_LDS_MAX entries: bitonic sort of (key, emit index), ascending
__global__ __launch_bounds__(256) void k_sort_lds(const int* __restrict__ seg_begin, const int* __restrict__ seg_end,
                                                   const unsigned long long* __restrict__ key, const int* __restrict__ idx, int* __restrict__ idx_s) {
  __shared__ unsigned long long sk[LOC_LDS_MAX];
  __shared__ unsigned int sv[LOC_LDS_MAX];
  const int b = seg_begin[blockIdx.x], n = seg_end[blockIdx.x] - b;
  int n2 = 1;
  while (n2 < n) n2 <<= 1;
  for (int t = threadIdx.x; t < n2; t += 256) {
    sk[t] = t < n ? key[b + t] : ~0ull;                       // padding sorts behind every entry: same key as a NaN, larger index
    sv[t] = t < n ? (unsigned int)idx[b + t] : 0xffffffffu;
  }
  __syncthreads();
  for (int size = 2; size <= n2; size <<= 1) {
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      for (int t = threadIdx.x; t < (n2 >> 1); t += 256) {
        const int lo = 2 * t - (t & (stride - 1)), hi = lo + stride;
        const unsigned long long ka = sk[lo], kb = sk[hi];
        const unsigned int va = sv[lo], vb = sv[hi];
        const bool gt = ka > kb || (ka == kb && va > vb);
        if (gt == ((lo & size) == 0)) { sk[lo] = kb; sk[hi] = ka; sv[lo] = vb; sv[hi] = va; }
      }
      __syncthreads();
    }
  }
  for (int t = threadIdx.x; t < n; t += 256) idx_s[b + t] = (int)sv[t];
}

__global__ __launch_bounds__(256) void k_gather(int T, const int* __restrict__ idx_s, const int* __restrict__ feat, const int* __restrict__ point,
                                                 const int* __restrict__ kp_row, const double* __restrict__ xyz, const float* __restrict__ kp,
                                                 int* __restrict__ corr_feat, int* __restrict__ corr_point, double* __restrict__ pts_w,
                                                 double* __restrict__ pts_2d) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= T) return;
  const int j = idx_s[e];
  const int p = point[j];
  corr_feat[e] = feat[j];
  corr_point[e] = p;
  if (pts_w) {   // :592-600
    const size_t r = (size_t)kp_row[j];
    pts_w[3 * (size_t)e] = xyz[3 * (size_t)p]; pts_w[3 * (size_t)e + 1] = xyz[3 * (size_t)p + 1]; pts_w[3 * (size_t)e + 2] = xyz[3 * (size_t)p + 2];
    pts_2d[2 * (size_t)e] = (double)kp[2 * r]; pts_2d[2 * (size_t)e + 1] = (double)kp[2 * r + 1];
  }
}

}  // namespace loc

#define LC_TRY(e) HIP_TRY(ctx, (e))

// The checks that are O(images + pairs), the row index, the device check of every feature index.  d_match holds the matches already.
static int store_finish(msfm_ctx* ctx, msfm_match_store* S, const char* who) {
  const int ni = S->n_images, np = S->n_pairs;
  S->feat_off.assign(ni + 1, 0);
  for (int i = 0; i < ni; i++) {
    if (S->n_features[i] < 0) return msfm_set_error(ctx, MSFM_E_INVAL, "%s: n_features[%d] < 0", who, i);
    if ((long)S->feat_off[i] + S->n_features[i] > 0x7fffffffL) return msfm_set_error(ctx, MSFM_E_INVAL, "%s: more than 2^31 features", who);
    S->feat_off[i + 1] = S->feat_off[i] + S->n_features[i];
  }
  if (np && S->match_off[0] != 0) return msfm_set_error(ctx, MSFM_E_INVAL, "%s: match_off[0] != 0", who);
  S->row_off.assign(ni + 1, 0);
  for (int p = 0; p < np; p++) {
    const int i1 = S->pair_img[2 * p], i2 = S->pair_img[2 * p + 1];
    if (i1 < 0 || i1 >= ni || i2 < 0 || i2 >= ni || S->match_off[p + 1] < S->match_off[p])
      return msfm_set_error(ctx, MSFM_E_INVAL, "%s: pair %d", who, p);
    if (p && (S->pair_img[2 * p - 2] > i1 || (S->pair_img[2 * p - 2] == i1 && S->pair_img[2 * p - 1] >= i2)))
      return msfm_set_error(ctx, MSFM_E_INVAL, "%s: pair %d = (%d, %d) is not behind pair %d: pairs must be strictly ascending in (idx1, idx2)", who, p,
                            i1, i2, p - 1);
    S->row_off[i1 + 1]++;
  }
  for (int i = 0; i < ni; i++) S->row_off[i + 1] += S->row_off[i];
  if (S->M == 0) return MSFM_OK;
  hipStream_t s = ctx->stream;
  DevBuf<int> d_nf, d_pair, d_moff, err;
  DevScope sc(ctx);
  LC_TRY(d_nf.from(S->n_features, s)); LC_TRY(d_pair.from(S->pair_img, s)); LC_TRY(d_moff.from(S->match_off, s)); LC_TRY(err.alloc(1));
  const int big = LOC_BIG;
  LC_TRY(hipMemcpyAsync(err.p, &big, sizeof(int), hipMemcpyHostToDevice, s));
  hipLaunchKernelGGL(loc::k_check_matches, dim3(cdiv(S->M, 256)), dim3(256), 0, s, S->M, np, d_moff.p, d_pair.p, S->d_match.p, d_nf.p, err.p);
  LC_TRY(hipGetLastError());
  int bad = big;
  LC_TRY(hipMemcpyAsync(&bad, err.p, sizeof(int), hipMemcpyDeviceToHost, s));
  LC_TRY(sc.finish());
  if (bad != big) return msfm_set_error(ctx, MSFM_E_INVAL, "%s: match %d names a feature outside its image", who, bad);
  return MSFM_OK;
}

MSFM_API int msfm_match_store_create(msfm_ctx* ctx, int n_images, const int* n_features, int n_pairs, const int* pair_img, const int* match_off,
                                     const int* matches, msfm_match_store** out) {
  if (!ctx) return MSFM_E_INVAL;
  if (n_images < 0 || n_pairs < 0 || !out || (n_images && !n_features) || (n_pairs && (!pair_img || !match_off)))
    return msfm_set_error(ctx, MSFM_E_INVAL, "msfm_match_store_create: null argument");
  *out = nullptr;
  const int M = n_pairs ? match_off[n_pairs] : 0;
  if (M < 0 || (M > 0 && !matches)) return msfm_set_error(ctx, MSFM_E_INVAL, "msfm_match_store_create: null matches");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  Child<msfm_match_store> S = child_new<msfm_match_store>(ctx);
  S->n_images = n_images; S->n_pairs = n_pairs; S->M = M;
  S->n_features.assign(n_features, n_features + n_images);
  S->pair_img.assign(pair_img, pair_img + 2 * (size_t)n_pairs);
  if (n_pairs) S->match_off.assign(match_off, match_off + n_pairs + 1); else S->match_off.assign(1, 0);
  S->has_kp.assign(std::max(1, n_images), 0);
  DevScope sc(ctx);
  LC_TRY(S->d_match.alloc(2 * (size_t)std::max(1, M)));
  LC_TRY(S->d_match.upload(matches, 2 * (size_t)M, ctx->stream));
  MSFM_TRY(store_finish(ctx, S.get(), "msfm_match_store_create"));
  LC_TRY(sc.finish());
  *out = S.release();
  return MSFM_OK;
}

MSFM_API int msfm_match_store_from_chain(msfm_chain* chain, msfm_match_store** out) {
  if (!chain || !out) return MSFM_E_INVAL;
  *out = nullptr;
  ChainMatchView v;
  MSFM_TRY(chain_match_view(chain, &v));
  msfm_ctx* ctx = v.ctx;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  Child<msfm_match_store> S = child_new<msfm_match_store>(ctx);
  S->n_images = v.n_images; S->n_pairs = v.n_pairs; S->M = v.match_off[v.n_pairs];
  S->n_features.assign(v.count, v.count + v.n_images);
  S->pair_img.assign(v.pairs, v.pairs + 2 * (size_t)v.n_pairs);
  S->match_off.assign(v.match_off, v.match_off + v.n_pairs + 1);
  S->has_kp.assign(std::max(1, v.n_images), 0);
  long nf = 0;
  for (int i = 0; i < v.n_images; i++) { S->has_kp[i] = v.kp[i] != nullptr; nf += v.count[i]; }
  // copies of its own, device to device: the chain may be destroyed while the store lives
  DevScope sc(ctx);
  LC_TRY(S->d_match.alloc(2 * (size_t)std::max(1, S->M)));
  if (S->M) LC_TRY(hipMemcpyAsync(S->d_match.p, v.d_match, sizeof(int) * 2 * (size_t)S->M, hipMemcpyDeviceToDevice, s));
  LC_TRY(S->d_kp.alloc(2 * (size_t)std::max(1L, nf)));
  if (nf) LC_TRY(hipMemcpyAsync(S->d_kp.p, v.d_kp, sizeof(float) * 2 * (size_t)nf, hipMemcpyDeviceToDevice, s));
  MSFM_TRY(store_finish(ctx, S.get(), "msfm_match_store_from_chain"));
  LC_TRY(sc.finish());
  *out = S.release();
  return MSFM_OK;
}

MSFM_API void msfm_match_store_destroy(msfm_match_store* S) { msfm_child_destroy(S); }

// The call on device arrays: with `dev` the bulk arrays of the state (feat_point, pt_bad, pt_mse, pt_views, point_xyz, keypoints)
// are the caller's resident ones - P then carries counts and the O(cameras + candidates) lists only - and the set keeps its
// correspondences on the device without reading pts_w / pts_2d back.  msfm_localize_candidates is this with dev = NULL: it uploads.
int localize_candidates_dev(msfm_ctx* ctx, const char* who, const msfm_match_store* S, const msfm_localize_problem* P, const LocalizeDev* dev,
                            msfm_localize_set** out) {
  using namespace loc;
  if (!ctx) return MSFM_E_INVAL;
  if (!S || !P || !out) return msfm_set_error(ctx, MSFM_E_INVAL, "%s: null argument", who);
  *out = nullptr;
  if (S->ctx != ctx) return msfm_set_error(ctx, MSFM_E_INVAL, "%s: the store belongs to another context", who);
  const int ni = S->n_images, nc = P->n_cams, nk = P->n_cand, npt = P->n_points;
  if (nc < 0 || nk < 0 || npt < 0 || (nc && !P->cam_img) || (nk && (!P->cand_img || !P->fail_times)) || (npt && !dev && (!P->pt_bad || !P->pt_mse || !P->pt_views)))
    return msfm_set_error(ctx, MSFM_E_INVAL, "%s: null array or negative count", who);
  // ---- O(images + cameras + candidates) on the host ----
  std::vector<int> cam_of_img(std::max(1, ni), -1), cam_fo(nc + 1, 0);
  for (int c = 0; c < nc; c++) {
    const int im = P->cam_img[c];
    if (im < 0 || im >= ni) return msfm_set_error(ctx, MSFM_E_INVAL, "%s: cam_img[%d] = %d is no image of the store", who, c, im);
    if (cam_of_img[im] >= 0) return msfm_set_error(ctx, MSFM_E_INVAL, "%s: image %d has two cameras", who, im);
    cam_of_img[im] = c;
    if ((long)cam_fo[c] + S->n_features[im] > 0x7fffffffL) return msfm_set_error(ctx, MSFM_E_INVAL, "%s: more than 2^31 registered features", who);
    cam_fo[c + 1] = cam_fo[c] + S->n_features[im];
  }
  const int FP = cam_fo[nc];
  if (FP && !dev && !P->feat_point) return msfm_set_error(ctx, MSFM_E_INVAL, "%s: null feat_point", who);
  std::vector<int> slot_off(nk + 1, 0);
  for (int k = 0; k < nk; k++) {
    const int im = P->cand_img[k];
    if (im < 0 || im >= ni) return msfm_set_error(ctx, MSFM_E_INVAL, "%s: cand_img[%d] = %d is no image of the store", who, k, im);
    if (k && P->cand_img[k - 1] >= im) return msfm_set_error(ctx, MSFM_E_INVAL, "%s: cand_img must be strictly ascending", who);
    if (cam_of_img[im] >= 0) return msfm_set_error(ctx, MSFM_E_INVAL, "%s: candidate image %d is registered already", who, im);
    if (P->fail_times[k] < 0) return msfm_set_error(ctx, MSFM_E_INVAL, "%s: fail_times[%d] < 0", who, k);
    if ((long)slot_off[k] + S->n_features[im] > 0x7fffffffL) return msfm_set_error(ctx, MSFM_E_INVAL, "%s: more than 2^31 candidate features", who);
    slot_off[k + 1] = slot_off[k] + S->n_features[im];
  }
  const bool want_pts = dev || P->point_xyz != nullptr;
  const bool own_kp = dev ? dev->kp != nullptr : P->keypoints != nullptr;   // keypoints that do not come from the store
  if (want_pts) {
    for (int k = 0; k < nk; k++)
      if (!own_kp && !S->has_kp[P->cand_img[k]])
        return msfm_set_error(ctx, MSFM_E_INVAL, "%s: point_xyz given, but no keypoints of candidate image %d (argument or chain)", who, P->cand_img[k]);
  }
  // the walk of :452-474 as a list: per candidate (ascending) its row of the store, entries with a registered idx2 and matches
  std::vector<WorkPair> wp;
  std::vector<int> wp_cam;
  long W = 0;
  for (int k = 0; k < nk; k++) {
    const int im = P->cand_img[k];
    for (int p = S->row_off[im]; p < S->row_off[im + 1]; p++) {
      const int c = cam_of_img[S->pair_img[2 * p + 1]];
      const int n = S->match_off[p + 1] - S->match_off[p];
      if (c < 0 || n == 0) continue;
      wp.push_back(WorkPair{(int)W, S->match_off[p], k, cam_fo[c]});
      wp_cam.push_back(c);
      W += n;
    }
  }
  const int nwp = (int)wp.size();
  Child<msfm_localize_set> R = child_new<msfm_localize_set>(ctx);
  R->have_pts = want_pts;
  R->corr_off.assign(1, 0); R->vis_off.assign(1, 0);
  if (nk == 0) { *out = R.release(); return MSFM_OK; }
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  const msfm_env env = msfm_env_read();
  const int lds_max = std::max(0, std::min(env.localize_lds_max, LOC_LDS_MAX));
  const int S_slots = slot_off[nk];
  DevBuf<WorkPair> d_wp;
  DevBuf<int> d_fp, d_views, d_slot, d_first, d_pcount, d_ncorr, d_err;
  DevBuf<uint8_t> d_bad;
  DevBuf<double> d_mse, d_xyz, d_pw, d_p2;
  DevBuf<float> d_kp_up;
  DevBuf<int> d_out, d_kpo, d_idx, d_idx_s, d_feat, d_point, d_kprow, d_cf, d_cp, d_sb, d_se, d_lb, d_le;   // (of the second half: emit, sort, gather)
  DevBuf<unsigned long long> d_key, d_key_s;
  PrimTmp tmp;
  DevScope sc(ctx);
  LC_TRY(sc.up(d_wp, wp.data(), (size_t)nwp)); LC_TRY(sc.up(d_slot, slot_off.data(), (size_t)nk + 1));
  if (!dev) {
    LC_TRY(sc.up(d_fp, P->feat_point, (size_t)FP)); LC_TRY(sc.up(d_bad, P->pt_bad, (size_t)npt));
    LC_TRY(sc.up(d_mse, P->pt_mse, (size_t)npt)); LC_TRY(sc.up(d_views, P->pt_views, (size_t)npt));
  }
  const int* fp_p = dev ? dev->feat_point : d_fp.p;
  const uint8_t* bad_p = dev ? dev->pt_bad : d_bad.p;
  const double* mse_p = dev ? dev->pt_mse : d_mse.p;
  const int* views_p = dev ? dev->pt_views : d_views.p;
  LC_TRY(d_first.alloc(std::max(1, S_slots))); LC_TRY(d_pcount.alloc(nwp)); LC_TRY(d_ncorr.alloc(nk)); LC_TRY(d_err.alloc(1));
  const int big = LOC_BIG;
  LC_TRY(hipMemcpyAsync(d_err.p, &big, sizeof(int), hipMemcpyHostToDevice, s));
  if (S_slots) LC_TRY(hipMemsetD32Async((hipDeviceptr_t)d_first.p, big, (size_t)S_slots, s));
  if (nwp) LC_TRY(hipMemsetAsync(d_pcount.p, 0, sizeof(int) * (size_t)nwp, s));
  {
    KTimer t(ctx, "localize_resolve");
    t.count = (FP ? 1 : 0) + (W ? 1 : 0) + 1;
    if (FP) hipLaunchKernelGGL(k_check_points, dim3(cdiv(FP, 256)), dim3(256), 0, s, FP, npt, fp_p, d_err.p);
    if (W) hipLaunchKernelGGL(k_resolve, dim3(cdiv(W, 256)), dim3(256), 0, s, (int)W, nwp, d_wp.p, S->d_match.p, fp_p, npt, bad_p, d_slot.p,
                              d_first.p, d_pcount.p);
    hipLaunchKernelGGL(k_count, dim3(nk), dim3(256), 0, s, d_slot.p, d_first.p, d_ncorr.p);
  }
  LC_TRY(hipGetLastError());
  int bad = big;
  std::vector<int> n_corr(nk), pcount(nwp);
  LC_TRY(hipMemcpyAsync(&bad, d_err.p, sizeof(int), hipMemcpyDeviceToHost, s));
  LC_TRY(hipMemcpyAsync(n_corr.data(), d_ncorr.p, sizeof(int) * (size_t)nk, hipMemcpyDeviceToHost, s));
  if (nwp) LC_TRY(hipMemcpyAsync(pcount.data(), d_pcount.p, sizeof(int) * (size_t)nwp, hipMemcpyDeviceToHost, s));
  LC_TRY(hipStreamSynchronize(s));
  if (bad != big) {
    int c = 0;
    while (c + 1 < nc && cam_fo[c + 1] <= bad) c++;
    return msfm_set_error(ctx, MSFM_E_INVAL, "%s: feat_point of camera %d, feature %d is no point (n_points = %d)", who, c, bad - cam_fo[c], npt);
  }
  // ---- ranking (:537-562): score = n_corr / (5 + fail_times), descending, ties to the lower image id, zero dropped ----
  std::vector<int> order;
  for (int k = 0; k < nk; k++) if (n_corr[k] / (5 + P->fail_times[k]) > 0) order.push_back(k);
  std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return n_corr[a] / (5 + P->fail_times[a]) > n_corr[b] / (5 + P->fail_times[b]); });
  const int nkept = (int)order.size();
  R->rank = order;
  std::vector<int> out_off(nk, -1), row_of(nk, -1);
  long T = 0;
  for (int r = 0; r < nkept; r++) {
    out_off[order[r]] = (int)T; row_of[order[r]] = r;
    T += n_corr[order[r]];
    R->corr_off.push_back((int)T);
  }
  // visible cameras (:503-506) in the order of the walk; the counts came back as one integer per walked pair
  std::vector<std::vector<int>> vis(nkept);
  for (int q = 0; q < nwp; q++)
    if (row_of[wp[q].cand] >= 0 && pcount[q] > 5) vis[row_of[wp[q].cand]].push_back(wp_cam[q]);
  for (int r = 0; r < nkept; r++) {
    R->vis_cam.insert(R->vis_cam.end(), vis[r].begin(), vis[r].end());
    R->vis_off.push_back((int)R->vis_cam.size());
  }
  R->h2d_bytes = sc.h2d;
  if (T == 0) { sc.dismiss(); *out = R.release(); return MSFM_OK; }   // (behind the wait above: nothing has been enqueued since)
  // ---- emit, sort, gather ----
  std::vector<int> kp_off(nk, 0);
  const float* d_kp = nullptr;
  if (want_pts) {
    if (!dev) LC_TRY(sc.up(d_xyz, P->point_xyz, 3 * (size_t)npt));
    if (dev && dev->kp) {   // every image's rows, resident
      for (int k = 0; k < nk; k++) kp_off[k] = S->feat_off[P->cand_img[k]];
      d_kp = dev->kp;
    } else if (P->keypoints) {   // the rows of the kept candidates only
      long n = 0;
      for (int r = 0; r < nkept; r++) { kp_off[order[r]] = (int)n; n += S->n_features[P->cand_img[order[r]]]; }
      LC_TRY(d_kp_up.alloc(2 * (size_t)std::max(1L, n)));
      for (int r = 0; r < nkept; r++) {
        const int im = P->cand_img[order[r]];
        const size_t cnt = 2 * (size_t)S->n_features[im];
        if (cnt) LC_TRY(hipMemcpyAsync(d_kp_up.p + 2 * (size_t)kp_off[order[r]], P->keypoints + 2 * (size_t)S->feat_off[im], sizeof(float) * cnt,
                                       hipMemcpyHostToDevice, s));
        sc.h2d += (int64_t)(sizeof(float) * cnt);
      }
      d_kp = d_kp_up.p;
    } else {
      for (int k = 0; k < nk; k++) kp_off[k] = S->feat_off[P->cand_img[k]];
      d_kp = S->d_kp.p;
    }
    LC_TRY(d_pw.alloc(3 * (size_t)T)); LC_TRY(d_p2.alloc(2 * (size_t)T));
  }
  std::vector<int> sb, se, lb, le;   // segments for the LDS sort / for rocPRIM
  for (int r = 0; r < nkept; r++) {
    const int b = R->corr_off[r], e = R->corr_off[r + 1];
    if (e - b <= lds_max) { sb.push_back(b); se.push_back(e); } else { lb.push_back(b); le.push_back(e); }
  }
  LC_TRY(sc.up(d_out, out_off.data(), (size_t)nk)); LC_TRY(sc.up(d_kpo, kp_off.data(), (size_t)nk));
  LC_TRY(d_key.alloc(T)); LC_TRY(d_idx.alloc(T)); LC_TRY(d_idx_s.alloc(T)); LC_TRY(d_feat.alloc(T)); LC_TRY(d_point.alloc(T)); LC_TRY(d_kprow.alloc(T));
  LC_TRY(d_cf.alloc(T)); LC_TRY(d_cp.alloc(T));
  LC_TRY(hipMemsetAsync(d_idx_s.p, 0, sizeof(int) * (size_t)T, s));   // (k_gather indexes with it: never an uninitialised value)
  {
    KTimer t(ctx, "localize_emit");
    hipLaunchKernelGGL(k_emit, dim3(nk), dim3(256), 0, s, d_slot.p, d_out.p, d_kpo.p, d_first.p, nwp, d_wp.p, S->d_match.p, fp_p, mse_p, views_p,
                       d_key.p, d_idx.p, d_feat.p, d_point.p, d_kprow.p);
  }
  if (!sb.empty()) {
    LC_TRY(sc.up(d_sb, sb)); LC_TRY(sc.up(d_se, se));
    KTimer t(ctx, "localize_sort_lds");
    hipLaunchKernelGGL(k_sort_lds, dim3((unsigned)sb.size()), dim3(256), 0, s, d_sb.p, d_se.p, d_key.p, d_idx.p, d_idx_s.p);
  }
  if (!lb.empty()) {
    // stable, so equal keys keep the emit order = ascending f_i: the order k_sort_lds spells out
    LC_TRY(sc.up(d_lb, lb)); LC_TRY(sc.up(d_le, le));
    LC_TRY(d_key_s.alloc(T));
    KTimer t(ctx, "localize_sort_rocprim");
    LC_TRY(prim_seg_sort_pairs(tmp, d_key.p, d_key_s.p, d_idx.p, d_idx_s.p, (unsigned)T, (unsigned)lb.size(), d_lb.p, d_le.p, 0, 64, s));
  }
  {
    KTimer t(ctx, "localize_gather");
    hipLaunchKernelGGL(k_gather, dim3(cdiv(T, 256)), dim3(256), 0, s, (int)T, d_idx_s.p, d_feat.p, d_point.p, d_kprow.p, dev ? dev->point_xyz : d_xyz.p, d_kp,
                       d_cf.p, d_cp.p, want_pts ? d_pw.p : nullptr, want_pts ? d_p2.p : nullptr);
  }
  LC_TRY(hipGetLastError());
  R->corr_feat.resize(T); R->corr_point.resize(T);
  LC_TRY(hipMemcpyAsync(R->corr_feat.data(), d_cf.p, sizeof(int) * (size_t)T, hipMemcpyDeviceToHost, s));
  LC_TRY(hipMemcpyAsync(R->corr_point.data(), d_cp.p, sizeof(int) * (size_t)T, hipMemcpyDeviceToHost, s));
  if (want_pts && !dev) {
    R->pts_w.resize(3 * (size_t)T); R->pts_2d.resize(2 * (size_t)T);
    LC_TRY(hipMemcpyAsync(R->pts_w.data(), d_pw.p, sizeof(double) * 3 * (size_t)T, hipMemcpyDeviceToHost, s));
    LC_TRY(hipMemcpyAsync(R->pts_2d.data(), d_p2.p, sizeof(double) * 2 * (size_t)T, hipMemcpyDeviceToHost, s));
  }
  LC_TRY(sc.finish());   // the scratch above is released on return
  R->h2d_bytes = sc.h2d;
  if (want_pts) { R->d_cp.swap(d_cp); R->d_pw.swap(d_pw); R->d_p2.swap(d_p2); }   // resident for msfm_localize_poses
  if (dev) R->d_cf.swap(d_cf);   // (a resident state commits the winner's row from the device)
  *out = R.release();
  return MSFM_OK;
}

MSFM_API int msfm_localize_candidates(msfm_ctx* ctx, const msfm_match_store* S, const msfm_localize_problem* P, msfm_localize_set** out) {
  return localize_candidates_dev(ctx, "msfm_localize_candidates", S, P, nullptr, out);
}

MSFM_API int msfm_localize_set_size(const msfm_localize_set* R, int* n_kept, int* n_corr, int* n_visible, int* has_points, int64_t* h2d_bytes) {
  if (!R) return MSFM_E_INVAL;
  if (n_kept) *n_kept = (int)R->rank.size();
  if (n_corr) *n_corr = (int)R->corr_feat.size();
  if (n_visible) *n_visible = (int)R->vis_cam.size();
  if (has_points) *has_points = R->have_pts ? 1 : 0;
  if (h2d_bytes) *h2d_bytes = R->h2d_bytes;
  return MSFM_OK;
}

MSFM_API int msfm_localize_set_fetch(const msfm_localize_set* R, int* rank, int* corr_off, int* corr_feat, int* corr_point, int* vis_off, int* vis_cam,
                                     double* pts_w, double* pts_2d) {
  if (!R) return MSFM_E_INVAL;
  if ((pts_w || pts_2d) && !R->have_pts) return MSFM_E_INVAL;
  if (rank) std::copy(R->rank.begin(), R->rank.end(), rank);
  if (corr_off) std::copy(R->corr_off.begin(), R->corr_off.end(), corr_off);
  if (corr_feat) std::copy(R->corr_feat.begin(), R->corr_feat.end(), corr_feat);
  if (corr_point) std::copy(R->corr_point.begin(), R->corr_point.end(), corr_point);
  if (vis_off) std::copy(R->vis_off.begin(), R->vis_off.end(), vis_off);
  if (vis_cam) std::copy(R->vis_cam.begin(), R->vis_cam.end(), vis_cam);
  if (pts_w) std::copy(R->pts_w.begin(), R->pts_w.end(), pts_w);
  if (pts_2d) std::copy(R->pts_2d.begin(), R->pts_2d.end(), pts_2d);
  return MSFM_OK;
}

MSFM_API void msfm_localize_set_destroy(msfm_localize_set* R) { msfm_child_destroy(R); }
