// The chain between matching and bundle adjustment with every intermediate result resident in HBM.
//
// The reference walks it through the host for every image pair and every point:
//   match lists -> GeoVerificationFundamental on the "good" set, closed-form filter on the "all" set
//                  (SfM/src/graph/fine_matching_graph.cc:138-153, :182-186)
//   -> data association of SLAMGPS::Triangulation (SfM/src/slam_gps.cc:565-635)
//   -> Point3D::Trianglate2 per point, points with fewer than three views or a failed triangulation marked bad (:638-648)
//   -> the residual blocks of BundleAdjuster::RunOptimizetion (SfM/src/optimizer.cc:59-129).
// Round 2 had a batched entry point for each step, each taking and returning host arrays: the 2-NN kernel of a pair takes
// 40 us inside a 0.63 ms call, the triangulation of config 3's tracks 0.06 ms inside 1.3 ms.  msfm_chain strings the same
// kernels together on device buffers: the match codes stay where msfm_match_pairs left them, the keypoint positions were
// uploaded once beside the descriptors (msfm_descset_upload_keypoints), and what crosses PCIe between the descriptor
// upload and the download of the adjusted parameters is a few integers per image pair (match counts, needed on the host
// to size the next step) plus the cameras.  Every step gives bit for bit what its host-array counterpart gives on the same
// input (tests/test_gpu_chain.py).
//
// A chain takes either form of match result and keeps which one it was made from:
//   msfm_match_pairs       codes with good / all sets -> msfm_chain_verify (above)
//   msfm_match_pairs_slam  codes = survivors of the ratio test and the two prior gates -> msfm_chain_verify_slam: the tail of
//                          SLAMGPS::FeatureMatching step 2 (SfM/src/slam_gps.cc:503-541).  GeoVerificationFundamental runs on ALL
//                          survivors of a pair in query order; there is no good / all split and no closed-form filter behind it.
//                          Then `matches[j] = {matches[j][inliers[k]]}` whatever the function returned:
//     - fewer than min_points (30) survivors: the function returns before RANSAC, `inliers` is empty, the pair keeps NO match;
//     - min_points or more survivors but fewer than min_inliers (30) RANSAC inliers: the function returns false with `inliers`
//       already filled, so the pair KEEPS those 1..29 matches - ok = 0 with n_matches > 0 (in msfm_chain_verify a failed pair
//       keeps none);
//     - no model found: the mask of msfm_fundamental_ransac_batch is all zero and the pair keeps nothing (the documented
//       departure of that call, which msfm_slam_priors carries too).
//   Kept matches are (train feature in id1, query feature m in id2) in ascending m, pairs in the order of the match result.
//   Everything behind the verification (tracks, triangulation, accuracy, registration, bundle adjustment, match store) is the
//   same code on either form (tests/test_gpu_slam_chain.py).
#include <algorithm>
#include <cstring>
#include <memory>

#include "prim_device.h"
#include "../../include/msfm.h"

namespace chn {

struct PairSrc {
  const float* kp1;   // train image positions
  const float* kp2;   // query image positions
  int nq, off;        // codes of the pair at code[off .. off + nq)
  int off_good, off_all;
};

// One workgroup per pair: the loop of fine_matching_graph.cc:116-133 on the codes - matches_good / matches_all and their
// point lists in query order - written at the pair's offsets.
__global__ __launch_bounds__(256) void k_gather_sets(const PairSrc* __restrict__ src, const int32_t* __restrict__ code,
                                                      int* __restrict__ m_good, float* __restrict__ g1, float* __restrict__ g2,
                                                      int* __restrict__ m_all, float* __restrict__ a1, float* __restrict__ a2,
                                                      int* __restrict__ pair_of_all) {
  __shared__ int wt[4];
  const PairSrc S = src[blockIdx.x];
  int ng = 0, na = 0;
  for (int m0 = 0; m0 < S.nq; m0 += 256) {
    const int m = m0 + threadIdx.x;
    const int32_t c = m < S.nq ? code[S.off + m] : -1;
    const bool any = c >= 0;
    const bool good = any && (c & MSFM_MATCH_GOOD) != 0, all = any && (c & MSFM_MATCH_NOT_ALL) == 0;
    const int id = c & MSFM_MATCH_ID_MASK;
    float x1 = 0.f, y1 = 0.f, x2 = 0.f, y2 = 0.f;
    if (any) { x1 = S.kp1[2 * id]; y1 = S.kp1[2 * id + 1]; x2 = S.kp2[2 * m]; y2 = S.kp2[2 * m + 1]; }
    int tot;
    const int rg = wg_rank<4>(good, wt, tot);
    if (good) {
      const size_t e = (size_t)S.off_good + ng + rg;
      m_good[2 * e] = id; m_good[2 * e + 1] = m;
      g1[2 * e] = x1; g1[2 * e + 1] = y1; g2[2 * e] = x2; g2[2 * e + 1] = y2;
    }
    ng += tot;
    const int ra = wg_rank<4>(all, wt, tot);
    if (all) {
      const size_t e = (size_t)S.off_all + na + ra;
      m_all[2 * e] = id; m_all[2 * e + 1] = m;
      a1[2 * e] = x1; a1[2 * e + 1] = y1; a2[2 * e] = x2; a2[2 * e + 1] = y2;
      pair_of_all[e] = blockIdx.x;
    }
    na += tot;
  }
}

// One workgroup per pair of a SLAM-form result (slam_gps.cc:503-519): every code >= 0 is a survivor of the three checks and its
// code the bare train index; (id, m) and the two cv::Point2f go to the pair's offset in query order.  One set, no pair_of
// array: the RANSAC that follows walks the set by offsets.  off_all + cap bounds the pair's rows (cap = the n_all the chain read
// at create time): a result whose codes were recomputed since then cannot write past them.
__global__ __launch_bounds__(256) void k_gather_slam(const PairSrc* __restrict__ src, const int* __restrict__ off_all, const int32_t* __restrict__ code,
                                                      int* __restrict__ m_all, float* __restrict__ a1, float* __restrict__ a2) {
  __shared__ int wt[4];
  const PairSrc S = src[blockIdx.x];
  const int cap = off_all[blockIdx.x + 1] - S.off_all;
  int na = 0;
  for (int m0 = 0; m0 < S.nq; m0 += 256) {
    const int m = m0 + threadIdx.x;
    const int32_t c = m < S.nq ? code[S.off + m] : -1;
    const bool any = c >= 0;
    int tot;
    const int ra = wg_rank<4>(any, wt, tot);
    if (any && na + ra < cap) {
      const int id = c & MSFM_MATCH_ID_MASK;
      const size_t e = (size_t)S.off_all + na + ra;
      m_all[2 * e] = id; m_all[2 * e + 1] = m;
      a1[2 * e] = S.kp1[2 * id]; a1[2 * e + 1] = S.kp1[2 * id + 1]; a2[2 * e] = S.kp2[2 * m]; a2[2 * e + 1] = S.kp2[2 * m + 1];
    }
    na += tot;
  }
}

// inliers of the "all" set per pair (zero for a pair whose RANSAC failed: its mask is all zero)
__global__ __launch_bounds__(256) void k_count_inliers(const int* __restrict__ off_all, const uint8_t* __restrict__ in_all, int* __restrict__ n_fin) {
  __shared__ int wt[4];
  const int b = off_all[blockIdx.x], e = off_all[blockIdx.x + 1];
  int n = 0;
  for (int i0 = b; i0 < e; i0 += 256) {
    const int i = i0 + threadIdx.x;
    int tot;
    (void)wg_rank<4>(i < e && in_all[i] != 0, wt, tot);
    n += tot;
  }
  if (threadIdx.x == 0) n_fin[blockIdx.x] = n;
}

// matches_inliers of every pair (fine_matching_graph.cc:150-153), in the order of matches_all
__global__ __launch_bounds__(256) void k_compact_matches(const int* __restrict__ off_all, const int* __restrict__ off_fin, const uint8_t* __restrict__ in_all,
                                                          const int* __restrict__ m_all, int* __restrict__ m_fin) {
  __shared__ int wt[4];
  const int b = off_all[blockIdx.x], e = off_all[blockIdx.x + 1];
  int n = 0;
  for (int i0 = b; i0 < e; i0 += 256) {
    const int i = i0 + threadIdx.x;
    const bool f = i < e && in_all[i] != 0;
    int tot;
    const int r = wg_rank<4>(f, wt, tot);
    if (f) {
      const size_t o = (size_t)off_fin[blockIdx.x] + n + r;
      m_fin[2 * o] = m_all[2 * (size_t)i]; m_fin[2 * o + 1] = m_all[2 * (size_t)i + 1];
    }
    n += tot;
  }
}

// positions of a track's observations as doubles (structure.h:65-66 keeps them as Eigen::Vector2d), from the resident keypoints
__global__ __launch_bounds__(256) void k_track_xy(int n_obs, const int* __restrict__ img, const int* __restrict__ feat, const float* const* __restrict__ kp,
                                                   double* __restrict__ xy) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= n_obs) return;
  const float* k = kp[img[e]];
  xy[2 * (size_t)e] = (double)k[2 * (size_t)feat[e]];
  xy[2 * (size_t)e + 1] = (double)k[2 * (size_t)feat[e] + 1];
}

// a track becomes a point of the bundle adjustment when its triangulation was accepted and it has min_views observations
__global__ __launch_bounds__(256) void k_keep(int n_tracks, const int* __restrict__ off, const uint8_t* __restrict__ ok, int min_views, int* __restrict__ keep,
                                               int* __restrict__ keep_obs) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t > n_tracks) return;
  if (t == n_tracks) { keep[t] = 0; keep_obs[t] = 0; return; }
  const int k = off[t + 1] - off[t];
  const int f = ok[t] && k >= min_views;
  keep[t] = f;
  keep_obs[t] = f ? k : 0;
}

// the flat problem arrays of optimizer.cc:59-129 for the kept tracks: points ascending, a point's observations in ascending
// image order (std::map), weight 1.0 for two views and `weight_ge3` for more (:69-78)
__global__ __launch_bounds__(256) void k_ba_arrays(int n_tracks, const int* __restrict__ off, const int* __restrict__ img, const double* __restrict__ xy,
                                                    const double* __restrict__ X, const int* __restrict__ keep, const int* __restrict__ new_pt,
                                                    const int* __restrict__ new_obs, double weight_ge3, int* __restrict__ obs_cam,
                                                    int* __restrict__ obs_pt, double* __restrict__ obs_xy, double* __restrict__ point,
                                                    double* __restrict__ pt_weight, int* __restrict__ track_of_point) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= n_tracks || !keep[t]) return;
  const int p = new_pt[t], o0 = new_obs[t], b = off[t], k = off[t + 1] - b;
  point[3 * (size_t)p] = X[3 * (size_t)t]; point[3 * (size_t)p + 1] = X[3 * (size_t)t + 1]; point[3 * (size_t)p + 2] = X[3 * (size_t)t + 2];
  pt_weight[p] = k == 2 ? 1.0 : weight_ge3;
  track_of_point[p] = t;
  for (int j = 0; j < k; j++) {
    obs_cam[o0 + j] = img[b + j];
    obs_pt[o0 + j] = p;
    obs_xy[2 * (size_t)(o0 + j)] = xy[2 * (size_t)(b + j)];
    obs_xy[2 * (size_t)(o0 + j) + 1] = xy[2 * (size_t)(b + j) + 1];
  }
}

}  // namespace chn

struct msfm_chain {
  msfm_ctx* ctx = nullptr;
  int n_images = 0, n_pairs = 0;
  std::vector<int> pairs, count, feat_off;
  // The chain keeps its OWN copy of the keypoints (one flat buffer, kp[i] points into it): the descriptor set may re-upload
  // or drop them, or be destroyed, while the chain lives (verify and triangulate read them long after create).
  DevBuf<float> kp_own;
  std::vector<const float*> kp;
  DevBuf<const float*> d_kp;
  // verification
  bool slam = false;                     // made from a msfm_match_pairs_slam result: msfm_chain_verify_slam, not msfm_chain_verify
  const msfm_match_result* src = nullptr;   // the result the chain was made from (compared, never read through)
  bool verified = false;
  std::vector<int> n_good, n_all;        // sizes of matches_good / matches_all per pair (read back once at create time);
                                         // SLAM form: n_all = survivors of the three checks, n_good is not used
  std::vector<int> n_fin, off_fin;       // matches_inliers per pair and their prefix sums
  std::vector<uint8_t> ok;
  std::vector<double> F;
  DevBuf<int> d_pair, d_moff, d_match, d_nf, d_fo;
  // tracks
  bool have_tracks = false;
  msfm_track_dev tracks;
  // triangulation
  bool triangulated = false;
  DevBuf<double> xy, X, mse;
  DevBuf<uint8_t> tok;
  // bundle adjustment
  int n_ba_points = 0, n_ba_obs = 0;
  DevBuf<int> track_of_point;
  const msfm_ba* last_ba = nullptr;      // the problem track_of_point belongs to (msfm_chain_store_points takes no other)
  // GetAccuracy (gpsreg.hip)
  bool have_accuracy = false;
  DevBuf<double> e_avg, e_mse;
  DevBuf<int> n_used;
};

#define CH_TRY(e) HIP_TRY(ctx, (e))

MSFM_API int msfm_chain_create(msfm_match_result* res, msfm_chain** out) {
  if (!res || !out) return MSFM_E_INVAL;
  *out = nullptr;
  MatchView v;
  MSFM_TRY(match_result_view(res, &v));
  msfm_ctx* ctx = v.ctx;
  for (int p = 0; p < v.n_pairs; p++) {
    const int a = v.pairs[2 * p], b = v.pairs[2 * p + 1];
    if (!v.kp[a] || (v.count[b] > 0 && !v.kp[b]))
      return msfm_set_error(ctx, MSFM_E_INVAL, "msfm_chain_create: pair %d needs the keypoints of both images (msfm_descset_upload_keypoints)", p);
  }
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  Child<msfm_chain> C = child_new<msfm_chain>(ctx);
  C->n_images = v.n_images; C->n_pairs = v.n_pairs;
  C->slam = v.slam; C->src = res;
  C->pairs.assign(v.pairs, v.pairs + 2 * (size_t)v.n_pairs);
  C->count = v.count;
  C->feat_off.assign(v.n_images + 1, 0);
  for (int i = 0; i < v.n_images; i++) C->feat_off[i + 1] = C->feat_off[i] + v.count[i];
  hipStream_t s = ctx->stream;
  DevScope sc(ctx);
  C->kp.assign(v.n_images, nullptr);
  CH_TRY(C->kp_own.alloc(2 * (size_t)std::max(1, C->feat_off[v.n_images])));
  for (int i = 0; i < v.n_images; i++) {
    if (!v.kp[i] || v.count[i] == 0) continue;
    float* dst = C->kp_own.p + 2 * (size_t)C->feat_off[i];
    CH_TRY(hipMemcpyAsync(dst, v.kp[i], sizeof(float) * 2 * (size_t)v.count[i], hipMemcpyDeviceToDevice, s));
    C->kp[i] = dst;
  }
  // ---- matches_good / matches_all of every pair, gathered from the codes ----
  std::vector<int> ng(std::max(1, v.n_pairs)), na(std::max(1, v.n_pairs));
  if (v.n_pairs) {
    CH_TRY(hipMemcpyAsync(ng.data(), v.n_good, sizeof(int) * v.n_pairs, hipMemcpyDeviceToHost, s));
    CH_TRY(hipMemcpyAsync(na.data(), v.n_all, sizeof(int) * v.n_pairs, hipMemcpyDeviceToHost, s));
    CH_TRY(hipStreamSynchronize(s));
  }
  C->n_good = ng; C->n_all = na;   // sizes of matches_good / matches_all per pair: msfm_chain_verify gathers them
  *out = C.release();
  sc.dismiss();   // the chain keeps its block (with pairs: behind the wait above)
  return MSFM_OK;
}

MSFM_API int msfm_chain_verify(msfm_chain* C, msfm_match_result* res, const msfm_fransac_options* opt, double th_filter) {
  if (!C || !res || !opt) return MSFM_E_INVAL;
  msfm_ctx* ctx = C->ctx;
  if (C->slam) return msfm_set_error(ctx, MSFM_E_INVAL, "msfm_chain_verify: the chain was made from a msfm_match_pairs_slam result (msfm_chain_verify_slam)");
  if (C->verified) return msfm_set_error(ctx, MSFM_E_INVAL, "msfm_chain_verify: already done");
  if (opt->max_iterations < 1 || opt->max_iterations > 65536 || !(opt->threshold > 0.0)) return msfm_set_error(ctx, MSFM_E_INVAL, "fransac: bad options");
  MatchView v;
  MSFM_TRY(match_result_view(res, &v));
  if (v.ctx != ctx || v.n_pairs != C->n_pairs) return msfm_set_error(ctx, MSFM_E_INVAL, "msfm_chain_verify: not the match result the chain was created from");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  const int np = C->n_pairs;
  C->ok.assign(std::max(1, np), 0);
  C->F.assign(9 * (size_t)std::max(1, np), 0.0);
  std::vector<int> off_g(np + 1, 0), off_a(np + 1, 0);
  for (int p = 0; p < np; p++) { off_g[p + 1] = off_g[p] + C->n_good[p]; off_a[p + 1] = off_a[p] + C->n_all[p]; }
  const int tg = off_g[np], ta = off_a[np];
  std::vector<chn::PairSrc> src(std::max(1, np));
  for (int p = 0; p < np; p++) {
    const int a = C->pairs[2 * p], b = C->pairs[2 * p + 1];
    src[p] = chn::PairSrc{C->kp[a], v.nq[p] ? C->kp[b] : nullptr, v.nq[p], v.out_off[p], off_g[p], off_a[p]};
  }
  DevBuf<chn::PairSrc> d_src;
  DevBuf<int> d_offg, d_offa, m_good, m_all, pair_of_all, d_nin, d_nfin, d_offfin;
  DevBuf<float> g1, g2, a1, a2;
  DevBuf<double> dF;
  DevBuf<uint8_t> in_g, in_a, d_ok;
  DevScope sc(ctx);
  CH_TRY(d_src.from(src, s)); CH_TRY(d_offg.from(off_g, s)); CH_TRY(d_offa.from(off_a, s));
  CH_TRY(m_good.alloc(2 * (size_t)std::max(1, tg))); CH_TRY(g1.alloc(2 * (size_t)std::max(1, tg))); CH_TRY(g2.alloc(2 * (size_t)std::max(1, tg)));
  CH_TRY(m_all.alloc(2 * (size_t)std::max(1, ta))); CH_TRY(a1.alloc(2 * (size_t)std::max(1, ta))); CH_TRY(a2.alloc(2 * (size_t)std::max(1, ta)));
  CH_TRY(pair_of_all.alloc(std::max(1, ta)));
  CH_TRY(dF.alloc(9 * (size_t)std::max(1, np))); CH_TRY(in_g.alloc(std::max(1, tg))); CH_TRY(in_a.alloc(std::max(1, ta)));
  CH_TRY(d_nin.alloc(std::max(1, np))); CH_TRY(d_ok.alloc(std::max(1, np))); CH_TRY(d_nfin.alloc(std::max(1, np)));
  C->n_fin.assign(std::max(1, np), 0);
  C->off_fin.assign(np + 1, 0);
  if (np) {
    {
      KTimer t(ctx, "chain_gather_sets");
      hipLaunchKernelGGL(chn::k_gather_sets, dim3(np), dim3(256), 0, s, d_src.p, v.code, m_good.p, g1.p, g2.p, m_all.p, a1.p, a2.p, pair_of_all.p);
    }
    CH_TRY(hipGetLastError());
    // GeoVerificationFundamental on the good sets (fine_matching_graph.cc:141), then the closed-form filter on the all sets of
    // the pairs that passed (:145-147)
    MSFM_TRY(geo_fransac_dev(ctx, np, off_g.data(), d_offg.p, g1.p, g2.p, opt, dF.p, in_g.p, d_nin.p, d_ok.p));
    CH_TRY(hipMemsetAsync(in_a.p, 0, std::max(1, ta), s));
    MSFM_TRY(geo_epipolar_batch_dev(ctx, ta, pair_of_all.p, a1.p, a2.p, dF.p, d_ok.p, th_filter, in_a.p));
    {
      KTimer t(ctx, "chain_compact_matches");
      hipLaunchKernelGGL(chn::k_count_inliers, dim3(np), dim3(256), 0, s, d_offa.p, in_a.p, d_nfin.p);
    }
    CH_TRY(hipMemcpyAsync(C->n_fin.data(), d_nfin.p, sizeof(int) * np, hipMemcpyDeviceToHost, s));
    CH_TRY(hipMemcpyAsync(C->ok.data(), d_ok.p, np, hipMemcpyDeviceToHost, s));
    CH_TRY(hipMemcpyAsync(C->F.data(), dF.p, sizeof(double) * 9 * (size_t)np, hipMemcpyDeviceToHost, s));
    CH_TRY(hipStreamSynchronize(s));
    for (int p = 0; p < np; p++) C->off_fin[p + 1] = C->off_fin[p] + C->n_fin[p];
  }
  const int M = C->off_fin[np];
  CH_TRY(C->d_moff.from(C->off_fin, s));
  CH_TRY(C->d_match.alloc(2 * (size_t)std::max(1, M)));
  CH_TRY(C->d_pair.from(C->pairs.empty() ? std::vector<int>(2, 0) : C->pairs, s));
  CH_TRY(C->d_nf.from(C->count, s));
  CH_TRY(C->d_fo.from(C->feat_off, s));
  if (np) {
    KTimer t(ctx, "chain_compact_matches");
    hipLaunchKernelGGL(chn::k_compact_matches, dim3(np), dim3(256), 0, s, d_offa.p, C->d_moff.p, in_a.p, m_all.p, C->d_match.p);
  }
  CH_TRY(hipGetLastError());
  CH_TRY(sc.finish());   // the scratch above goes back to the pool
  C->verified = true;
  return MSFM_OK;
}

// The tail of SLAMGPS::FeatureMatching step 2 (slam_gps.cc:503-541) for every pair of a SLAM-form result: the conventions are in
// the header comment of this file.
MSFM_API int msfm_chain_verify_slam(msfm_chain* C, msfm_match_result* res, const msfm_fransac_options* opt) {
  if (!C || !res || !opt) return MSFM_E_INVAL;
  msfm_ctx* ctx = C->ctx;
  if (!C->slam) return msfm_set_error(ctx, MSFM_E_INVAL, "msfm_chain_verify_slam: the chain was made from a msfm_match_pairs result (msfm_chain_verify)");
  if (C->verified) return msfm_set_error(ctx, MSFM_E_INVAL, "msfm_chain_verify_slam: already done");
  if (opt->max_iterations < 1 || opt->max_iterations > 65536 || !(opt->threshold > 0.0)) return msfm_set_error(ctx, MSFM_E_INVAL, "fransac: bad options");
  if (res != C->src) return msfm_set_error(ctx, MSFM_E_INVAL, "msfm_chain_verify_slam: not the match result the chain was created from");
  MatchView v;
  MSFM_TRY(match_result_view(res, &v));
  if (v.ctx != ctx || v.n_pairs != C->n_pairs || !v.slam)
    return msfm_set_error(ctx, MSFM_E_INVAL, "msfm_chain_verify_slam: not the match result the chain was created from");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  const int np = C->n_pairs;
  std::vector<int> off_a(np + 1, 0);
  for (int p = 0; p < np; p++) off_a[p + 1] = off_a[p] + C->n_all[p];
  const int ta = off_a[np];
  std::vector<chn::PairSrc> src(std::max(1, np));
  for (int p = 0; p < np; p++) {
    const int a = C->pairs[2 * p], b = C->pairs[2 * p + 1];
    src[p] = chn::PairSrc{C->kp[a], v.nq[p] ? C->kp[b] : nullptr, v.nq[p], v.out_off[p], 0, off_a[p]};
  }
  DevBuf<chn::PairSrc> d_src;
  DevBuf<int> d_offa, m_all, d_nin;
  DevBuf<float> a1, a2;
  DevBuf<double> dF;
  DevBuf<uint8_t> in_a, d_ok;
  DevScope sc(ctx);
  CH_TRY(d_src.from(src, s)); CH_TRY(d_offa.from(off_a, s));
  CH_TRY(m_all.alloc(2 * (size_t)std::max(1, ta))); CH_TRY(a1.alloc(2 * (size_t)std::max(1, ta))); CH_TRY(a2.alloc(2 * (size_t)std::max(1, ta)));
  CH_TRY(dF.alloc(9 * (size_t)std::max(1, np))); CH_TRY(in_a.alloc(std::max(1, ta)));
  CH_TRY(d_nin.alloc(std::max(1, np))); CH_TRY(d_ok.alloc(std::max(1, np)));
  std::vector<int> n_fin(std::max(1, np), 0), off_fin(np + 1, 0);
  std::vector<uint8_t> ok(std::max(1, np), 0);
  std::vector<double> F(9 * (size_t)std::max(1, np), 0.0);
  if (np) {
    {
      KTimer t(ctx, "chain_gather_slam");
      hipLaunchKernelGGL(chn::k_gather_slam, dim3(np), dim3(256), 0, s, d_src.p, d_offa.p, v.code, m_all.p, a1.p, a2.p);
    }
    CH_TRY(hipGetLastError());
    // GeoVerificationFundamental on all survivors (slam_gps.cc:521); the mask and n_inliers of a pair whose verdict is 0 stay
    // as the RANSAC left them, which is what :524-529 keeps
    MSFM_TRY(geo_fransac_dev(ctx, np, off_a.data(), d_offa.p, a1.p, a2.p, opt, dF.p, in_a.p, d_nin.p, d_ok.p));
    CH_TRY(sc.down(n_fin.data(), d_nin.p, (size_t)np));
    CH_TRY(sc.down(ok.data(), d_ok.p, (size_t)np));
    CH_TRY(sc.down(F.data(), dF.p, 9 * (size_t)np));
    CH_TRY(hipStreamSynchronize(s));
    for (int p = 0; p < np; p++) off_fin[p + 1] = off_fin[p] + n_fin[p];
  }
  C->n_fin.swap(n_fin); C->off_fin.swap(off_fin); C->ok.swap(ok); C->F.swap(F);
  const int M = C->off_fin[np];
  CH_TRY(C->d_moff.from(C->off_fin, s));
  CH_TRY(C->d_match.alloc(2 * (size_t)std::max(1, M)));
  CH_TRY(C->d_pair.from(C->pairs.empty() ? std::vector<int>(2, 0) : C->pairs, s));
  CH_TRY(C->d_nf.from(C->count, s));
  CH_TRY(C->d_fo.from(C->feat_off, s));
  if (np) {
    KTimer t(ctx, "chain_compact_matches");
    hipLaunchKernelGGL(chn::k_compact_matches, dim3(np), dim3(256), 0, s, d_offa.p, C->d_moff.p, in_a.p, m_all.p, C->d_match.p);
  }
  CH_TRY(hipGetLastError());
  CH_TRY(sc.finish());   // the scratch above goes back to the pool
  C->verified = true;
  return MSFM_OK;
}

MSFM_API int msfm_chain_matches(msfm_chain* C, int* n_matches, uint8_t* ok, double* F) {
  if (!C) return MSFM_E_INVAL;
  if (!C->verified) return msfm_set_error(C->ctx, MSFM_E_INVAL, "msfm_chain_matches: msfm_chain_verify first");
  for (int p = 0; p < C->n_pairs; p++) {
    if (n_matches) n_matches[p] = C->n_fin[p];
    if (ok) ok[p] = C->ok[p];
    if (F) for (int k = 0; k < 9; k++) F[9 * (size_t)p + k] = C->F[9 * (size_t)p + k];
  }
  return MSFM_OK;
}

int chain_match_view(msfm_chain* C, ChainMatchView* out) {
  if (!C->verified) return msfm_set_error(C->ctx, MSFM_E_INVAL, "msfm_match_store_from_chain: msfm_chain_verify first");
  *out = ChainMatchView{C->ctx, C->n_images, C->n_pairs, C->pairs.data(), C->count.data(), C->off_fin.data(), C->d_match.p, C->kp_own.p, C->kp};
  return MSFM_OK;
}

MSFM_API int msfm_chain_fetch_matches(msfm_chain* C, int pair, int* matches) {
  if (!C || pair < 0 || pair >= C->n_pairs) return MSFM_E_INVAL;
  msfm_ctx* ctx = C->ctx;
  if (!C->verified) return msfm_set_error(ctx, MSFM_E_INVAL, "msfm_chain_fetch_matches: msfm_chain_verify first");
  const int n = C->n_fin[pair];
  if (n == 0) return MSFM_OK;
  if (!matches) return MSFM_E_INVAL;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  CH_TRY(hipMemcpyAsync(matches, C->d_match.p + 2 * (size_t)C->off_fin[pair], sizeof(int) * 2 * (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
  CH_TRY(hipStreamSynchronize(ctx->stream));
  return MSFM_OK;
}

MSFM_API int msfm_chain_build_tracks(msfm_chain* C, int* n_tracks, int* n_observations) {
  if (!C) return MSFM_E_INVAL;
  msfm_ctx* ctx = C->ctx;
  if (!C->verified) return msfm_set_error(ctx, MSFM_E_INVAL, "msfm_chain_build_tracks: msfm_chain_verify first");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  if (!C->have_tracks) {
    if ((long)C->feat_off[C->n_images] > 0x7fffffffL) return msfm_set_error(ctx, MSFM_E_INVAL, "more than 2^31 features");
    MSFM_TRY(tracks_build_dev(ctx, C->n_images, C->feat_off, C->d_nf.p, C->d_fo.p, C->n_pairs, C->d_pair.p, C->d_moff.p, C->d_match.p,
                              C->off_fin[C->n_pairs], &C->tracks));
    C->have_tracks = true;
  }
  if (n_tracks) *n_tracks = C->tracks.n_tracks;
  if (n_observations) *n_observations = C->tracks.n_obs;
  return MSFM_OK;
}

MSFM_API int msfm_chain_fetch_tracks(msfm_chain* C, int* track_off, int* obs_image, int* obs_feature) {
  if (!C) return MSFM_E_INVAL;
  msfm_ctx* ctx = C->ctx;
  if (!C->have_tracks) return msfm_set_error(ctx, MSFM_E_INVAL, "msfm_chain_fetch_tracks: msfm_chain_build_tracks first");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  const msfm_track_dev& T = C->tracks;
  if (track_off) CH_TRY(hipMemcpyAsync(track_off, T.off.p, sizeof(int) * ((size_t)T.n_tracks + 1), hipMemcpyDeviceToHost, s));
  if (obs_image && T.n_obs) CH_TRY(hipMemcpyAsync(obs_image, T.img.p, sizeof(int) * (size_t)T.n_obs, hipMemcpyDeviceToHost, s));
  if (obs_feature && T.n_obs) CH_TRY(hipMemcpyAsync(obs_feature, T.feat.p, sizeof(int) * (size_t)T.n_obs, hipMemcpyDeviceToHost, s));
  CH_TRY(hipStreamSynchronize(s));
  return MSFM_OK;
}

MSFM_API int msfm_chain_triangulate(msfm_chain* C, int n_cams, const double* cam_R, const double* cam_t, const double* cam_c, const double* cam_fk,
                                    double th_error, double th_angle, int* n_accepted) {
  if (!C || !cam_R || !cam_t || !cam_c || !cam_fk) return MSFM_E_INVAL;
  msfm_ctx* ctx = C->ctx;
  if (!C->have_tracks) return msfm_set_error(ctx, MSFM_E_INVAL, "msfm_chain_triangulate: msfm_chain_build_tracks first");
  if (n_cams < C->n_images) return msfm_set_error(ctx, MSFM_E_INVAL, "msfm_chain_triangulate: %d cameras for %d images (image index = camera index)", n_cams, C->n_images);
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  const msfm_track_dev& T = C->tracks;
  const int nt = T.n_tracks, no = T.n_obs;
  DevBuf<double> dR, dt, dc, dfk;
  DevScope sc(ctx);
  CH_TRY(sc.up(dR, cam_R, 9 * (size_t)n_cams)); CH_TRY(sc.up(dt, cam_t, 3 * (size_t)n_cams));
  CH_TRY(sc.up(dc, cam_c, 3 * (size_t)n_cams)); CH_TRY(sc.up(dfk, cam_fk, 3 * (size_t)n_cams));
  CH_TRY(C->d_kp.from(C->kp, s));
  CH_TRY(C->xy.alloc(2 * (size_t)std::max(1, no)));
  CH_TRY(C->X.alloc(3 * (size_t)std::max(1, nt))); CH_TRY(C->mse.alloc(std::max(1, nt))); CH_TRY(C->tok.alloc(std::max(1, nt)));
  CH_TRY(hipMemsetAsync(C->X.p, 0, sizeof(double) * 3 * (size_t)std::max(1, nt), s));   // X is in / out: zeros where the 4x4 LLT fails
  if (no) hipLaunchKernelGGL(chn::k_track_xy, dim3(cdiv(no, 256)), dim3(256), 0, s, no, T.img.p, T.feat.p, C->d_kp.p, C->xy.p);
  const TrackPtrs P{nt, T.off.p, T.img.p, C->xy.p, dR.p, dt.p, dc.p, dfk.p};
  MSFM_TRY(tri_midpoint_dev(ctx, P, th_error, th_angle, C->X.p, C->mse.p, C->tok.p));
  CH_TRY(hipGetLastError());
  if (n_accepted) {
    std::vector<uint8_t> okh(std::max(1, nt));
    if (nt) CH_TRY(hipMemcpyAsync(okh.data(), C->tok.p, nt, hipMemcpyDeviceToHost, s));
    CH_TRY(sc.finish());
    int n = 0;
    for (int t = 0; t < nt; t++) n += okh[t] != 0;
    *n_accepted = n;
  } else {
    CH_TRY(sc.finish());   // the camera arrays above are released on return
  }
  C->triangulated = true;
  return MSFM_OK;
}

MSFM_API int msfm_chain_fetch_points(msfm_chain* C, double* X, double* mse, uint8_t* ok) {
  if (!C) return MSFM_E_INVAL;
  msfm_ctx* ctx = C->ctx;
  if (!C->triangulated) return msfm_set_error(ctx, MSFM_E_INVAL, "msfm_chain_fetch_points: msfm_chain_triangulate first");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  const int nt = C->tracks.n_tracks;
  if (nt) {
    if (X) CH_TRY(hipMemcpyAsync(X, C->X.p, sizeof(double) * 3 * (size_t)nt, hipMemcpyDeviceToHost, s));
    if (mse) CH_TRY(hipMemcpyAsync(mse, C->mse.p, sizeof(double) * (size_t)nt, hipMemcpyDeviceToHost, s));
    if (ok) CH_TRY(hipMemcpyAsync(ok, C->tok.p, (size_t)nt, hipMemcpyDeviceToHost, s));
  }
  CH_TRY(hipStreamSynchronize(s));
  return MSFM_OK;
}

// msfm_chain_ba_create (gps_xyz == nullptr: no GPS rows) and msfm_chain_ba_create_gps
static int chain_ba_create(msfm_chain* C, int n_cams, int n_models, double* cam_pose, double* cam_model, const int32_t* cam_model_of_cam, int min_views,
                           double weight_ge3, const double* gps_xyz, double gps_weight, double* gps_weight_used, msfm_ba** out, int* n_points,
                           int* n_observations) {
  if (!C || !out || !cam_pose || !cam_model || !cam_model_of_cam) return MSFM_E_INVAL;
  msfm_ctx* ctx = C->ctx;
  *out = nullptr;
  if (!C->triangulated) return msfm_set_error(ctx, MSFM_E_INVAL, "msfm_chain_ba_create: msfm_chain_triangulate first");
  if (n_cams < C->n_images) return msfm_set_error(ctx, MSFM_E_INVAL, "msfm_chain_ba_create: %d cameras for %d images", n_cams, C->n_images);
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  const msfm_track_dev& T = C->tracks;
  const int nt = T.n_tracks;
  DevBuf<int> keep, keep_obs, new_pt, new_obs, obs_cam, obs_pt;
  DevBuf<double> obs_xy, point, ptw;
  PrimTmp tmp;
  DevScope sc(ctx);
  CH_TRY(keep.alloc((size_t)nt + 1)); CH_TRY(keep_obs.alloc((size_t)nt + 1)); CH_TRY(new_pt.alloc((size_t)nt + 1)); CH_TRY(new_obs.alloc((size_t)nt + 1));
  hipLaunchKernelGGL(chn::k_keep, dim3(cdiv(nt + 1, 256)), dim3(256), 0, s, nt, T.off.p, C->tok.p, min_views, keep.p, keep_obs.p);
  CH_TRY(prim_scan_excl(tmp, keep.p, new_pt.p, (size_t)nt + 1, s));
  CH_TRY(prim_scan_excl(tmp, keep_obs.p, new_obs.p, (size_t)nt + 1, s));
  int np = 0, no = 0;
  CH_TRY(hipMemcpyAsync(&np, new_pt.p + nt, sizeof(int), hipMemcpyDeviceToHost, s));
  CH_TRY(hipMemcpyAsync(&no, new_obs.p + nt, sizeof(int), hipMemcpyDeviceToHost, s));
  CH_TRY(hipStreamSynchronize(s));
  if (np == 0) return msfm_set_error(ctx, MSFM_E_INVAL, "msfm_chain_ba_create: no track qualifies (%d tracks)", nt);
  CH_TRY(obs_cam.alloc(no)); CH_TRY(obs_pt.alloc(no)); CH_TRY(obs_xy.alloc(2 * (size_t)no)); CH_TRY(point.alloc(3 * (size_t)np)); CH_TRY(ptw.alloc(np));
  CH_TRY(C->track_of_point.alloc(np));
  hipLaunchKernelGGL(chn::k_ba_arrays, dim3(cdiv(nt, 256)), dim3(256), 0, s, nt, T.off.p, T.img.p, C->xy.p, C->X.p, keep.p, new_pt.p, new_obs.p, weight_ge3,
                     obs_cam.p, obs_pt.p, obs_xy.p, point.p, ptw.p, C->track_of_point.p);
  CH_TRY(hipGetLastError());
  msfm_ba_problem P;
  memset(&P, 0, sizeof P);
  P.n_cams = n_cams; P.n_models = n_models; P.n_points = np; P.n_obs = no;
  P.cam_pose = cam_pose; P.cam_model = cam_model; P.cam_model_of_cam = cam_model_of_cam;
  P.point = point.p; P.obs_cam = obs_cam.p; P.obs_pt = obs_pt.p; P.obs_xy = obs_xy.p; P.pt_weight = ptw.p;
  if (gps_xyz) {   // the GPS rows of FullBundleAdjustment, slam_gps.cc:818-830; the weight of :824 is an integer division
    P.gps_xyz = gps_xyz;
    P.gps_weight = gps_weight > 0.0 ? gps_weight : (double)(no / n_cams);
    if (gps_weight_used) *gps_weight_used = P.gps_weight;
  }
  C->last_ba = nullptr;   // (track_of_point has been rewritten)
  MSFM_TRY(ba_create_impl(ctx, &P, /*bulk_on_device=*/true, out));
  CH_TRY(sc.finish());
  C->n_ba_points = np; C->n_ba_obs = no;
  C->last_ba = *out;
  if (n_points) *n_points = np;
  if (n_observations) *n_observations = no;
  return MSFM_OK;
}

MSFM_API int msfm_chain_ba_create(msfm_chain* C, int n_cams, int n_models, double* cam_pose, double* cam_model, const int32_t* cam_model_of_cam,
                                  int min_views, double weight_ge3, msfm_ba** out, int* n_points, int* n_observations) {
  return chain_ba_create(C, n_cams, n_models, cam_pose, cam_model, cam_model_of_cam, min_views, weight_ge3, nullptr, 0.0, nullptr, out, n_points,
                         n_observations);
}

MSFM_API int msfm_chain_ba_create_gps(msfm_chain* C, int n_cams, int n_models, double* cam_pose, double* cam_model, const int32_t* cam_model_of_cam,
                                      int min_views, double weight_ge3, const double* gps_xyz, double gps_weight, double* gps_weight_used,
                                      msfm_ba** out, int* n_points, int* n_observations) {
  if (!C) return MSFM_E_INVAL;
  if (!gps_xyz || !(gps_weight == gps_weight)) return msfm_set_error(C->ctx, MSFM_E_INVAL, "msfm_chain_ba_create_gps: gps_xyz is null or gps_weight NaN");
  return chain_ba_create(C, n_cams, n_models, cam_pose, cam_model, cam_model_of_cam, min_views, weight_ge3, gps_xyz, gps_weight, gps_weight_used, out,
                         n_points, n_observations);
}

// ---- the SLAM + GPS registration steps on the resident tracks / xy / X / tok (kernels: gpsreg.hip) ----
MSFM_API int msfm_chain_accuracy(msfm_chain* C, int n_cams, const double* cam_R, const double* cam_t, const double* cam_fk, const double* cam_dc,
                                 int min_views, double th_outlier, int* n_outliers, int* n_inliers) {
  if (!C || !cam_R || !cam_t || !cam_fk) return MSFM_E_INVAL;
  msfm_ctx* ctx = C->ctx;
  if (!C->triangulated) return msfm_set_error(ctx, MSFM_E_INVAL, "msfm_chain_accuracy: msfm_chain_triangulate first");
  if (n_cams < C->n_images) return msfm_set_error(ctx, MSFM_E_INVAL, "msfm_chain_accuracy: %d cameras for %d images", n_cams, C->n_images);
  if (!(th_outlier == th_outlier)) return msfm_set_error(ctx, MSFM_E_INVAL, "msfm_chain_accuracy: th_outlier is NaN");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  const msfm_track_dev& T = C->tracks;
  const int nt = T.n_tracks;
  DevBuf<double> dR, dt, dfk, ddc;
  DevBuf<int> dcount;
  DevScope sc(ctx);
  CH_TRY(sc.up(dR, cam_R, 9 * (size_t)n_cams)); CH_TRY(sc.up(dt, cam_t, 3 * (size_t)n_cams)); CH_TRY(sc.up(dfk, cam_fk, 3 * (size_t)n_cams));
  if (cam_dc) CH_TRY(sc.up(ddc, cam_dc, 2 * (size_t)n_cams));
  CH_TRY(dcount.alloc(1));
  if (!C->have_accuracy) {
    CH_TRY(C->e_avg.alloc(std::max(1, nt))); CH_TRY(C->e_mse.alloc(std::max(1, nt))); CH_TRY(C->n_used.alloc(std::max(1, nt)));
  }
  const AccuracyPtrs P{nt, T.off.p, T.img.p, C->xy.p, dR.p, dt.p, dfk.p, cam_dc ? ddc.p : nullptr, C->X.p, C->tok.p, min_views, th_outlier,
                       C->e_avg.p, C->e_mse.p, C->n_used.p, C->tok.p};
  MSFM_TRY(gps_accuracy_dev(ctx, P, T.n_obs, dcount.p));
  int outl = 0;
  CH_TRY(sc.down(&outl, dcount.p, 1));
  CH_TRY(sc.finish());
  C->have_accuracy = true;
  if (n_outliers) *n_outliers = outl;
  if (n_inliers) *n_inliers = nt - outl;
  return MSFM_OK;
}

MSFM_API int msfm_chain_fetch_accuracy(msfm_chain* C, double* e_avg, double* e_mse, int32_t* n_used) {
  if (!C) return MSFM_E_INVAL;
  msfm_ctx* ctx = C->ctx;
  if (!C->have_accuracy) return msfm_set_error(ctx, MSFM_E_INVAL, "msfm_chain_fetch_accuracy: msfm_chain_accuracy first");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  const int nt = C->tracks.n_tracks;
  if (nt) {
    if (e_avg) CH_TRY(hipMemcpyAsync(e_avg, C->e_avg.p, sizeof(double) * (size_t)nt, hipMemcpyDeviceToHost, s));
    if (e_mse) CH_TRY(hipMemcpyAsync(e_mse, C->e_mse.p, sizeof(double) * (size_t)nt, hipMemcpyDeviceToHost, s));
    if (n_used) CH_TRY(hipMemcpyAsync(n_used, C->n_used.p, sizeof(int32_t) * (size_t)nt, hipMemcpyDeviceToHost, s));
  }
  CH_TRY(hipStreamSynchronize(s));
  return MSFM_OK;
}

MSFM_API int msfm_chain_gps_register(msfm_chain* C, int n_cams, const double* cam_c, const double* gps) {
  if (!C || !cam_c || !gps) return MSFM_E_INVAL;
  msfm_ctx* ctx = C->ctx;
  if (!C->triangulated) return msfm_set_error(ctx, MSFM_E_INVAL, "msfm_chain_gps_register: msfm_chain_triangulate first");
  if (n_cams < C->n_images) return msfm_set_error(ctx, MSFM_E_INVAL, "msfm_chain_gps_register: %d cameras for %d images", n_cams, C->n_images);
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  const msfm_track_dev& T = C->tracks;
  const std::vector<double> offs = gps_cam_offsets(n_cams, cam_c, gps);
  DevBuf<double> dc, doff;
  DevScope sc(ctx);
  CH_TRY(sc.up(dc, cam_c, 3 * (size_t)n_cams)); CH_TRY(sc.up(doff, offs));
  const RegisterPtrs P{T.n_tracks, T.off.p, T.img.p, C->tok.p, dc.p, doff.p, C->X.p};
  MSFM_TRY(gps_register_dev(ctx, P));
  CH_TRY(sc.finish());
  return MSFM_OK;
}

MSFM_API int msfm_chain_store_points(msfm_chain* C, msfm_ba* ba) {
  if (!C || !ba) return MSFM_E_INVAL;
  msfm_ctx* ctx = C->ctx;
  if (ba != C->last_ba || C->n_ba_points == 0)
    return msfm_set_error(ctx, MSFM_E_INVAL, "msfm_chain_store_points: not the problem this chain made last");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  MSFM_TRY(gps_store_points_dev(ctx, C->n_ba_points, C->track_of_point.p, ba_device_points(ba), C->X.p));
  CH_TRY(hipStreamSynchronize(ctx->stream));
  return MSFM_OK;
}

MSFM_API int msfm_chain_fetch_point_tracks(msfm_chain* C, int* track_of_point) {
  if (!C || !track_of_point) return MSFM_E_INVAL;
  msfm_ctx* ctx = C->ctx;
  if (C->n_ba_points == 0) return msfm_set_error(ctx, MSFM_E_INVAL, "msfm_chain_fetch_point_tracks: msfm_chain_ba_create first");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  CH_TRY(hipMemcpyAsync(track_of_point, C->track_of_point.p, sizeof(int) * (size_t)C->n_ba_points, hipMemcpyDeviceToHost, ctx->stream));
  CH_TRY(hipStreamSynchronize(ctx->stream));
  return MSFM_OK;
}

MSFM_API void msfm_chain_destroy(msfm_chain* C) { msfm_child_destroy(C); }
