// SLAMGPS::FeatureMatching step 1 (SfM/src/slam_gps.cc:323-423) on the GPU: for every camera pair of the SLAM window the
// shared SLAM points, their binary32 observations, findFundamentalMat + findHomography by the batched RANSACs of geo.hip,
// and the two binary32 gates - the prior F / H that msfm_match_pairs_slam (step 2) takes.
//   host    checks the input, sorts the point-major observations by camera (a stable counting sort: each camera's list is
//           ascending in point index and carries the observation index), forms the window slots
//   k_prior_count   one wave per slot: |list(i) n list(j)| by a binary search of each element of list(i) in list(j)
//   k_prior_gather  one wave per candidate (>= th_same_pts shared points): the same walk, the found elements written in
//                   ascending point order (ballot + prefix count) as pts1 / pts2
//   geo_fransac_dev / geo_hransac_dev on those resident buffers (H only where the F gate passed), gates on the host.
// The intersection is never materialised as (pair, point) keys: config 5 has tens of millions of them.
#include "common.h"

#include <cfloat>

#define PRIOR_WAVE 64

// the position of v in the ascending list p[lo, hi), or -1
__device__ static inline int prior_find(const int* __restrict__ p, int lo, int hi, int v) {
  const int end = hi;
  while (lo < hi) {
    const int mid = lo + ((hi - lo) >> 1);
    if (p[mid] < v) lo = mid + 1; else hi = mid;
  }
  return lo < end && p[lo] == v ? lo : -1;
}

__global__ __launch_bounds__(PRIOR_WAVE) void k_prior_count(const int* __restrict__ slot_ij, const int* __restrict__ cam_off,
                                                             const int* __restrict__ cam_pt, int* __restrict__ cnt) {
  const int slot = blockIdx.x, lane = threadIdx.x;
  const int i = slot_ij[2 * slot], j = slot_ij[2 * slot + 1];
  const int a0 = cam_off[i], a1 = cam_off[i + 1], b0 = cam_off[j], b1 = cam_off[j + 1];
  int c = 0;
  for (int e = a0 + lane; e < a1; e += PRIOR_WAVE) c += prior_find(cam_pt, b0, b1, cam_pt[e]) >= 0 ? 1 : 0;
  c = wave_sum_int(c);
  if (lane == 0) cnt[slot] = c;
}

__global__ __launch_bounds__(PRIOR_WAVE) void k_prior_gather(const int* __restrict__ cand_slot, const int* __restrict__ slot_ij,
                                                              const int* __restrict__ cam_off, const int* __restrict__ cam_pt,
                                                              const int* __restrict__ cam_obs, const float2* __restrict__ xy,
                                                              const int* __restrict__ off, float2* __restrict__ pt1, float2* __restrict__ pt2) {
  const int c = blockIdx.x, lane = threadIdx.x;
  const int slot = cand_slot[c];
  const int i = slot_ij[2 * slot], j = slot_ij[2 * slot + 1];
  const int a0 = cam_off[i], a1 = cam_off[i + 1], b0 = cam_off[j], b1 = cam_off[j + 1];
  int base = off[c];
  const int end = off[c + 1];
  for (int e0 = a0; e0 < a1; e0 += PRIOR_WAVE) {
    const int e = e0 + lane;
    const int pos = e < a1 ? prior_find(cam_pt, b0, b1, cam_pt[e]) : -1;
    const uint64_t m = __ballot(pos >= 0);
    const int out = base + __popcll(m & ((1ull << lane) - 1ull));
    if (pos >= 0 && out < end) {
      pt1[out] = xy[cam_obs[e]];
      pt2[out] = xy[cam_obs[pos]];
    }
    base += __popcll(m);
  }
}

MSFM_API void msfm_slam_prior_default_options(msfm_slam_prior_options* o) {
  if (!o) return;
  o->win_size = 5;
  o->th_same_pts = 20;
  o->th_epipolar = 2.0f;
  o->th_distance = 5.0f;
  o->th_ratio_f = 0.5f;
  o->th_h_f_ratio = 0.90f;
  o->seed_f = 0x4D53464D46ull;
  o->seed_h = 0x4D53464D48ull;
}

MSFM_API int msfm_slam_priors(msfm_ctx* ctx, const msfm_tracks* P, const msfm_slam_prior_options* opt, int* n_pairs, int* pairs,
                              double* F, double* H, int* n_candidates, int* candidates) {
  if (!ctx || !P || !opt || !n_pairs) return MSFM_E_INVAL;
  *n_pairs = 0;
  if (n_candidates) *n_candidates = 0;
  if (opt->win_size < 1) return msfm_set_error(ctx, MSFM_E_INVAL, "slam_priors: win_size < 1");
  if (opt->th_same_pts < 15) return msfm_set_error(ctx, MSFM_E_INVAL, "slam_priors: th_same_pts < 15 (findFundamentalMat would not run RANSAC)");
  // the thresholds as the public calls take them: msfm_fundamental_ransac_batch refuses threshold <= 0 or NaN,
  // msfm_homography_ransac_batch refuses NaN (and maps <= 0 to 3.0, as geo_hransac_dev does here)
  if (!(opt->th_epipolar > 0.0f)) return msfm_set_error(ctx, MSFM_E_INVAL, "slam_priors: th_epipolar must be > 0");
  if (opt->th_distance != opt->th_distance) return msfm_set_error(ctx, MSFM_E_INVAL, "slam_priors: th_distance is NaN");
  const int n_pts = P->n_tracks, n_cams = P->n_cams;
  if (n_pts < 0 || n_cams < 0 || (n_pts > 0 && !P->track_off)) return msfm_set_error(ctx, MSFM_E_INVAL, "slam_priors: bad point arrays");
  const int n_obs = n_pts > 0 ? P->track_off[n_pts] : 0;
  if (n_pts > 0 && P->track_off[0] != 0) return msfm_set_error(ctx, MSFM_E_INVAL, "slam_priors: track_off[0] must be 0");
  for (int t = 0; t < n_pts; t++)
    if (P->track_off[t + 1] < P->track_off[t]) return msfm_set_error(ctx, MSFM_E_INVAL, "slam_priors: track_off must be non-decreasing");
  if (n_obs > 0 && (!P->track_cam || !P->track_xy)) return msfm_set_error(ctx, MSFM_E_INVAL, "slam_priors: missing observations");
  const long long cap = (long long)n_cams * (2 * opt->win_size - 1);
  if (cap > 0 && (!pairs || !F || !H)) return msfm_set_error(ctx, MSFM_E_INVAL, "slam_priors: missing output buffers");
  // stable counting sort of the observations by camera; one observation per (point, camera)
  std::vector<int> cam_off((size_t)n_cams + 1, 0), last((size_t)n_cams, -1);
  for (int t = 0; t < n_pts; t++)
    for (int o = P->track_off[t]; o < P->track_off[t + 1]; o++) {
      const int c = P->track_cam[o];
      if (c < 0 || c >= n_cams) return msfm_set_error(ctx, MSFM_E_INVAL, "slam_priors: camera %d of point %d outside [0, %d)", c, t, n_cams);
      if (last[c] == t) return msfm_set_error(ctx, MSFM_E_INVAL, "slam_priors: point %d has two observations in camera %d", t, c);
      last[c] = t;
      cam_off[c + 1]++;
    }
  for (int c = 0; c < n_cams; c++) cam_off[c + 1] += cam_off[c];
  std::vector<int> cam_pt(std::max(1, n_obs)), cam_obs(std::max(1, n_obs));
  std::vector<float> xy(2 * (size_t)std::max(1, n_obs));
  {
    std::vector<int> fill(cam_off.begin(), cam_off.end() - 1);
    for (int t = 0; t < n_pts; t++)
      for (int o = P->track_off[t]; o < P->track_off[t + 1]; o++) {
        const int k = fill[P->track_cam[o]]++;
        cam_pt[k] = t;
        cam_obs[k] = o;
        xy[2 * (size_t)o] = (float)P->track_xy[2 * (size_t)o];          // cv::Point2f(it1->second(0), it1->second(1))
        xy[2 * (size_t)o + 1] = (float)P->track_xy[2 * (size_t)o + 1];
      }
  }
  // window slots in (i, j) order (slam_gps.cc:348-357)
  std::vector<int> slot_ij;
  for (int i = 0; i < n_cams; i++)
    for (int j = std::max(i - opt->win_size, 0); j < std::min(i + opt->win_size, n_cams); j++)
      if (j != i) { slot_ij.push_back(i); slot_ij.push_back(j); }
  const int n_slots = (int)slot_ij.size() / 2;
  if (n_slots == 0) return MSFM_OK;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  DevBuf<int> d_slot, d_cam_off, d_cam_pt, d_cam_obs, d_cnt, d_cand, d_off, d_nin;
  DevBuf<float> d_xy, d1, d2;
  DevBuf<double> dF, dH;
  DevBuf<uint8_t> d_in, d_ok;
  DevScope sc(ctx);
  HIP_TRY(ctx, d_slot.from(slot_ij, s));
  HIP_TRY(ctx, d_cam_off.from(cam_off, s));
  HIP_TRY(ctx, d_cam_pt.from(cam_pt, s));
  HIP_TRY(ctx, d_cam_obs.from(cam_obs, s));
  HIP_TRY(ctx, d_xy.from(xy, s));
  HIP_TRY(ctx, d_cnt.alloc(n_slots));
  {
    KTimer t(ctx, "prior_count");
    hipLaunchKernelGGL(k_prior_count, dim3(n_slots), dim3(PRIOR_WAVE), 0, s, d_slot.p, d_cam_off.p, d_cam_pt.p, d_cnt.p);
  }
  HIP_TRY(ctx, hipGetLastError());
  std::vector<int> cnt(n_slots);
  HIP_TRY(ctx, hipMemcpyAsync(cnt.data(), d_cnt.p, sizeof(int) * (size_t)n_slots, hipMemcpyDeviceToHost, s));
  HIP_TRY(ctx, hipStreamSynchronize(s));
  // candidates: the slots with enough shared points; their index in this list is the RANSACs' sampler index
  std::vector<int> cand_slot, off(1, 0);
  for (int k = 0; k < n_slots; k++)
    if (cnt[k] >= opt->th_same_pts) { cand_slot.push_back(k); off.push_back(off.back() + cnt[k]); }
  const int n_cand = (int)cand_slot.size();
  std::vector<int> nf(std::max(1, n_cand), 0), nh(std::max(1, n_cand), -1);
  std::vector<double> Fc(9 * (size_t)std::max(1, n_cand)), Hc(9 * (size_t)std::max(1, n_cand));
  std::vector<uint8_t> fpass(std::max(1, n_cand), 0);
  if (n_cand > 0) {
    const int total = off[n_cand];
    HIP_TRY(ctx, d_cand.from(cand_slot, s));
    HIP_TRY(ctx, d_off.from(off, s));
    HIP_TRY(ctx, d1.alloc(2 * (size_t)total));
    HIP_TRY(ctx, d2.alloc(2 * (size_t)total));
    {
      KTimer t(ctx, "prior_gather");
      hipLaunchKernelGGL(k_prior_gather, dim3(n_cand), dim3(PRIOR_WAVE), 0, s, d_cand.p, d_slot.p, d_cam_off.p, d_cam_pt.p, d_cam_obs.p,
                         reinterpret_cast<const float2*>(d_xy.p), d_off.p, reinterpret_cast<float2*>(d1.p), reinterpret_cast<float2*>(d2.p));
    }
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, dF.alloc(9 * (size_t)n_cand));
    HIP_TRY(ctx, dH.alloc(9 * (size_t)n_cand));
    HIP_TRY(ctx, d_in.alloc(total));
    HIP_TRY(ctx, d_nin.alloc(n_cand));
    HIP_TRY(ctx, d_ok.alloc(n_cand));
    // F: cv::findFundamentalMat(pts1, pts2, status_f, FM_RANSAC, th_epipolar)  (:385-393)
    msfm_fransac_options fo;
    msfm_fransac_default_options(&fo);
    fo.threshold = opt->th_epipolar;
    fo.confidence = 0.99;
    fo.max_iterations = 2000;
    fo.min_points = 8;
    fo.min_inliers = 0;
    fo.seed = opt->seed_f;
    MSFM_TRY(geo_fransac_dev(ctx, n_cand, off.data(), d_off.p, d1.p, d2.p, &fo, dF.p, d_in.p, d_nin.p, d_ok.p));
    HIP_TRY(ctx, hipMemcpyAsync(nf.data(), d_nin.p, sizeof(int) * (size_t)n_cand, hipMemcpyDeviceToHost, s));
    HIP_TRY(ctx, hipMemcpyAsync(Fc.data(), dF.p, sizeof(double) * 9 * (size_t)n_cand, hipMemcpyDeviceToHost, s));
    HIP_TRY(ctx, hipStreamSynchronize(s));
    int n_pass = 0;
    for (int c = 0; c < n_cand; c++) {
      const int N = off[c + 1] - off[c];
      // count_inlier_f < pts1.size() * th_ratio_f || count_inlier_f < 30   (:396, binary32)
      fpass[c] = !((float)nf[c] < (float)N * opt->th_ratio_f || nf[c] < 30);
      n_pass += fpass[c];
    }
    if (n_pass > 0) {
      // H: cv::findHomography(pts1, pts2, status_h, RANSAC, th_distance)  (:400-408), only where the F gate passed
      msfm_hransac_options ho;
      msfm_hransac_default_options(&ho);
      ho.threshold = opt->th_distance;
      ho.seed = opt->seed_h;
      MSFM_TRY(geo_hransac_dev(ctx, n_cand, off.data(), d_off.p, d1.p, d2.p, &ho, fpass.data(), dH.p, d_in.p, d_nin.p, d_ok.p));
      HIP_TRY(ctx, hipMemcpyAsync(nh.data(), d_nin.p, sizeof(int) * (size_t)n_cand, hipMemcpyDeviceToHost, s));
      HIP_TRY(ctx, hipMemcpyAsync(Hc.data(), dH.p, sizeof(double) * 9 * (size_t)n_cand, hipMemcpyDeviceToHost, s));
      HIP_TRY(ctx, hipStreamSynchronize(s));
    }
  }
  sc.dismiss();   // behind the last of the waits above: nothing has been enqueued since
  // verdicts in slot order
  int kept = 0, c = 0;
  for (int k = 0; k < n_slots; k++) {
    const int i = slot_ij[2 * k], j = slot_ij[2 * k + 1];
    int v_nf = -1, v_nh = -1, verdict = 1;
    if (c < n_cand && cand_slot[c] == k) {
      v_nf = nf[c];
      if (!fpass[c]) verdict = 2;
      else {
        v_nh = nh[c];
        // count_inlier_h > count_inlier_f * th_h_f_ratio   (:409, binary32)
        if ((float)nh[c] > (float)nf[c] * opt->th_h_f_ratio) verdict = 3;
        else {
          verdict = 0;
          pairs[2 * kept] = i; pairs[2 * kept + 1] = j;
          for (int q = 0; q < 9; q++) { F[9 * (size_t)kept + q] = Fc[9 * (size_t)c + q]; H[9 * (size_t)kept + q] = Hc[9 * (size_t)c + q]; }
          kept++;
        }
      }
      c++;
    }
    if (candidates) {
      int* r = candidates + 6 * (size_t)k;
      r[0] = i; r[1] = j; r[2] = cnt[k]; r[3] = v_nf; r[4] = v_nh; r[5] = verdict;
    }
  }
  *n_pairs = kept;
  if (n_candidates) *n_candidates = n_slots;
  return MSFM_OK;
}
