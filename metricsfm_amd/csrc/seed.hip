// Which seed pair reconstructs, and with which points: the loop body of
//   IncrementalSfM::FindSeedPairThenReconstruct     SfM/src/sfm_incremental.cc:235-390
// for a whole list of hypotheses in one call, on the resident match store (the reference walks its sorted pair list one
// hypothesis at a time and re-parses a `<i>_match` file for each; on unordered photo sets most hypotheses fail).
//
//   k_gather    one thread per match of all hypotheses: (f1, f2) from the store, the four keypoint floats -> double
//               (:298-303), into the CSR of the hypothesis' arm.  Two offset arrays over all n_hyp, each with empty segments
//               for the other arm, so hypothesis h is problem h of the pose call it belongs to.
//   pose        pose_relpose5_dev / pose_relpose8_dev of pose.hip on those buffers (:307-322): the kernels of
//               msfm_relpose_5pt_batch / msfm_relpose_8pt_batch, not copies of them
//   k_camera    one thread per hypothesis: the focal rule (:324-332), c = -(R^T t) (:334), the fk rows of both cameras
//   k_tri       one thread per match: Point3D::Trianglate2 for two views (structure.cc:211-265 with Reprojection :267-300 and
//               SufficientTriangulationAngle :325-355): tri_two_views of point3d_device.h.  A workgroup lies inside one
//               hypothesis (block map by binary search in n_hyp + 1 block offsets); its camera data is loaded once into LDS.
//   k_compact   one workgroup per hypothesis walks its flags in chunks of 256 (wave ballot + the four wave counts): accepted
//               points in match order, the count and the two gates (:380-381); a hypothesis that passes enters the minimum
//               that names the winner
//   k_keep      the winner's points into blocks of their own, which the set keeps (msfm_recon_create_from_seed reads them)
// No host synchronisation between the stages: every size follows from the store's host-side match_off; one synchronisation
// at the end.  This file is compiled without fused multiply-adds and uses + - * / sqrt only (pose.hip's discipline), so
// tests/seed_ref.cpp built with -ffp-contract=off agrees bit for bit; tri.hip is contracted and agrees to 1e-9.
#include <climits>
#include <cmath>
#include <memory>

#include "common.h"

#pragma clang fp contract(off)
#include "point3d_device.h"   // View, tri_two_views

namespace seed {

struct Hyp { int m0, kp1, kp2, arm; };   // first match in the store, keypoint rows of image 1 / 2, 5 or 8

__global__ __launch_bounds__(256) void k_gather(int M, int n, const int* __restrict__ off_all, const Hyp* __restrict__ hyp,
                                                 const int* __restrict__ off5, const int* __restrict__ off8, const int* __restrict__ matches,
                                                 const float* __restrict__ kp, double* __restrict__ ref5, double* __restrict__ cur5,
                                                 double* __restrict__ ref8, double* __restrict__ cur8) {
  const int m = blockIdx.x * 256 + threadIdx.x;
  if (m >= M) return;
  const int h = csr_segment_of(off_all, n, m);
  const Hyp H = hyp[h];
  const int j = m - off_all[h];
  const size_t sm = (size_t)H.m0 + j;
  const size_t r1 = (size_t)H.kp1 + matches[2 * sm], r2 = (size_t)H.kp2 + matches[2 * sm + 1];
  const bool five = H.arm == 5;
  const size_t o = (size_t)(five ? off5[h] : off8[h]) + j;
  double* a = five ? ref5 : ref8;
  double* b = five ? cur5 : cur8;
  a[2 * o] = (double)kp[2 * r1]; a[2 * o + 1] = (double)kp[2 * r1 + 1];
  b[2 * o] = (double)kp[2 * r2]; b[2 * o + 1] = (double)kp[2 * r2 + 1];
}

// cam [n][21]: R (9), t (3), c (3) of camera 1, fk of camera 0 (3), fk of camera 1 (3)
#define SEED_CAM 21
__global__ __launch_bounds__(64) void k_camera(int n, const Hyp* __restrict__ hyp, const double* __restrict__ cam_fk, const uint8_t* __restrict__ same_model,
                                                const uint8_t* __restrict__ ok5, const double* __restrict__ R5, const double* __restrict__ t5,
                                                const uint8_t* __restrict__ ok8, const double* __restrict__ R8, const double* __restrict__ t8,
                                                const double* __restrict__ f1_8, const double* __restrict__ f2_8, uint8_t* __restrict__ pose_ok,
                                                double* __restrict__ f_out, double* __restrict__ cam) {
  const int h = blockIdx.x * 64 + threadIdx.x;
  if (h >= n) return;
  const bool five = hyp[h].arm == 5;
  const bool ok = (five ? ok5[h] : ok8[h]) != 0;
  double fa = cam_fk[6 * (size_t)h], fb = cam_fk[6 * (size_t)h + 3];
  double* C = cam + SEED_CAM * (size_t)h;
  for (int k = 0; k < 15; k++) C[k] = 0.0;
  if (ok) {
    const double* R = (five ? R5 : R8) + 9 * (size_t)h;
    const double* t = (five ? t5 : t8) + 3 * (size_t)h;
    if (!five) {   // :324-332
      const double f1 = f1_8[h], f2 = f2_8[h];
      if (same_model[h]) { fa = (f1 + f2) / 2.0; fb = fa; }
      else { fa = f1; fb = f2; }
    }
    for (int k = 0; k < 9; k++) C[k] = R[k];
    for (int k = 0; k < 3; k++) C[9 + k] = t[k];
    for (int k = 0; k < 3; k++) C[12 + k] = -(R[k] * t[0] + R[3 + k] * t[1] + R[6 + k] * t[2]);   // Camera::SetRTPose
  }
  C[15] = fa; C[16] = cam_fk[6 * (size_t)h + 1]; C[17] = cam_fk[6 * (size_t)h + 2];
  C[18] = fb; C[19] = cam_fk[6 * (size_t)h + 4]; C[20] = cam_fk[6 * (size_t)h + 5];
  pose_ok[h] = ok ? 1 : 0;
  f_out[2 * (size_t)h] = fa; f_out[2 * (size_t)h + 1] = fb;
}

__global__ __launch_bounds__(256) void k_tri(int n, const int* __restrict__ blk_off, const int* __restrict__ off_all, const Hyp* __restrict__ hyp,
                                              const int* __restrict__ off5, const int* __restrict__ off8, const double* __restrict__ ref5,
                                              const double* __restrict__ cur5, const double* __restrict__ ref8, const double* __restrict__ cur8,
                                              const uint8_t* __restrict__ pose_ok, const double* __restrict__ cam, double th_error, double cos_min,
                                              uint8_t* __restrict__ flag, double* __restrict__ Xall, double* __restrict__ mse_all) {
  __shared__ double s_cam[SEED_CAM + 12];   // + camera 0: R = I (9), t = c = 0 (3)
  const int h = csr_segment_of(blk_off, n, (int)blockIdx.x);   // (uniform)
  if (threadIdx.x < SEED_CAM) s_cam[threadIdx.x] = cam[SEED_CAM * (size_t)h + threadIdx.x];
  else if (threadIdx.x < SEED_CAM + 12) { const int k = threadIdx.x - SEED_CAM; s_cam[threadIdx.x] = (k == 0 || k == 4 || k == 8) ? 1.0 : 0.0; }
  __syncthreads();
  const int b = off_all[h], N = off_all[h + 1] - b;
  const int j = ((int)blockIdx.x - blk_off[h]) * 256 + threadIdx.x;
  if (j >= N) return;
  const size_t m = (size_t)b + j;
  if (!pose_ok[h]) { flag[m] = 0; return; }   // :313, :321
  const bool five = hyp[h].arm == 5;
  const size_t o = (size_t)(five ? off5[h] : off8[h]) + j;
  const double* pa = five ? ref5 : ref8;
  const double* pb = five ? cur5 : cur8;
  View V[2];
  V[0].R = s_cam + SEED_CAM; V[0].t = s_cam + SEED_CAM + 9; V[0].c = s_cam + SEED_CAM + 9; V[0].fk = s_cam + 15;
  V[0].x = pa[2 * o]; V[0].y = pa[2 * o + 1];
  V[1].R = s_cam; V[1].t = s_cam + 9; V[1].c = s_cam + 12; V[1].fk = s_cam + 18;
  V[1].x = pb[2 * o]; V[1].y = pb[2 * o + 1];
  double X[3] = {0, 0, 0}, mse = 0.0;
  const bool ok = tri_two_views(V, th_error, cos_min, X, &mse);
  flag[m] = ok ? 1 : 0;
  Xall[3 * m] = X[0]; Xall[3 * m + 1] = X[1]; Xall[3 * m + 2] = X[2];
  mse_all[m] = mse;
}

// one workgroup per hypothesis; the accepted points of hypothesis h go to [off_all[h], off_all[h] + count[h]) of the outputs
__global__ __launch_bounds__(256) void k_compact(const int* __restrict__ off_all, const uint8_t* __restrict__ flag, const double* __restrict__ Xall,
                                                  const double* __restrict__ mse_all, const uint8_t* __restrict__ pose_ok, int th_structures,
                                                  int* __restrict__ pt_match, double* __restrict__ Xout, double* __restrict__ mse_out,
                                                  int* __restrict__ count, uint8_t* __restrict__ pass, int* __restrict__ winner) {
  __shared__ int part[4];
  const int h = blockIdx.x;
  const int b = off_all[h], N = off_all[h + 1] - b;
  int base = 0;
  for (int c0 = 0; c0 < N; c0 += 256) {
    const int j = c0 + threadIdx.x;
    const bool keep = j < N && flag[(size_t)b + j] != 0;
    int total;
    const int before = wg_rank<4>(keep, part, total);
    if (keep) {
      const size_t s = (size_t)b + j, e = (size_t)b + base + before;
      pt_match[e] = j;
      Xout[3 * e] = Xall[3 * s]; Xout[3 * e + 1] = Xall[3 * s + 1]; Xout[3 * e + 2] = Xall[3 * s + 2];
      mse_out[e] = mse_all[s];
    }
    base += total;
  }
  if (threadIdx.x == 0) {
    count[h] = base;
    const bool ok = pose_ok[h] && base >= th_structures && base >= N / 5;   // :380-381
    pass[h] = ok ? 1 : 0;
    if (ok) atomicMin(winner, h);
  }
}

// The winner's segment of k_compact's outputs, copied to the front of blocks of `cap` points (cap >= the matches of any
// hypothesis); *winner is INT_MAX when no hypothesis passed.
__global__ __launch_bounds__(256) void k_keep(int cap, const int* __restrict__ winner, const int* __restrict__ off_all, const int* __restrict__ count,
                                               const int* __restrict__ pt_match, const double* __restrict__ X, const double* __restrict__ mse,
                                               int* __restrict__ w_match, double* __restrict__ w_X, double* __restrict__ w_mse) {
  const int w = *winner;
  if (w == INT_MAX) return;
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= count[w] || j >= cap) return;
  const size_t s = (size_t)off_all[w] + j;
  w_match[j] = pt_match[s];
  w_X[3 * (size_t)j] = X[3 * s]; w_X[3 * (size_t)j + 1] = X[3 * s + 1]; w_X[3 * (size_t)j + 2] = X[3 * s + 2];
  w_mse[j] = mse[s];
}

}  // namespace seed

#define SD_TRY(e) HIP_TRY(ctx, (e))

MSFM_API void msfm_seed_default_options(msfm_seed_options* o) {
  if (!o) return;
  o->th_mse_reprojection = 3.0;
  o->th_angle_small = 3.0 / 180.0 * 3.1415;
  o->th_seedpair_structures = 20;
  o->ransac_times_5pt = 100;
  o->ransac_times_8pt = 200;
  o->seed_5pt = 0x4D53464D45ull;
  o->seed_8pt = 0x4D53464D38ull;
}

MSFM_API int msfm_seed_hypotheses(msfm_ctx* ctx, const msfm_match_store* S, const msfm_seed_problem* P, const msfm_seed_options* opt_in,
                                  msfm_seed_set** out) {
  using namespace seed;
  const char* who = "msfm_seed_hypotheses";
  if (!ctx) return MSFM_E_INVAL;
  if (!S || !P || !out) return msfm_set_error(ctx, MSFM_E_INVAL, "%s: null argument", who);
  *out = nullptr;
  if (S->ctx != ctx) return msfm_set_error(ctx, MSFM_E_INVAL, "%s: the store belongs to another context", who);
  msfm_seed_options opt;
  if (opt_in) opt = *opt_in; else msfm_seed_default_options(&opt);
  const int n = P->n_hyp, ni = S->n_images;
  if (n < 0 || n > 65535) return msfm_set_error(ctx, MSFM_E_INVAL, "%s: n_hyp = %d outside [0, 65535]", who, n);
  if (n && (!P->hyp_img || !P->cam_fk || !P->same_model)) return msfm_set_error(ctx, MSFM_E_INVAL, "%s: null array", who);
  if (opt.th_mse_reprojection != opt.th_mse_reprojection || opt.th_angle_small != opt.th_angle_small || opt.th_seedpair_structures < 0)
    return msfm_set_error(ctx, MSFM_E_INVAL, "%s: a threshold is NaN or negative", who);
  if (opt.ransac_times_5pt < 1 || opt.ransac_times_5pt > 65536 || opt.ransac_times_8pt < 1 || opt.ransac_times_8pt > 65536)
    return msfm_set_error(ctx, MSFM_E_INVAL, "%s: ransac_times out of range", who);
  // ---- O(hypotheses) on the host: the store pair of each, its arm, the three CSRs, the block map ----
  Child<msfm_seed_set> R = child_new<msfm_seed_set>(ctx);
  R->store = S; R->n = n;
  R->arm.assign(n, 0); R->n_matches.assign(n, 0);
  std::vector<Hyp> hyp(n);
  std::vector<int> off_all(n + 1, 0), off5(n + 1, 0), off8(n + 1, 0), blk_off(n + 1, 0);
  int longest = 0;                           // matches of the longest hypothesis: the capacity of the winner's blocks
  std::vector<int> kp_base;                  // per image: its first row in the uploaded keypoints, -1: not uploaded
  std::vector<int> kp_imgs;
  std::vector<double> f5_ref(n), f5_cur(n);   // f of the five-point arm = the given values (uploaded only if that arm has a match)
  if (P->keypoints) kp_base.assign(std::max(1, ni), -1);
  long kp_rows = 0;
  for (int h = 0; h < n; h++) {
    const int i1 = P->hyp_img[2 * h], i2 = P->hyp_img[2 * h + 1];
    if (i1 < 0 || i1 >= ni || i2 < 0 || i2 >= ni) return msfm_set_error(ctx, MSFM_E_INVAL, "%s: hypothesis %d = (%d, %d) names no image of the store", who, h, i1, i2);
    if (i1 == i2) return msfm_set_error(ctx, MSFM_E_INVAL, "%s: hypothesis %d pairs image %d with itself", who, h, i1);
    const double f1 = P->cam_fk[6 * (size_t)h], f2 = P->cam_fk[6 * (size_t)h + 3];
    if (!(f1 >= 0.0) || !(f2 >= 0.0)) return msfm_set_error(ctx, MSFM_E_INVAL, "%s: hypothesis %d has a negative or NaN focal length", who, h);
    for (int im : {i1, i2}) {
      if (P->keypoints) {
        if (kp_base[im] < 0) { kp_base[im] = (int)kp_rows; kp_imgs.push_back(im); kp_rows += S->n_features[im]; }
      } else if (!S->has_kp[im]) {
        return msfm_set_error(ctx, MSFM_E_INVAL, "%s: no keypoints of image %d (argument or chain)", who, im);
      }
    }
    if (kp_rows > 0x7fffffffL) return msfm_set_error(ctx, MSFM_E_INVAL, "%s: more than 2^31 keypoints", who);
    int m0 = 0, cnt = 0;
    for (int p = S->row_off[i1]; p < S->row_off[i1 + 1]; p++)   // QueryMatch(i1, i2): row i1, entry i2
      if (S->pair_img[2 * p + 1] == i2) { m0 = S->match_off[p]; cnt = S->match_off[p + 1] - m0; break; }
    const int arm = (f1 != 0.0 && f2 != 0.0) ? 5 : 8;   // :307
    hyp[h] = Hyp{m0, P->keypoints ? kp_base[i1] : S->feat_off[i1], P->keypoints ? kp_base[i2] : S->feat_off[i2], arm};
    R->arm[h] = (uint8_t)arm; R->n_matches[h] = cnt;
    longest = std::max(longest, cnt);
    if ((long)off_all[h] + cnt > 0x7fffffffL) return msfm_set_error(ctx, MSFM_E_INVAL, "%s: more than 2^31 matches in one call", who);
    off_all[h + 1] = off_all[h] + cnt;
    off5[h + 1] = off5[h] + (arm == 5 ? cnt : 0);
    off8[h + 1] = off8[h] + (arm == 8 ? cnt : 0);
    blk_off[h + 1] = blk_off[h] + cdiv(cnt, 256);
  }
  const int M = off_all[n], M5 = off5[n], M8 = off8[n];
  R->pose_ok.assign(n, 0); R->pass.assign(n, 0); R->pt_off.assign(n + 1, 0);
  R->f.assign(2 * (size_t)n, 0.0); R->R.assign(9 * (size_t)n, 0.0); R->t.assign(3 * (size_t)n, 0.0); R->c.assign(3 * (size_t)n, 0.0);
  if (n == 0) { *out = R.release(); return MSFM_OK; }
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  DevBuf<Hyp> d_hyp;
  DevBuf<int> d_offa, d_off5, d_off8, d_blk, d_ptm, d_count, d_win;
  DevBuf<double> d_fk, d_ref5, d_cur5, d_ref8, d_cur8, d_f5a, d_f5b;
  DevBuf<double> d_fout, d_cam, d_Xall, d_mseall, d_X, d_mse;
  DevBuf<uint8_t> d_same, d_pok, d_flag, d_pass;
  DevBuf<float> d_kp_up;
  Relpose5Result r5;
  Relpose8Result r8;
  DevScope sc(ctx);
  SD_TRY(sc.up(d_hyp, hyp.data(), (size_t)n)); SD_TRY(sc.up(d_offa, off_all.data(), (size_t)n + 1)); SD_TRY(sc.up(d_off5, off5.data(), (size_t)n + 1));
  SD_TRY(sc.up(d_off8, off8.data(), (size_t)n + 1)); SD_TRY(sc.up(d_blk, blk_off.data(), (size_t)n + 1)); SD_TRY(sc.up(d_fk, P->cam_fk, 6 * (size_t)n));
  SD_TRY(sc.up(d_same, P->same_model, (size_t)n));
  const float* d_kp = S->d_kp.p;
  if (P->keypoints) {   // the rows of the hypotheses' images only
    SD_TRY(d_kp_up.alloc(2 * (size_t)std::max(1L, kp_rows)));
    for (int im : kp_imgs) {
      const size_t cnt = 2 * (size_t)S->n_features[im];
      if (cnt) SD_TRY(hipMemcpyAsync(d_kp_up.p + 2 * (size_t)kp_base[im], P->keypoints + 2 * (size_t)S->feat_off[im], sizeof(float) * cnt, hipMemcpyHostToDevice, s));
      sc.h2d += (int64_t)(sizeof(float) * cnt);
    }
    d_kp = d_kp_up.p;
  }
  const size_t Mx = (size_t)std::max(1, M);
  SD_TRY(d_ref5.alloc(2 * (size_t)std::max(1, M5))); SD_TRY(d_cur5.alloc(2 * (size_t)std::max(1, M5)));
  SD_TRY(d_ref8.alloc(2 * (size_t)std::max(1, M8))); SD_TRY(d_cur8.alloc(2 * (size_t)std::max(1, M8)));
  SD_TRY(r5.alloc(n, M5)); SD_TRY(r8.alloc(n, M8));   // both: k_camera gets every array, and reads an arm's only where its ok is set
  SD_TRY(d_pok.alloc(n)); SD_TRY(d_fout.alloc(2 * (size_t)n)); SD_TRY(d_cam.alloc(SEED_CAM * (size_t)n));
  SD_TRY(d_flag.alloc(Mx)); SD_TRY(d_Xall.alloc(3 * Mx)); SD_TRY(d_mseall.alloc(Mx));
  SD_TRY(d_ptm.alloc(Mx)); SD_TRY(d_X.alloc(3 * Mx)); SD_TRY(d_mse.alloc(Mx)); SD_TRY(d_count.alloc(n)); SD_TRY(d_pass.alloc(n));
  SD_TRY(d_win.alloc(1));
  SD_TRY(hipMemsetD32Async((hipDeviceptr_t)d_win.p, INT_MAX, 1, s));
  if (longest) {
    SD_TRY(R->d_ptm.alloc((size_t)longest)); SD_TRY(R->d_X.alloc(3 * (size_t)longest)); SD_TRY(R->d_mse.alloc((size_t)longest));
  }
  // an arm without a match is not launched: its hypotheses have failed (fewer than 5 / 8 matches)
  SD_TRY(hipMemsetAsync(r5.ok.p, 0, (size_t)n, s)); SD_TRY(hipMemsetAsync(r8.ok.p, 0, (size_t)n, s));
  if (M) {
    KTimer tm(ctx, "seed_gather");
    hipLaunchKernelGGL(k_gather, dim3(cdiv(M, 256)), dim3(256), 0, s, M, n, d_offa.p, d_hyp.p, d_off5.p, d_off8.p, S->d_match.p, d_kp, d_ref5.p, d_cur5.p,
                       d_ref8.p, d_cur8.p);
  }
  SD_TRY(hipGetLastError());
  if (M5) {
    // the eight-point hypotheses' entries (problems without matches) are not read
    for (int h = 0; h < n; h++) { f5_ref[h] = P->cam_fk[6 * (size_t)h]; f5_cur[h] = P->cam_fk[6 * (size_t)h + 3]; }
    SD_TRY(sc.up(d_f5a, f5_ref.data(), (size_t)n)); SD_TRY(sc.up(d_f5b, f5_cur.data(), (size_t)n));
    MSFM_TRY(pose_relpose5_dev(ctx, PoseView{n, d_off5.p, d_ref5.p, d_cur5.p, d_f5a.p, d_f5b.p}, opt.ransac_times_5pt, opt.seed_5pt, r5));
  }
  if (M8) MSFM_TRY(pose_relpose8_dev(ctx, PoseView{n, d_off8.p, d_ref8.p, d_cur8.p, nullptr, nullptr}, opt.ransac_times_8pt, opt.seed_8pt, r8));
  {
    KTimer tm(ctx, "seed_camera");
    hipLaunchKernelGGL(k_camera, dim3(cdiv(n, 64)), dim3(64), 0, s, n, d_hyp.p, d_fk.p, d_same.p, r5.ok.p, r5.R.p, r5.t.p, r8.ok.p, r8.R.p, r8.t.p,
                       r8.f_ref.p, r8.f_cur.p, d_pok.p, d_fout.p, d_cam.p);
  }
  if (M) {
    KTimer tm(ctx, "seed_triangulate");
    hipLaunchKernelGGL(k_tri, dim3(blk_off[n]), dim3(256), 0, s, n, d_blk.p, d_offa.p, d_hyp.p, d_off5.p, d_off8.p, d_ref5.p, d_cur5.p, d_ref8.p, d_cur8.p,
                       d_pok.p, d_cam.p, opt.th_mse_reprojection, cos(opt.th_angle_small), d_flag.p, d_Xall.p, d_mseall.p);
  }
  {
    KTimer tm(ctx, "seed_compact");
    hipLaunchKernelGGL(k_compact, dim3(n), dim3(256), 0, s, d_offa.p, d_flag.p, d_Xall.p, d_mseall.p, d_pok.p, (int)opt.th_seedpair_structures, d_ptm.p,
                       d_X.p, d_mse.p, d_count.p, d_pass.p, d_win.p);
  }
  if (longest) {
    KTimer tm(ctx, "seed_keep");
    hipLaunchKernelGGL(k_keep, dim3(cdiv(longest, 256)), dim3(256), 0, s, longest, d_win.p, d_offa.p, d_count.p, d_ptm.p, d_X.p, d_mse.p, R->d_ptm.p,
                       R->d_X.p, R->d_mse.p);
  }
  SD_TRY(hipGetLastError());
  // ---- one read-back: the per-hypothesis records and the point arrays at their uncompacted capacity (M is known here, the
  //      counts are not); the host closes the gaps between the hypotheses ----
  std::vector<int> count(n), ptm(M);
  std::vector<double> cam(SEED_CAM * (size_t)n), X(3 * (size_t)M), mse(M);
  SD_TRY(hipMemcpyAsync(R->pose_ok.data(), d_pok.p, (size_t)n, hipMemcpyDeviceToHost, s));
  SD_TRY(hipMemcpyAsync(R->pass.data(), d_pass.p, (size_t)n, hipMemcpyDeviceToHost, s));
  SD_TRY(hipMemcpyAsync(count.data(), d_count.p, sizeof(int) * (size_t)n, hipMemcpyDeviceToHost, s));
  SD_TRY(hipMemcpyAsync(R->f.data(), d_fout.p, sizeof(double) * 2 * (size_t)n, hipMemcpyDeviceToHost, s));
  SD_TRY(hipMemcpyAsync(cam.data(), d_cam.p, sizeof(double) * SEED_CAM * (size_t)n, hipMemcpyDeviceToHost, s));
  if (M) {
    SD_TRY(hipMemcpyAsync(ptm.data(), d_ptm.p, sizeof(int) * (size_t)M, hipMemcpyDeviceToHost, s));
    SD_TRY(hipMemcpyAsync(X.data(), d_X.p, sizeof(double) * 3 * (size_t)M, hipMemcpyDeviceToHost, s));
    SD_TRY(hipMemcpyAsync(mse.data(), d_mse.p, sizeof(double) * (size_t)M, hipMemcpyDeviceToHost, s));
  }
  SD_TRY(sc.finish());   // the scratch above is released on return
  for (int h = 0; h < n; h++) {
    const double* C = cam.data() + SEED_CAM * (size_t)h;
    std::copy(C, C + 9, R->R.begin() + 9 * (size_t)h);
    std::copy(C + 9, C + 12, R->t.begin() + 3 * (size_t)h);
    std::copy(C + 12, C + 15, R->c.begin() + 3 * (size_t)h);
    R->pt_off[h + 1] = R->pt_off[h] + count[h];
    if (R->winner < 0 && R->pass[h]) R->winner = h;
  }
  const int T = R->pt_off[n];
  R->pt_match.resize(T); R->X.resize(3 * (size_t)T); R->mse.resize(T);
  for (int h = 0; h < n; h++) {
    const size_t b = (size_t)off_all[h], e = (size_t)R->pt_off[h], k = (size_t)count[h];
    std::copy(ptm.begin() + b, ptm.begin() + b + k, R->pt_match.begin() + e);
    std::copy(X.begin() + 3 * b, X.begin() + 3 * (b + k), R->X.begin() + 3 * e);
    std::copy(mse.begin() + b, mse.begin() + b + k, R->mse.begin() + e);
  }
  if (R->winner >= 0) {
    const Hyp& W = hyp[R->winner];
    R->win_img[0] = P->hyp_img[2 * R->winner]; R->win_img[1] = P->hyp_img[2 * R->winner + 1];
    R->win_m0 = W.m0;
    R->win_kp[0] = S->feat_off[R->win_img[0]]; R->win_kp[1] = S->feat_off[R->win_img[1]];
  } else {   // nothing to keep
    R->d_ptm.release(); R->d_X.release(); R->d_mse.release();
  }
  R->h2d_bytes = sc.h2d;
  *out = R.release();
  return MSFM_OK;
}

MSFM_API int msfm_seed_set_size(const msfm_seed_set* R, int* n_hyp, int* n_points, int* winner, int64_t* h2d_bytes) {
  if (!R) return MSFM_E_INVAL;
  if (n_hyp) *n_hyp = R->n;
  if (n_points) *n_points = R->pt_off[R->n];
  if (winner) *winner = R->winner;
  if (h2d_bytes) *h2d_bytes = R->h2d_bytes;
  return MSFM_OK;
}

MSFM_API int msfm_seed_set_fetch(const msfm_seed_set* R, uint8_t* arm, uint8_t* pose_ok, uint8_t* pass, int* n_matches, double* f, double* Rm, double* t,
                                 double* c, int* pt_off, int* pt_match, double* X, double* mse) {
  if (!R) return MSFM_E_INVAL;
  if (arm) std::copy(R->arm.begin(), R->arm.end(), arm);
  if (pose_ok) std::copy(R->pose_ok.begin(), R->pose_ok.end(), pose_ok);
  if (pass) std::copy(R->pass.begin(), R->pass.end(), pass);
  if (n_matches) std::copy(R->n_matches.begin(), R->n_matches.end(), n_matches);
  if (f) std::copy(R->f.begin(), R->f.end(), f);
  if (Rm) std::copy(R->R.begin(), R->R.end(), Rm);
  if (t) std::copy(R->t.begin(), R->t.end(), t);
  if (c) std::copy(R->c.begin(), R->c.end(), c);
  if (pt_off) std::copy(R->pt_off.begin(), R->pt_off.end(), pt_off);
  if (pt_match) std::copy(R->pt_match.begin(), R->pt_match.end(), pt_match);
  if (X) std::copy(R->X.begin(), R->X.end(), X);
  if (mse) std::copy(R->mse.begin(), R->mse.end(), mse);
  return MSFM_OK;
}

MSFM_API void msfm_seed_set_destroy(msfm_seed_set* R) { msfm_child_destroy(R); }
