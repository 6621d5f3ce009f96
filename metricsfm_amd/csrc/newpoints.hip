// The new 3D points of a localised image:
//   IncrementalSfM::GenerateNew3DPoints     SfM/src/sfm_incremental.cc:755-915
// for a list of new cameras in one call, on the resident match store (the reference re-parses a `<i>_match` file per visible
// camera, :777, and runs one Trianglate2 per new match, :821).
//
//   host        O(visible entries): the store pair of each entry from the store's row index, the segment CSR over all entries of
//               all new cameras (the "walk": new camera, visible entry, match - ascending), the block map, the rows of the
//               involved cameras.  No size is read back from the device.
//   k_tri       one thread per match of the walk; a workgroup lies inside one entry, whose two cameras it loads once into LDS:
//               the candidate test against the two feat_point rows (:804-808), the keypoint gather, tri_two_views (:810-821),
//               the sort key, and the entry's two counts (one atomic per wave)
//   sort        the key of walk position w is (new camera, accepted ? (int)mse : sentinel), the sentinel above every
//               possible (int)mse; ONE stable rocPRIM radix sort of (key, w) over the whole walk leaves every new camera's
//               range in place, its accepted points first, by truncated mse, ties in walk order (:829, :897).  The keys are a
//               few bits wide (4 + log2(n_new) for the default 3 px): one or two digit passes over the whole device.  An LDS
//               bitonic sort in the manner of localize.hip would need the accepted counts on the host, or LDS for a whole
//               camera's matches; a segmented sort hands a camera's range to one workgroup, and n_new = 1 is the usual case.
//               So there is one path.
//   k_claim     one thread per sorted position: atomicMin of the position into the (camera, feature) slot of both
//               observations - std::map::insert, the first point that names a slot keeps it (:908-909); slots are per new camera
//   k_emit      one thread per sorted position: features, X, mse and takes = (slot == own position)
// The call is newpoints_plan (checks and the host's tables) + a packed upload of the involved cameras' rows + newpoints_dev (the
// kernels; the result block stays on the device) + one read-back and newpoints_collect.  recon.hip runs plan and kernels on a
// resident feat_point / keypoint array (fp_resident, NP_KP_ALL: a camera's rows start at its offset in the whole array).
// One synchronisation, at the end.  Compiled without fused multiply-adds, + - * / sqrt only (seed.hip's discipline):
// tests/newpoints_ref.cpp built with -ffp-contract=off agrees bit for bit.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <memory>

#include "prim_device.h"

#pragma clang fp contract(off)
#include "point3d_device.h"   // View, tri_two_views

namespace newpts {

#define NP_CAM 18    // R (9), t (3), c (3), fk (3)
#define NP_BIG 0x7fffffff

using Ent = NewPointsEnt;   // one visible entry of one new camera (common.h)

__global__ __launch_bounds__(256) void k_tri(int E, const int* __restrict__ blk_off, const int* __restrict__ off_all, const Ent* __restrict__ ent,
                                              const int* __restrict__ matches, const int* __restrict__ fp, const float* __restrict__ kp,
                                              const double* __restrict__ cam, double th_error, double cos_small, double cos_large,
                                              unsigned sentinel, int key_bits, unsigned long long* __restrict__ key, int* __restrict__ val,
                                              double* __restrict__ Xall, double* __restrict__ mse_all, int* __restrict__ n_cand,
                                              int* __restrict__ n_acc) {
  __shared__ double s_cam[2 * NP_CAM];
  const int q = csr_segment_of(blk_off, E, (int)blockIdx.x);   // (uniform)
  const Ent e = ent[q];
  if (threadIdx.x < NP_CAM) s_cam[threadIdx.x] = cam[NP_CAM * (size_t)e.cam1 + threadIdx.x];
  else if (threadIdx.x < 2 * NP_CAM) s_cam[threadIdx.x] = cam[NP_CAM * (size_t)e.cam2 + (threadIdx.x - NP_CAM)];
  __syncthreads();
  const int b = off_all[q], N = off_all[q + 1] - b;
  const int j = ((int)blockIdx.x - blk_off[q]) * 256 + threadIdx.x;
  bool cand = false, ok = false;
  if (j < N) {
    const size_t m = (size_t)b + j, sm = (size_t)e.m0 + j;
    const int f1 = matches[2 * sm], f2 = matches[2 * sm + 1];
    cand = fp[(size_t)e.fp1 + f1] < 0 && fp[(size_t)e.fp2 + f2] < 0;   // :804-808
    double X[3] = {0, 0, 0}, mse = 0.0;
    if (cand) {
      const size_t r1 = (size_t)e.kp1 + f1, r2 = (size_t)e.kp2 + f2;
      View V[2];
      V[0].R = s_cam; V[0].t = s_cam + 9; V[0].c = s_cam + 12; V[0].fk = s_cam + 15;
      V[0].x = (double)kp[2 * r1]; V[0].y = (double)kp[2 * r1 + 1];
      V[1].R = s_cam + NP_CAM; V[1].t = s_cam + NP_CAM + 9; V[1].c = s_cam + NP_CAM + 12; V[1].fk = s_cam + NP_CAM + 15;
      V[1].x = (double)kp[2 * r2]; V[1].y = (double)kp[2 * r2 + 1];
      ok = tri_two_views(V, th_error, e.large ? cos_large : cos_small, X, &mse);
    }
    unsigned kk = sentinel;
    // sqrt(mse) <= th_error < 46340: the conversion is defined and below the sentinel; a NaN (non-finite input, outside
    // the contract of msfm.h) sorts first
    if (ok) kk = mse == mse ? (unsigned)(int)mse : 0u;
    key[m] = ((unsigned long long)e.k << key_bits) | kk;
    val[m] = (int)m;
    Xall[3 * m] = X[0]; Xall[3 * m + 1] = X[1]; Xall[3 * m + 2] = X[2];
    mse_all[m] = mse;
  }
  // a workgroup lies inside one entry: one add per wave and count
  const unsigned long long bc = __ballot(cand), ba = __ballot(ok);
  if ((threadIdx.x & 63) == 0) {
    if (bc) atomicAdd(&n_cand[q], __popcll(bc));
    if (ba) atomicAdd(&n_acc[q], __popcll(ba));
  }
}

__global__ __launch_bounds__(256) void k_claim(int M, int E, const int* __restrict__ off_all, const Ent* __restrict__ ent, const int* __restrict__ matches,
                                                const unsigned long long* __restrict__ key_s, const int* __restrict__ val_s, unsigned sentinel,
                                                unsigned key_mask, int* __restrict__ slot) {
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= M) return;
  if (((unsigned)key_s[p] & key_mask) == sentinel) return;
  const int w = val_s[p];
  const int q = csr_segment_of(off_all, E, w);
  const Ent e = ent[q];
  const size_t sm = (size_t)e.m0 + (w - off_all[q]);
  atomicMin(&slot[(size_t)e.slot1 + matches[2 * sm]], p);       // std::map::insert: the earliest position keeps the key
  atomicMin(&slot[(size_t)e.slot2 + matches[2 * sm + 1]], p);
}

__global__ __launch_bounds__(256) void k_emit(int M, int E, const int* __restrict__ off_all, const Ent* __restrict__ ent, const int* __restrict__ matches,
                                               const unsigned long long* __restrict__ key_s, const int* __restrict__ val_s, unsigned sentinel,
                                               unsigned key_mask, const int* __restrict__ slot, const double* __restrict__ Xall,
                                               const double* __restrict__ mse_all, int* __restrict__ out_w, int* __restrict__ feat1,
                                               int* __restrict__ feat2, double* __restrict__ X, double* __restrict__ mse, uint8_t* __restrict__ takes1,
                                               uint8_t* __restrict__ takes2) {
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= M) return;
  if (((unsigned)key_s[p] & key_mask) == sentinel) return;
  const int w = val_s[p];
  const int q = csr_segment_of(off_all, E, w);
  const Ent e = ent[q];
  const size_t sm = (size_t)e.m0 + (w - off_all[q]);
  const int f1 = matches[2 * sm], f2 = matches[2 * sm + 1];
  out_w[p] = w; feat1[p] = f1; feat2[p] = f2;
  X[3 * (size_t)p] = Xall[3 * (size_t)w]; X[3 * (size_t)p + 1] = Xall[3 * (size_t)w + 1]; X[3 * (size_t)p + 2] = Xall[3 * (size_t)w + 2];
  mse[p] = mse_all[w];
  takes1[p] = slot[(size_t)e.slot1 + f1] == p ? 1 : 0;
  takes2[p] = slot[(size_t)e.slot2 + f2] == p ? 1 : 0;
}

}  // namespace newpts

#define NP_TRY(e) HIP_TRY(ctx, (e))

MSFM_API void msfm_new_points_default_options(msfm_new_points_options* o) {
  if (!o) return;
  o->th_mse_reprojection = 3.0;
  o->th_angle_small = 3.0 / 180.0 * 3.1415;
  o->th_angle_large = 5.0 / 180.0 * 3.1415;
  o->th_matches_large = 500;
}

// The checks and O(cameras + visible entries) on the host: the walk and the rows of the involved cameras.  fp_resident: the
// feat_point row of camera c starts at its offset in the whole array (a resident state) instead of in a packed upload;
// kp_mode: where a camera's keypoint rows start (NP_KP_*).  R gets its per-entry tables.
int newpoints_plan(msfm_ctx* ctx, const char* who, const msfm_match_store* S, const NewPointsArgs& P, const msfm_new_points_options& opt,
                   bool fp_resident, int kp_mode, NewPointsPlan* L, msfm_new_points_set* R) {
  const int ni = S->n_images, nc = P.n_cams, nn = P.n_new;
  if (opt.th_mse_reprojection != opt.th_mse_reprojection || opt.th_angle_small != opt.th_angle_small || opt.th_angle_large != opt.th_angle_large)
    return msfm_set_error(ctx, MSFM_E_INVAL, "%s: a threshold is NaN", who);
  if (!(opt.th_mse_reprojection >= 0.0) || !(opt.th_mse_reprojection < 46340.0))
    return msfm_set_error(ctx, MSFM_E_INVAL, "%s: th_mse_reprojection = %g outside [0, 46340): the sort key is an int of a value up to its square", who,
                          opt.th_mse_reprojection);
  if (opt.th_matches_large < 0) return msfm_set_error(ctx, MSFM_E_INVAL, "%s: th_matches_large < 0", who);
  // ---- O(cameras + visible entries) on the host ----
  std::vector<int>& cam_fo = L->cam_fo;
  cam_fo.assign(nc + 1, 0);
  {
    std::vector<uint8_t> seen(std::max(1, ni), 0);
    for (int c = 0; c < nc; c++) {
      const int im = P.cam_img[c];
      if (im < 0 || im >= ni) return msfm_set_error(ctx, MSFM_E_INVAL, "%s: cam_img[%d] = %d is no image of the store", who, c, im);
      if (seen[im]) return msfm_set_error(ctx, MSFM_E_INVAL, "%s: image %d has two cameras", who, im);
      seen[im] = 1;
      if ((long)cam_fo[c] + S->n_features[im] > 0x7fffffffL) return msfm_set_error(ctx, MSFM_E_INVAL, "%s: more than 2^31 registered features", who);
      cam_fo[c + 1] = cam_fo[c] + S->n_features[im];
    }
  }
  if (nn) MSFM_TRY(msfm_check_offsets(ctx, who, nn, P.vis_off));
  const int E = nn ? P.vis_off[nn] : 0;
  if (E && !P.vis_cam) return msfm_set_error(ctx, MSFM_E_INVAL, "%s: null vis_cam", who);
  R->n_new = nn; R->n_entries = E;
  R->pt_off.assign(nn + 1, 0);
  R->n_matches.assign(E, 0); R->n_candidates.assign(E, 0); R->n_accepted.assign(E, 0); R->large.assign(E, 0);
  L->nn = nn; L->E = E;
  std::vector<NewPointsEnt>& ent = L->ent;
  ent.assign(E, NewPointsEnt());
  std::vector<int>&off_all = L->off_all, &blk_off = L->blk_off, &cam_off = L->cam_off, &involved = L->involved, &fp_base = L->fp_base, &kp_base = L->kp_base;
  off_all.assign(E + 1, 0); blk_off.assign(E + 1, 0); cam_off.assign(nn + 1, 0);
  involved.clear(); fp_base.clear(); kp_base.clear();
  std::vector<int> row_of_cam(std::max(1, nc), -1);   // camera -> row of the uploaded tables
  std::vector<int> slot_stamp(std::max(1, nc), -1), slot_of(std::max(1, nc), 0);
  long fp_rows = 0, kp_rows = 0, n_slots = 0;
  auto involve = [&](int c) -> int {   // 0, or the image without keypoints + 1
    if (row_of_cam[c] >= 0) return 0;
    const int im = P.cam_img[c];
    if (kp_mode == NP_KP_STORE && !S->has_kp[im]) return im + 1;
    row_of_cam[c] = (int)involved.size();
    involved.push_back(c);
    if (fp_resident) fp_base.push_back(cam_fo[c]);
    else fp_base.push_back((int)fp_rows);
    fp_rows += S->n_features[im];
    if (kp_mode == NP_KP_PACKED) { kp_base.push_back((int)kp_rows); kp_rows += S->n_features[im]; }
    else kp_base.push_back(S->feat_off[im]);
    return 0;
  };
  for (int k = 0; k < nn; k++) {
    const int c1 = P.new_cam[k];
    if (c1 < 0 || c1 >= nc) return msfm_set_error(ctx, MSFM_E_INVAL, "%s: new_cam[%d] = %d outside n_cams = %d", who, k, c1, nc);
    for (int q = P.vis_off[k]; q < P.vis_off[k + 1]; q++)
      if (P.vis_cam[q] < 0 || P.vis_cam[q] >= nc)
        return msfm_set_error(ctx, MSFM_E_INVAL, "%s: vis_cam[%d] = %d outside n_cams = %d", who, q, P.vis_cam[q], nc);
    const int i1 = P.cam_img[c1];
    if (int bad = involve(c1)) return msfm_set_error(ctx, MSFM_E_INVAL, "%s: no keypoints of image %d (argument or chain)", who, bad - 1);
    auto slots = [&](int c) {   // the claim slots of camera c inside new camera k's table
      if (slot_stamp[c] != k) { slot_stamp[c] = k; slot_of[c] = (int)n_slots; n_slots += S->n_features[P.cam_img[c]]; }
      return slot_of[c];
    };
    const int s1 = slots(c1);
    cam_off[k] = off_all[P.vis_off[k]];
    for (int q = P.vis_off[k]; q < P.vis_off[k + 1]; q++) {
      const int c2 = P.vis_cam[q];
      int m0 = 0, cnt = 0;
      if (c2 != c1) {   // :769
        const int i2 = P.cam_img[c2];
        for (int p = S->row_off[i1]; p < S->row_off[i1 + 1]; p++)   // QueryMatch(i1, i2): row i1, entry i2
          if (S->pair_img[2 * p + 1] == i2) { m0 = S->match_off[p]; cnt = S->match_off[p + 1] - m0; break; }
        if (int bad = involve(c2)) return msfm_set_error(ctx, MSFM_E_INVAL, "%s: no keypoints of image %d (argument or chain)", who, bad - 1);
      }
      const int large = cnt > opt.th_matches_large ? 1 : 0;   // :780-784
      const int r2 = c2 != c1 ? row_of_cam[c2] : row_of_cam[c1];
      ent[q] = NewPointsEnt{m0, fp_base[row_of_cam[c1]], fp_base[r2], kp_base[row_of_cam[c1]], kp_base[r2], row_of_cam[c1], r2, s1,
                            c2 != c1 ? slots(c2) : s1, k, large};
      R->n_matches[q] = cnt; R->large[q] = (uint8_t)large;
      if ((long)off_all[q] + cnt > 0x7fffffffL) return msfm_set_error(ctx, MSFM_E_INVAL, "%s: more than 2^31 matches in one call", who);
      off_all[q + 1] = off_all[q] + cnt;
      blk_off[q + 1] = blk_off[q] + cdiv(cnt, 256);
    }
    if (fp_rows > 0x7fffffffL || kp_rows > 0x7fffffffL || n_slots > 0x7fffffffL)
      return msfm_set_error(ctx, MSFM_E_INVAL, "%s: more than 2^31 features of involved cameras", who);
  }
  cam_off[nn] = off_all[E];
  L->M = off_all[E];
  L->fp_rows = fp_rows; L->kp_rows = kp_rows; L->n_slots = n_slots;
  return MSFM_OK;
}

// The kernels of the call on device arrays: the walk's tables go up, k_tri / sort / k_claim / k_emit run, the result block
// W->d_out is left on the device.  No synchronisation: W belongs to the caller, who declares it in front of the scope `sc`.
int newpoints_dev(msfm_ctx* ctx, const msfm_match_store* S, const NewPointsArgs& P, const NewPointsPlan& L, const msfm_new_points_options& opt,
                  const int* d_fp, const float* d_kp, DevScope& sc, NewPointsDev* W) {
  using namespace newpts;
  const int E = L.E, M = L.M, nn = L.nn;
  // the sentinel of a match that yields no point sorts behind every (int)mse: sqrt(mse) <= th gives mse <= th^2 (1 + 2^-52)
  const unsigned sentinel = (unsigned)(opt.th_mse_reprojection * opt.th_mse_reprojection) + 2u;
  const int key_bits = bits_for(sentinel), cam_bits = nn > 1 ? bits_for((unsigned)(nn - 1)) : 0;
  const unsigned key_mask = key_bits >= 32 ? 0xffffffffu : ((1u << key_bits) - 1u);
  hipStream_t s = ctx->stream;
  const int ninv = (int)L.involved.size();
  std::vector<double> cam(NP_CAM * (size_t)ninv);
  for (int r = 0; r < ninv; r++) {
    const size_t c = (size_t)L.involved[r];
    double* C = cam.data() + NP_CAM * (size_t)r;
    std::copy(P.cam_R + 9 * c, P.cam_R + 9 * c + 9, C);
    std::copy(P.cam_t + 3 * c, P.cam_t + 3 * c + 3, C + 9);
    std::copy(P.cam_c + 3 * c, P.cam_c + 3 * c + 3, C + 12);
    std::copy(P.cam_fk + 3 * c, P.cam_fk + 3 * c + 3, C + 15);
  }
  NP_TRY(sc.up(W->d_ent, L.ent.data(), (size_t)E)); NP_TRY(sc.up(W->d_offa, L.off_all.data(), (size_t)E + 1)); NP_TRY(sc.up(W->d_blk, L.blk_off.data(), (size_t)E + 1));
  NP_TRY(sc.up(W->d_cam, cam));
  const size_t Mx = (size_t)M;
  NP_TRY(W->d_key.alloc(Mx)); NP_TRY(W->d_key_s.alloc(Mx)); NP_TRY(W->d_val.alloc(Mx)); NP_TRY(W->d_val_s.alloc(Mx));
  NP_TRY(W->d_Xall.alloc(3 * Mx)); NP_TRY(W->d_mseall.alloc(Mx));
  NP_TRY(W->d_slot.alloc((size_t)std::max(1L, L.n_slots)));
  // everything that goes back to the host in ONE block, widest elements first: X [M][3], mse [M] | w, f1, f2 [M], the two
  // counts [E] | takes1, takes2 [M] - 46 bytes per match of the walk and 8 per entry, one copy
  const size_t Ex = (size_t)E;
  W->o_mse = 24 * Mx; W->o_w = 32 * Mx; W->o_f1 = W->o_w + 4 * Mx; W->o_f2 = W->o_f1 + 4 * Mx; W->o_nc = W->o_f2 + 4 * Mx; W->o_na = W->o_nc + 4 * Ex;
  W->o_t1 = W->o_na + 4 * Ex; W->o_t2 = W->o_t1 + Mx; W->out_bytes = W->o_t2 + Mx;
  NP_TRY(W->d_out.alloc(W->out_bytes));
  double* d_X = (double*)W->d_out.p;
  double* d_mse = (double*)(W->d_out.p + W->o_mse);
  int* d_w = (int*)(W->d_out.p + W->o_w);
  int* d_f1 = (int*)(W->d_out.p + W->o_f1);
  int* d_f2 = (int*)(W->d_out.p + W->o_f2);
  int* d_ncand = (int*)(W->d_out.p + W->o_nc);
  int* d_nacc = (int*)(W->d_out.p + W->o_na);
  uint8_t* d_t1 = (uint8_t*)(W->d_out.p + W->o_t1);
  uint8_t* d_t2 = (uint8_t*)(W->d_out.p + W->o_t2);
  NP_TRY(hipMemsetAsync(d_ncand, 0, sizeof(int) * 2 * Ex, s));
  if (L.n_slots) NP_TRY(hipMemsetD32Async((hipDeviceptr_t)W->d_slot.p, NP_BIG, (size_t)L.n_slots, s));
  {
    KTimer tm(ctx, "newpoints_triangulate");
    hipLaunchKernelGGL(k_tri, dim3(L.blk_off[E]), dim3(256), 0, s, E, W->d_blk.p, W->d_offa.p, W->d_ent.p, S->d_match.p, d_fp, d_kp, W->d_cam.p,
                       opt.th_mse_reprojection, cos(opt.th_angle_small), cos(opt.th_angle_large), sentinel, key_bits, W->d_key.p, W->d_val.p, W->d_Xall.p,
                       W->d_mseall.p, d_ncand, d_nacc);
  }
  NP_TRY(hipGetLastError());
  {
    KTimer tm(ctx, "newpoints_sort");
    NP_TRY(prim_sort_pairs(W->tmp, W->d_key.p, W->d_key_s.p, W->d_val.p, W->d_val_s.p, Mx, 0u, (unsigned)(key_bits + cam_bits), s));
  }
  {
    KTimer tm(ctx, "newpoints_claim");
    tm.count = 2;
    hipLaunchKernelGGL(k_claim, dim3(cdiv(M, 256)), dim3(256), 0, s, M, E, W->d_offa.p, W->d_ent.p, S->d_match.p, W->d_key_s.p, W->d_val_s.p, sentinel, key_mask,
                       W->d_slot.p);
    hipLaunchKernelGGL(k_emit, dim3(cdiv(M, 256)), dim3(256), 0, s, M, E, W->d_offa.p, W->d_ent.p, S->d_match.p, W->d_key_s.p, W->d_val_s.p, sentinel, key_mask,
                       W->d_slot.p, W->d_Xall.p, W->d_mseall.p, d_w, d_f1, d_f2, d_X, d_mse, d_t1, d_t2);
  }
  NP_TRY(hipGetLastError());
  return MSFM_OK;
}

// The result block on the host (hb, after the wait) into the set: the host closes the gaps between the new cameras
void newpoints_collect(const NewPointsArgs& P, const NewPointsPlan& L, const NewPointsDev& W, const char* hb, msfm_new_points_set* R) {
  const int nn = L.nn;
  const size_t Ex = (size_t)L.E;
  const std::vector<int>& off_all = L.off_all;
  const double* X = (const double*)hb;
  const double* mse = (const double*)(hb + W.o_mse);
  const int* w = (const int*)(hb + W.o_w);
  const int* f1 = (const int*)(hb + W.o_f1);
  const int* f2 = (const int*)(hb + W.o_f2);
  const uint8_t* t1 = (const uint8_t*)(hb + W.o_t1);
  const uint8_t* t2 = (const uint8_t*)(hb + W.o_t2);
  std::copy((const int*)(hb + W.o_nc), (const int*)(hb + W.o_nc) + Ex, R->n_candidates.begin());
  std::copy((const int*)(hb + W.o_na), (const int*)(hb + W.o_na) + Ex, R->n_accepted.begin());
  for (int k = 0; k < nn; k++) {
    int cnt = 0;
    for (int q = P.vis_off[k]; q < P.vis_off[k + 1]; q++) cnt += R->n_accepted[q];
    R->pt_off[k + 1] = R->pt_off[k] + cnt;
  }
  const size_t T = (size_t)R->pt_off[nn];
  R->cam2.resize(T); R->feat1.resize(T); R->feat2.resize(T); R->vis_entry.resize(T); R->pt_match.resize(T);
  R->X.resize(3 * T); R->mse.resize(T); R->takes1.resize(T); R->takes2.resize(T);
  for (int k = 0; k < nn; k++) {
    const size_t b = (size_t)L.cam_off[k], e0 = (size_t)R->pt_off[k], cnt = (size_t)(R->pt_off[k + 1] - R->pt_off[k]);
    const int* ob = off_all.data() + P.vis_off[k];
    const int* oe = off_all.data() + P.vis_off[k + 1] + 1;
    for (size_t i = 0; i < cnt; i++) {
      const int q = (int)(std::upper_bound(ob, oe, w[b + i]) - off_all.data()) - 1;   // the entry of that walk position
      R->cam2[e0 + i] = P.vis_cam[q];
      R->vis_entry[e0 + i] = q - P.vis_off[k];
      R->pt_match[e0 + i] = w[b + i] - off_all[q];
    }
    std::copy(f1 + b, f1 + b + cnt, R->feat1.begin() + e0);
    std::copy(f2 + b, f2 + b + cnt, R->feat2.begin() + e0);
    std::copy(X + 3 * b, X + 3 * (b + cnt), R->X.begin() + 3 * e0);
    std::copy(mse + b, mse + b + cnt, R->mse.begin() + e0);
    std::copy(t1 + b, t1 + b + cnt, R->takes1.begin() + e0);
    std::copy(t2 + b, t2 + b + cnt, R->takes2.begin() + e0);
  }
}

MSFM_API int msfm_new_points(msfm_ctx* ctx, const msfm_match_store* S, const msfm_new_points_problem* P, const msfm_new_points_options* opt_in,
                             msfm_new_points_set** out) {
  const char* who = "msfm_new_points";
  if (!ctx) return MSFM_E_INVAL;
  if (!S || !P || !out) return msfm_set_error(ctx, MSFM_E_INVAL, "%s: null argument", who);
  *out = nullptr;
  if (S->ctx != ctx) return msfm_set_error(ctx, MSFM_E_INVAL, "%s: the store belongs to another context", who);
  msfm_new_points_options opt;
  if (opt_in) opt = *opt_in; else msfm_new_points_default_options(&opt);
  const int nc = P->n_cams, nn = P->n_new;
  if (nn < 0 || nn > 65535) return msfm_set_error(ctx, MSFM_E_INVAL, "%s: n_new = %d outside [0, 65535]", who, nn);
  if (nc < 0 || P->n_points < 0) return msfm_set_error(ctx, MSFM_E_INVAL, "%s: negative count", who);
  if ((nc && (!P->cam_img || !P->cam_R || !P->cam_t || !P->cam_c || !P->cam_fk)) || (nn && (!P->new_cam || !P->vis_off)))
    return msfm_set_error(ctx, MSFM_E_INVAL, "%s: null array", who);
  NewPointsArgs A;
  A.n_cams = nc; A.cam_img = P->cam_img; A.cam_R = P->cam_R; A.cam_t = P->cam_t; A.cam_c = P->cam_c; A.cam_fk = P->cam_fk;
  A.n_new = nn; A.new_cam = P->new_cam; A.vis_off = P->vis_off; A.vis_cam = P->vis_cam;
  std::unique_ptr<msfm_new_points_set> R(new msfm_new_points_set());
  NewPointsPlan L;
  MSFM_TRY(newpoints_plan(ctx, who, S, A, opt, /*fp_resident=*/false, P->keypoints ? NP_KP_PACKED : NP_KP_STORE, &L, R.get()));
  if (L.fp_rows && !P->feat_point) return msfm_set_error(ctx, MSFM_E_INVAL, "%s: null feat_point", who);
  if (L.M == 0) { *out = R.release(); return MSFM_OK; }   // (also n_new = 0 and empty visible lists)
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  NewPointsDev W;
  DevBuf<int> d_fp;
  DevBuf<float> d_kp_up;
  DevScope sc(ctx);
  // the rows of the involved cameras only, packed on the host: one copy per table instead of one per camera
  const int ninv = (int)L.involved.size();
  std::vector<int> h_fp((size_t)L.fp_rows);
  std::vector<float> h_kp(P->keypoints ? 2 * (size_t)L.kp_rows : 0);
  for (int r = 0; r < ninv; r++) {
    const int c = L.involved[r], im = P->cam_img[c];
    const size_t cnt = (size_t)S->n_features[im];
    if (!cnt) continue;
    std::copy(P->feat_point + L.cam_fo[c], P->feat_point + L.cam_fo[c] + cnt, h_fp.begin() + L.fp_base[r]);
    if (P->keypoints)
      std::copy(P->keypoints + 2 * (size_t)S->feat_off[im], P->keypoints + 2 * ((size_t)S->feat_off[im] + cnt), h_kp.begin() + 2 * (size_t)L.kp_base[r]);
  }
  NP_TRY(sc.up(d_fp, h_fp));
  if (P->keypoints) NP_TRY(sc.up(d_kp_up, h_kp));
  MSFM_TRY(newpoints_dev(ctx, S, A, L, opt, d_fp.p, P->keypoints ? d_kp_up.p : S->d_kp.p, sc, &W));
  // ---- one read-back: the two counts per entry and the point arrays at the capacity of the walk (M is known here, the
  //      accepted counts are not) ----
  std::vector<double> h_out((W.out_bytes + 7) / 8);   // (doubles: the block's alignment)
  NP_TRY(hipMemcpyAsync(h_out.data(), W.d_out.p, W.out_bytes, hipMemcpyDeviceToHost, s));
  NP_TRY(sc.finish());   // the scratch above is released on return
  newpoints_collect(A, L, W, (const char*)h_out.data(), R.get());
  R->h2d_bytes = sc.h2d;
  *out = R.release();
  return MSFM_OK;
}

MSFM_API int msfm_new_points_set_size(const msfm_new_points_set* R, int* n_new, int* n_points, int* n_entries, int64_t* h2d_bytes) {
  if (!R) return MSFM_E_INVAL;
  if (n_new) *n_new = R->n_new;
  if (n_points) *n_points = R->pt_off[R->n_new];
  if (n_entries) *n_entries = R->n_entries;
  if (h2d_bytes) *h2d_bytes = R->h2d_bytes;
  return MSFM_OK;
}

MSFM_API int msfm_new_points_set_fetch(const msfm_new_points_set* R, int* pt_off, int* cam2, int* feat1, int* feat2, int* vis_entry, int* pt_match,
                                       double* X, double* mse, uint8_t* takes1, uint8_t* takes2, int* n_matches, uint8_t* large, int* n_candidates,
                                       int* n_accepted) {
  if (!R) return MSFM_E_INVAL;
  if (pt_off) std::copy(R->pt_off.begin(), R->pt_off.end(), pt_off);
  if (cam2) std::copy(R->cam2.begin(), R->cam2.end(), cam2);
  if (feat1) std::copy(R->feat1.begin(), R->feat1.end(), feat1);
  if (feat2) std::copy(R->feat2.begin(), R->feat2.end(), feat2);
  if (vis_entry) std::copy(R->vis_entry.begin(), R->vis_entry.end(), vis_entry);
  if (pt_match) std::copy(R->pt_match.begin(), R->pt_match.end(), pt_match);
  if (X) std::copy(R->X.begin(), R->X.end(), X);
  if (mse) std::copy(R->mse.begin(), R->mse.end(), mse);
  if (takes1) std::copy(R->takes1.begin(), R->takes1.end(), takes1);
  if (takes2) std::copy(R->takes2.begin(), R->takes2.end(), takes2);
  if (n_matches) std::copy(R->n_matches.begin(), R->n_matches.end(), n_matches);
  if (large) std::copy(R->large.begin(), R->large.end(), large);
  if (n_candidates) std::copy(R->n_candidates.begin(), R->n_candidates.end(), n_candidates);
  if (n_accepted) std::copy(R->n_accepted.begin(), R->n_accepted.end(), n_accepted);
  return MSFM_OK;
}

MSFM_API void msfm_new_points_set_destroy(msfm_new_points_set* R) { delete R; }
