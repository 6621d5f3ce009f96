// The tries of one localisation round: the loop of IncrementalSfM::Run (SfM/src/sfm_incremental.cc:143-164) around
//   IncrementalSfM::LocalizeImage            SfM/src/sfm_incremental.cc:565-753
// for the ranked rows of a msfm_localize_set in one call.  The set keeps corr_point / pts_w / pts_2d on the device
// (localize.hip), so no correspondence crosses PCIe on the way in, and the host waits once.
//
// A failed try returns at :670 / :701 having touched nothing but localize_fail_times_, so the rows are independent.  As in
// seed.hip each arm gets an offset array over all n_kept rows in which the rows of the other arm and the untried rows are
// empty: the row index stays the problem index, hence the sampler index, of pose_epnp_dev / pose_epnpf_dev (pose.hip).
//   k_gather   one thread per correspondence of the tried rows: pts_w / pts_2d from the resident set into its arm's buffers
//   (pose_epnp_dev, pose_epnpf_dev: the launches of the two public absolute-pose calls)
//   k_rows     one thread per tried row: its arm's record into the per-row outputs, pass = !(avg_error > th)    :648 / :679
//   k_first    one thread per correspondence of the passing rows: an inlier (!(error > avg_error), :713) whose point is not
//              pt_new_added does atomicMin of its position into the slot of (tried row, point) - the first inlier of the walk
//              that names the point is the one `if (!is_new_added_)` lets through (:721), the pattern of k_resolve
//   k_state    the same threads: errors back into the layout of corr_off, the state of :709-729, the two counts (a wave
//              ballot + one integer atomicAdd where a wave lies inside one row)
// Integer atomics only; nothing depends on the order in which threads run.  Scratch: tried rows x n_points integers.
#include <climits>
#include <memory>

#include "common.h"

#define LP_BIG 0x7fffffff


namespace lpose {

// a tried row: its row of the set, its first correspondence there, its first entry in its arm's buffers, its count, its arm
struct Slot { int row, src0, dst0, n, arm; };

// the tried row of entry e of the tried rows' concatenation: last s with toff[s] <= e (rows with no entry are skipped by the
// strict ascent of the others; an empty tried row cannot exist: a tried row has >= 3 entries)
__device__ static inline int slot_of(const int* __restrict__ toff, int nt, int e) {
  int lo = 0, hi = nt;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (toff[mid] <= e) lo = mid; else hi = mid;
  }
  return lo;
}

__global__ __launch_bounds__(256) void k_gather(int E, int nt, const int* __restrict__ toff, const Slot* __restrict__ slot,
                                                 const double* __restrict__ pw, const double* __restrict__ p2, double* __restrict__ w1,
                                                 double* __restrict__ x1, double* __restrict__ w2, double* __restrict__ x2) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= E) return;
  const int s = slot_of(toff, nt, e);
  const Slot S = slot[s];
  const size_t i = (size_t)S.src0 + (e - toff[s]), o = (size_t)S.dst0 + (e - toff[s]);
  double* w = S.arm == 1 ? w1 : w2;
  double* x = S.arm == 1 ? x1 : x2;
  w[3 * o] = pw[3 * i]; w[3 * o + 1] = pw[3 * i + 1]; w[3 * o + 2] = pw[3 * i + 2];
  x[2 * o] = p2[2 * i]; x[2 * o + 1] = p2[2 * i + 1];
}

struct ArmOut { const double *f, *R, *t, *avg; const int *bstep, *biter; };   // [n_kept] records of one arm; f / bstep may be null

__global__ __launch_bounds__(64) void k_rows(int nt, const Slot* __restrict__ slot, ArmOut a1, ArmOut a2, const double* __restrict__ row_f,
                                              double th, double* __restrict__ f, double* __restrict__ R, double* __restrict__ t,
                                              double* __restrict__ avg, int* __restrict__ bstep, int* __restrict__ biter,
                                              uint8_t* __restrict__ pass) {
  const int s = blockIdx.x * 64 + threadIdx.x;
  if (s >= nt) return;
  const Slot S = slot[s];
  const ArmOut A = S.arm == 1 ? a1 : a2;
  const size_t r = (size_t)S.row;
  f[r] = S.arm == 1 ? row_f[r] : A.f[r];          // :703 on the sweep arm
  for (int i = 0; i < 9; i++) R[9 * r + i] = A.R[9 * r + i];
  for (int i = 0; i < 3; i++) t[3 * r + i] = A.t[3 * r + i];
  const double a = A.avg[r];
  avg[r] = a;
  bstep[r] = S.arm == 1 ? -1 : A.bstep[r];
  biter[r] = A.biter[r];
  pass[r] = !(a > th);                            // :648 / :679 negated: a NaN passes
}

__global__ __launch_bounds__(256) void k_first(int E, int nt, const int* __restrict__ toff, const Slot* __restrict__ slot,
                                                const double* __restrict__ err1, const double* __restrict__ err2, const double* __restrict__ avg,
                                                const uint8_t* __restrict__ pass, const int* __restrict__ cp, int n_points,
                                                const uint8_t* __restrict__ added, int* __restrict__ first) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= E) return;
  const int s = slot_of(toff, nt, e);
  const Slot S = slot[s];
  if (!pass[S.row]) return;
  const int i = e - toff[s];
  const double er = (S.arm == 1 ? err1 : err2)[(size_t)S.dst0 + i];
  if (er > avg[S.row]) return;                                               // :713
  const int p = cp[(size_t)S.src0 + i];                                      // (< n_points: checked on the host)
  if (added && added[p]) return;
  atomicMin(&first[(size_t)s * n_points + p], i);
}

__global__ __launch_bounds__(256) void k_state(int E, int nt, const int* __restrict__ toff, const Slot* __restrict__ slot,
                                                const double* __restrict__ err1, const double* __restrict__ err2, const double* __restrict__ avg,
                                                const uint8_t* __restrict__ pass, const int* __restrict__ cp, int n_points,
                                                const uint8_t* __restrict__ added, const int* __restrict__ first, double* __restrict__ errors,
                                                uint8_t* __restrict__ state, int* __restrict__ n_in, int* __restrict__ n_out) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  const bool in = e < E;
  int s = 0, row = 0, st = 0;
  if (in) {
    s = slot_of(toff, nt, e);
    const Slot S = slot[s];
    row = S.row;
    const int i = e - toff[s];
    const double er = (S.arm == 1 ? err1 : err2)[(size_t)S.dst0 + i];
    errors[(size_t)S.src0 + i] = er;
    if (pass[row]) {
      const int p = cp[(size_t)S.src0 + i];
      if (er > avg[row]) st = 1;
      else if (!(added && added[p]) && first[(size_t)s * n_points + p] == i) st = 2;
      else st = 3;
    }
    state[(size_t)S.src0 + i] = (uint8_t)st;
  }
  const int s0 = __shfl(s, 0);
  if (__all(!in || s == s0)) {
    const unsigned long long b2 = __ballot(st == 2), b1 = __ballot(st == 1);
    const int row0 = __shfl(row, 0);
    if ((threadIdx.x & 63) == 0) {
      if (b2) atomicAdd(&n_in[row0], __popcll(b2));
      if (b1) atomicAdd(&n_out[row0], __popcll(b1));
    }
  } else if (st == 2) {
    atomicAdd(&n_in[row], 1);
  } else if (st == 1) {
    atomicAdd(&n_out[row], 1);
  }
}

}  // namespace lpose

#define LP_TRY(e) HIP_TRY(ctx, (e))

MSFM_API void msfm_localize_pose_default_options(msfm_localize_pose_options* o) {
  if (!o) return;
  o->th_mse_localization = 5.0;
  o->th_min_2d3d_corres = 20;
  o->max_iter = 200;
  o->seed = 0x4D53464D50ull;
  msfm_epnpf_default_options(&o->sweep);
  o->first_row = 0;
  o->max_tries = 16;
}

// The call with pt_new_added optionally on the device (d_added, a resident state's: nothing is uploaded for it then) and, with
// keep_state, the corr_state array [n_corr] handed to the caller on the device as well; h2d_bytes (optional) is incremented at
// every upload.  msfm_localize_poses is this with none of the three.
int localize_poses_dev(msfm_ctx* ctx, const char* who, const msfm_localize_set* L, const double* row_f, const double* row_f_init, int n_points,
                       const uint8_t* pt_new_added, const uint8_t* d_added_dev, const msfm_localize_pose_options* opt_in, msfm_localize_pose_set** out,
                       DevBuf<uint8_t>* keep_state, int64_t* h2d_bytes) {
  using namespace lpose;
  if (!ctx) return MSFM_E_INVAL;
  if (!L || !out) return msfm_set_error(ctx, MSFM_E_INVAL, "%s: null argument", who);
  *out = nullptr;
  if (L->ctx != ctx) return msfm_set_error(ctx, MSFM_E_INVAL, "%s: the set belongs to another context", who);
  if (!L->have_pts) return msfm_set_error(ctx, MSFM_E_INVAL, "%s: the set was made without point_xyz: it holds no points", who);
  msfm_localize_pose_options opt;
  if (opt_in) opt = *opt_in; else msfm_localize_pose_default_options(&opt);
  const int n = (int)L->rank.size(), T = (int)L->corr_point.size();
  if (n && !row_f) return msfm_set_error(ctx, MSFM_E_INVAL, "%s: null row_f", who);
  if (n_points < 0) return msfm_set_error(ctx, MSFM_E_INVAL, "%s: n_points < 0", who);
  if (opt.first_row < 0) return msfm_set_error(ctx, MSFM_E_INVAL, "%s: first_row < 0", who);
  if (opt.max_tries < 0) return msfm_set_error(ctx, MSFM_E_INVAL, "%s: max_tries < 0", who);
  if (opt.max_iter < 1 || opt.max_iter > 65536) return msfm_set_error(ctx, MSFM_E_INVAL, "%s: max_iter out of range", who);
  if (!(opt.sweep.f_ratio_step > 0.0) || !(opt.sweep.f_ratio_max > opt.sweep.f_ratio_min))
    return msfm_set_error(ctx, MSFM_E_INVAL, "%s: sweep needs f_ratio_step > 0 and f_ratio_max > f_ratio_min", who);
  const int n_steps = msfm_epnpf_num_steps(&opt.sweep);
  if (n_steps < 1) return msfm_set_error(ctx, MSFM_E_INVAL, "%s: the sweep options give a step count outside 1..65535", who);
  if (opt.sweep.max_iter < 1 || opt.sweep.max_iter > 65536) return msfm_set_error(ctx, MSFM_E_INVAL, "%s: sweep.max_iter out of range", who);
  if (n > 65535) return msfm_set_error(ctx, MSFM_E_INVAL, "%s: at most 65535 rows per call", who);
  int max_pt = -1;
  for (int p : L->corr_point) max_pt = std::max(max_pt, p);
  if (max_pt >= n_points) return msfm_set_error(ctx, MSFM_E_INVAL, "%s: the set holds point %d, n_points = %d", who, max_pt, n_points);
  for (int r = 0; r < n; r++)
    if (!(row_f[r] >= 0.0)) return msfm_set_error(ctx, MSFM_E_INVAL, "%s: row_f[%d] is negative or NaN", who, r);
  // ---- O(rows) on the host: which rows are tried, the two arms' CSRs, the tried rows' own CSR ----
  std::unique_ptr<msfm_localize_pose_set> R(new msfm_localize_pose_set());
  R->n = n; R->n_corr = T;
  R->tried.assign(n, 0); R->arm.assign(n, 0); R->pass.assign(n, 0); R->state.assign(T, 0);
  R->f.assign(n, 0.0); R->R.assign(9 * (size_t)n, 0.0); R->t.assign(3 * (size_t)n, 0.0); R->avg.assign(n, 0.0); R->errors.assign(T, 0.0);
  R->best_step.assign(n, 0); R->best_iter.assign(n, 0); R->n_in.assign(n, 0); R->n_out.assign(n, 0);
  auto eligible = [&](int r) {
    const int c = L->corr_off[r + 1] - L->corr_off[r];
    return c >= opt.th_min_2d3d_corres && c >= 3;   // :148, :567
  };
  std::vector<Slot> slot;
  std::vector<int> off1(n + 1, 0), off2(n + 1, 0), toff(1, 0);
  std::vector<double> f_init(n, 0.0);
  int last = -1;
  for (int r = 0; r < n; r++) {
    int c1 = 0, c2 = 0;
    if (r >= opt.first_row && eligible(r) && (opt.max_tries == 0 || (int)slot.size() < opt.max_tries)) {
      const int c = L->corr_off[r + 1] - L->corr_off[r];
      const int arm = row_f[r] != 0.0 ? 1 : 2;   // :644
      if (arm == 2) {
        if (!row_f_init) return msfm_set_error(ctx, MSFM_E_INVAL, "%s: row %d has no focal length and row_f_init is null", who, r);
        f_init[r] = row_f_init[r];
      }
      slot.push_back(Slot{r, L->corr_off[r], arm == 1 ? off1[r] : off2[r], c, arm});
      toff.push_back(toff.back() + c);
      (arm == 1 ? c1 : c2) = c;
      R->tried[r] = 1; R->arm[r] = (uint8_t)arm;
      last = r;
    }
    off1[r + 1] = off1[r] + c1; off2[r + 1] = off2[r] + c2;
  }
  const int nt = (int)slot.size(), E = toff.back(), E1 = off1[n], E2 = off2[n];
  R->n_tried = nt;
  for (int r = std::max(last + 1, opt.first_row); r < n && nt; r++)
    if (eligible(r)) { R->next_row = r; break; }
  if (E2 && (long long)n * n_steps > INT_MAX)
    return msfm_set_error(ctx, MSFM_E_INVAL, "%s: rows * sweep steps = %lld does not fit an int", who, (long long)n * n_steps);
  if (nt == 0) { *out = R.release(); return MSFM_OK; }
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  DevBuf<Slot> d_slot;
  DevBuf<int> d_toff, d_off1, d_off2, d_first, d_bstep, d_biter, d_nin, d_nout;
  DevBuf<double> d_rowf, d_finit, d_w1, d_x1, d_w2, d_x2;
  DevBuf<double> d_f, d_R, d_t, d_avg, d_err;
  DevBuf<uint8_t> d_added, d_pass, d_state;
  EpnpResult r1;
  EpnpfResult r2;
  DevScope sc(ctx);
  LP_TRY(sc.up(d_slot, slot)); LP_TRY(sc.up(d_toff, toff)); LP_TRY(sc.up(d_off1, off1)); LP_TRY(sc.up(d_off2, off2));
  LP_TRY(sc.up(d_rowf, row_f, (size_t)n));
  if (!d_added_dev && pt_new_added && n_points) LP_TRY(sc.up(d_added, pt_new_added, (size_t)n_points));
  const uint8_t* added_p = d_added_dev ? d_added_dev : d_added.p;
  LP_TRY(d_w1.alloc(3 * (size_t)std::max(1, E1))); LP_TRY(d_x1.alloc(2 * (size_t)std::max(1, E1)));
  LP_TRY(d_w2.alloc(3 * (size_t)std::max(1, E2))); LP_TRY(d_x2.alloc(2 * (size_t)std::max(1, E2)));
  LP_TRY(d_f.alloc(n)); LP_TRY(d_R.alloc(9 * (size_t)n)); LP_TRY(d_t.alloc(3 * (size_t)n)); LP_TRY(d_avg.alloc(n)); LP_TRY(d_bstep.alloc(n));
  LP_TRY(d_biter.alloc(n)); LP_TRY(d_pass.alloc(n)); LP_TRY(d_nin.alloc(n)); LP_TRY(d_nout.alloc(n));
  LP_TRY(d_err.alloc(T)); LP_TRY(d_state.alloc(T));
  const size_t n_first = (size_t)nt * (size_t)std::max(1, n_points);
  LP_TRY(d_first.alloc(n_first));
  // untried rows return zeros
  LP_TRY(hipMemsetAsync(d_f.p, 0, sizeof(double) * (size_t)n, s)); LP_TRY(hipMemsetAsync(d_R.p, 0, sizeof(double) * 9 * (size_t)n, s));
  LP_TRY(hipMemsetAsync(d_t.p, 0, sizeof(double) * 3 * (size_t)n, s)); LP_TRY(hipMemsetAsync(d_avg.p, 0, sizeof(double) * (size_t)n, s));
  LP_TRY(hipMemsetAsync(d_bstep.p, 0, sizeof(int) * (size_t)n, s)); LP_TRY(hipMemsetAsync(d_biter.p, 0, sizeof(int) * (size_t)n, s));
  LP_TRY(hipMemsetAsync(d_pass.p, 0, (size_t)n, s)); LP_TRY(hipMemsetAsync(d_nin.p, 0, sizeof(int) * (size_t)n, s));
  LP_TRY(hipMemsetAsync(d_nout.p, 0, sizeof(int) * (size_t)n, s));
  LP_TRY(hipMemsetAsync(d_err.p, 0, sizeof(double) * (size_t)T, s)); LP_TRY(hipMemsetAsync(d_state.p, 0, (size_t)T, s));
  LP_TRY(hipMemsetD32Async((hipDeviceptr_t)d_first.p, LP_BIG, n_first, s));
  {
    KTimer tm(ctx, "localizepose_gather");
    hipLaunchKernelGGL(k_gather, dim3(cdiv(E, 256)), dim3(256), 0, s, E, nt, d_toff.p, d_slot.p, L->d_pw.p, L->d_p2.p, d_w1.p, d_x1.p, d_w2.p,
                       d_x2.p);
  }
  LP_TRY(hipGetLastError());
  ArmOut a1{nullptr, nullptr, nullptr, nullptr, nullptr, nullptr}, a2 = a1;
  if (E1) {   // :644-672
    LP_TRY(r1.alloc(n, E1));
    MSFM_TRY(pose_epnp_dev(ctx, PoseView{n, d_off1.p, d_w1.p, d_x1.p, d_rowf.p, nullptr}, opt.max_iter, opt.seed, r1));
    a1 = ArmOut{nullptr, r1.R.p, r1.t.p, r1.avg.p, nullptr, r1.best_iter.p};
  }
  if (E2) {   // :673-704
    LP_TRY(sc.up(d_finit, f_init));
    LP_TRY(r2.alloc(n, E2));
    MSFM_TRY(pose_epnpf_dev(ctx, PoseView{n, d_off2.p, d_w2.p, d_x2.p, d_finit.p, nullptr}, n_steps, &opt.sweep, r2));
    a2 = ArmOut{r2.f.p, r2.R.p, r2.t.p, r2.avg.p, r2.best_step.p, r2.best_iter.p};
  }
  {
    KTimer tm(ctx, "localizepose_state");
    tm.count = 3;
    hipLaunchKernelGGL(k_rows, dim3(cdiv(nt, 64)), dim3(64), 0, s, nt, d_slot.p, a1, a2, d_rowf.p, opt.th_mse_localization, d_f.p, d_R.p, d_t.p,
                       d_avg.p, d_bstep.p, d_biter.p, d_pass.p);
    hipLaunchKernelGGL(k_first, dim3(cdiv(E, 256)), dim3(256), 0, s, E, nt, d_toff.p, d_slot.p, r1.err.p, r2.err.p, d_avg.p, d_pass.p, L->d_cp.p,
                       n_points, added_p, d_first.p);
    hipLaunchKernelGGL(k_state, dim3(cdiv(E, 256)), dim3(256), 0, s, E, nt, d_toff.p, d_slot.p, r1.err.p, r2.err.p, d_avg.p, d_pass.p, L->d_cp.p,
                       n_points, added_p, d_first.p, d_err.p, d_state.p, d_nin.p, d_nout.p);
  }
  LP_TRY(hipGetLastError());
  // ---- one read-back, one wait ----
  LP_TRY(sc.down(R->pass.data(), d_pass.p, (size_t)n)); LP_TRY(sc.down(R->f.data(), d_f.p, (size_t)n)); LP_TRY(sc.down(R->R.data(), d_R.p, 9 * (size_t)n));
  LP_TRY(sc.down(R->t.data(), d_t.p, 3 * (size_t)n)); LP_TRY(sc.down(R->avg.data(), d_avg.p, (size_t)n));
  LP_TRY(sc.down(R->best_step.data(), d_bstep.p, (size_t)n)); LP_TRY(sc.down(R->best_iter.data(), d_biter.p, (size_t)n));
  LP_TRY(sc.down(R->n_in.data(), d_nin.p, (size_t)n)); LP_TRY(sc.down(R->n_out.data(), d_nout.p, (size_t)n));
  LP_TRY(sc.down(R->errors.data(), d_err.p, (size_t)T)); LP_TRY(sc.down(R->state.data(), d_state.p, (size_t)T));
  LP_TRY(sc.finish());   // the scratch above is released on return
  for (int r = 0; r < n; r++)
    if (R->tried[r] && R->pass[r]) { R->winner = r; break; }
  if (keep_state) keep_state->swap(d_state);
  if (h2d_bytes) *h2d_bytes += sc.h2d;
  *out = R.release();
  return MSFM_OK;
}

MSFM_API int msfm_localize_poses(msfm_ctx* ctx, const msfm_localize_set* L, const double* row_f, const double* row_f_init, int n_points,
                                 const uint8_t* pt_new_added, const msfm_localize_pose_options* opt_in, msfm_localize_pose_set** out) {
  return localize_poses_dev(ctx, "msfm_localize_poses", L, row_f, row_f_init, n_points, pt_new_added, nullptr, opt_in, out, nullptr, nullptr);
}

MSFM_API int msfm_localize_pose_set_size(const msfm_localize_pose_set* R, int* n_rows, int* n_corr, int* n_tried, int* winner, int* next_row) {
  if (!R) return MSFM_E_INVAL;
  if (n_rows) *n_rows = R->n;
  if (n_corr) *n_corr = R->n_corr;
  if (n_tried) *n_tried = R->n_tried;
  if (winner) *winner = R->winner;
  if (next_row) *next_row = R->next_row;
  return MSFM_OK;
}

MSFM_API int msfm_localize_pose_set_fetch(const msfm_localize_pose_set* R, uint8_t* tried, uint8_t* arm, uint8_t* pass, double* f, double* Rm,
                                          double* t, double* avg_error, int* best_step, int* best_iter, int* n_inliers, int* n_outliers,
                                          double* errors, uint8_t* corr_state) {
  if (!R) return MSFM_E_INVAL;
  if (tried) std::copy(R->tried.begin(), R->tried.end(), tried);
  if (arm) std::copy(R->arm.begin(), R->arm.end(), arm);
  if (pass) std::copy(R->pass.begin(), R->pass.end(), pass);
  if (f) std::copy(R->f.begin(), R->f.end(), f);
  if (Rm) std::copy(R->R.begin(), R->R.end(), Rm);
  if (t) std::copy(R->t.begin(), R->t.end(), t);
  if (avg_error) std::copy(R->avg.begin(), R->avg.end(), avg_error);
  if (best_step) std::copy(R->best_step.begin(), R->best_step.end(), best_step);
  if (best_iter) std::copy(R->best_iter.begin(), R->best_iter.end(), best_iter);
  if (n_inliers) std::copy(R->n_in.begin(), R->n_in.end(), n_inliers);
  if (n_outliers) std::copy(R->n_out.begin(), R->n_out.end(), n_outliers);
  if (errors) std::copy(R->errors.begin(), R->errors.end(), errors);
  if (corr_state) std::copy(R->state.begin(), R->state.end(), corr_state);
  return MSFM_OK;
}

MSFM_API void msfm_localize_pose_set_destroy(msfm_localize_pose_set* R) { delete R; }
