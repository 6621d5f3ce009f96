// Two small pieces of the bundle adjustment's LM step that ride along with launches of the factorisation (chol.hip) instead of
// being launches of their own on the dependent chain.  Both are plain data for the factorisation: it runs them, it does not
// know what they mean.
//   ModelSumArgs   the per-intrinsics sums and the intrinsics block of the reduced system (the body of k_modelsum, ba.hip):
//                  extra workgroups behind the level-0 k_corner_syrk launch - nothing before that level's k_merge_corners
//                  touches the entries it stores.
//   SolveEpilogue  the camera / intrinsics part of the step (the arithmetic of k_update_params, ba.hip), done by the workgroup
//                  of k_backsolve_chain that owns the columns, behind the publication of its block.
#pragma once
#include "ba_device.h"

constexpr int MODELSUM_PSTRIDE = 80, MODELSUM_JMJM = 54, MODELSUM_JMR = 69;   // PSTRIDE, F_JMJM, F_JMR of ba.hip (asserted there)

// Per intrinsics block: sum camftf(Jm^T Jm | Jm^T r) over its cameras (one wave, lanes strided,
// fixed butterfly) -> modelsum[mb][12]; LM diagonal / raw norms; gradient.
// fin.M set (see CamFinish; one intrinsics block at most, so its diagonal block is the only intrinsics x intrinsics block): the
// workgroup has a second wave, which sums the block's chunk partials (written by the launch before) beside the model sum; the
// first wave then assembles the block and its rhs entries from both, as asm_mm does.
struct ModelFinish {
  double* M; int ld, n, mo, n_mm;
  const int *mm_row, *mm_col, *mm_first; const double* mm_partial;
  double radius;
};
struct ModelSumArgs {
  int nmb;   // intrinsics blocks = workgroups
  const int *mcam_first, *mcam;
  const double* camftf;
  double *modelsum, *diag_m;
  const double* scale_m;
  int reuse_diag, mode;
  double dmin, dmax;
  double* gmax_m;
  ModelFinish fin;
};

// intrinsics-intrinsics blocks: one wave per block, lanes strided over chunks.
// partial layout per chunk: 9 (Tm Tm'^T) + 3 (sum Tm.u, self pairs only).
__device__ __forceinline__ void mm_chunk_sums(int b, const int* __restrict__ blk_chunk_first, const double* __restrict__ partial, int lane, double (&acc)[12]) {
#pragma unroll
  for (int k = 0; k < 12; k++) acc[k] = 0.0;
  int ch = blk_chunk_first[b] + lane;
  const int ch1 = blk_chunk_first[b + 1];
  for (; ch + 192 < ch1; ch += 256) {   // the records of four of a lane's chunks asked for at once, added in chunk order as below
    double v[4][12];
#pragma unroll
    for (int j = 0; j < 4; j++)
#pragma unroll
      for (int k = 0; k < 12; k++) v[j][k] = partial[(size_t)(ch + 64 * j) * 12 + k];
#pragma unroll
    for (int j = 0; j < 4; j++)
#pragma unroll
      for (int k = 0; k < 12; k++) acc[k] += v[j][k];
  }
  for (; ch < ch1; ch += 64)
#pragma unroll
    for (int k = 0; k < 12; k++) acc[k] += partial[(size_t)ch * 12 + k];
#pragma unroll
  for (int k = 0; k < 12; k++) acc[k] = wave_sum(acc[k]);
}
__device__ __forceinline__ void mm_finish(int mb, int lane, const ModelFinish& f, const double* mmacc, const double* __restrict__ modelsum, const double* __restrict__ diag_m) {
  if (lane < 9) {
    const int a = lane / 3, c = lane % 3;
    double v = -mmacc[lane];
    v += modelsum[12 * (size_t)mb + lane];
    if (a == c) { const double q = sqrt(diag_m[3 * mb + a] / f.radius); v += q * q; }
    f.M[(size_t)(f.mo + 3 * mb + a) * f.ld + f.mo + 3 * mb + c] = v;
  } else if (lane < 12) {
    f.M[(size_t)f.n * f.ld + f.mo + 3 * mb + lane - 9] = modelsum[12 * (size_t)mb + lane] - mmacc[lane];
  }
}
// The workgroup of intrinsics block mb: thread `tid` of its first wave (and of its second, with fin.M); mmacc: 13 doubles of LDS.
// Every thread that comes in reaches the barrier (without fin.M there is none and only one wave); other waves of the
// workgroup must have left before.
__device__ __forceinline__ void modelsum_body(const ModelSumArgs& A, int mb, int tid, double* mmacc /*[13]: the second wave's sums; [12]: the block is in the list*/) {
  const ModelFinish& fin = A.fin;
  const int lane = tid & 63;
  if (tid >= 64) {   // (only with fin.M)
    int blk = -1;
    for (int b = 0; b < fin.n_mm; b++) if (fin.mm_row[b] == mb && fin.mm_col[b] == mb) blk = b;
    if (blk >= 0) {
      double a12[12];
      mm_chunk_sums(blk, fin.mm_first, fin.mm_partial, lane, a12);
#pragma unroll
      for (int k = 0; k < 12; k++) if (k == lane) mmacc[k] = a12[k];
    }
    if (lane == 0) mmacc[12] = blk >= 0 ? 1.0 : 0.0;
    __syncthreads();
    return;
  }
  const int* __restrict__ mcam_first = A.mcam_first;
  const int* __restrict__ mcam = A.mcam;
  const double* __restrict__ camftf = A.camftf;
  double* __restrict__ modelsum = A.modelsum;
  double* __restrict__ diag_m = A.diag_m;
  double acc[12];
#pragma unroll
  for (int k = 0; k < 12; k++) acc[k] = 0.0;
  // (a lane's cameras q, q + 64, ... in that order; the records of FOUR of them are asked for before the first is added - the
  //  work is one wave whose time is its dependent load rounds: 8 rounds of 12 loads at config 3, 12.7 us, before)
  const int q1 = mcam_first[mb + 1];
  for (int q = mcam_first[mb] + lane; q < q1; q += 256) {
    double v[4][12];
#pragma unroll
    for (int j = 0; j < 4; j++) {
      const int qq = q + 64 * j;
      const double* f = camftf + (size_t)mcam[min(qq, q1 - 1)] * MODELSUM_PSTRIDE;
#pragma unroll
      for (int k = 0; k < 9; k++) v[j][k] = f[MODELSUM_JMJM + k];
#pragma unroll
      for (int k = 0; k < 3; k++) v[j][9 + k] = f[MODELSUM_JMR + k];
    }
#pragma unroll
    for (int j = 0; j < 4; j++)
      if (q + 64 * j < q1) {
#pragma unroll
        for (int k = 0; k < 12; k++) acc[k] += v[j][k];
      }
  }
#pragma unroll
  for (int k = 0; k < 12; k++) acc[k] = wave_sum(acc[k]);
  if (lane == 0) {
    for (int k = 0; k < 12; k++) modelsum[12 * (size_t)mb + k] = acc[k];
    for (int a = 0; a < 3; a++) {
      const double s = acc[a * 3 + a];
      if (A.mode == 1) diag_m[3 * mb + a] = s;
      else if (!A.reuse_diag) diag_m[3 * mb + a] = fmin(fmax(s, A.dmin), A.dmax);
      A.gmax_m[3 * mb + a] = fabs(acc[9 + a] / A.scale_m[3 * mb + a]);
    }
  }
  if (!fin.M) return;
  __syncthreads();   // (the second wave's sums; modelsum and diag_m of this block, written by lane 0 above, are read back by the other lanes)
  if (mmacc[12] != 0.0) mm_finish(mb, lane, fin, mmacc, modelsum, diag_m);
}

// The step's reduced part from the solution of the reduced system, per column of the system: the solution leaves the solver's
// elimination order for the caller's parameter order (z_out), with the finiteness check on the way, and the candidates
// x - z * scale go to the candidate buffers; the squares |dx|^2 and |x|^2 go out per scalar (the caller sums them in blocks
// of 256).  Parameters [0, n0) live in the arrays with index 0, the others in those with index 1.
struct SolveEpilogue {
  const int* col_param;    // [columns of the system]: parameter index i, -1 for padding and the rhs column
  const int* col_slot;     // [columns]: where the parameter sits in cur / dst of its array pair
  int n0;
  const double *scale0, *scale1;   // [i], [i - n0]
  const double *cur0, *cur1;
  double *dst0, *dst1;
  double* z_out;           // [i]
  double *dx2, *x2;        // [i]
  int* fail;               // or-ed with 4 for a solution value that is not finite
  double count_weight;
};
// In two halves: what does not depend on the solution (two dependent rounds of loads) is fetched while the workgroup still
// waits for the blocks behind its own; behind the publication only the arithmetic and the stores are left - for the last
// block to be solved they are the tail of the launch (k_backsolve_chain at config 3: 41.6 -> 43.6 us with everything behind
// the publication, 41.4 -> 41.9 us so).
struct EpilogueColumn { int i, k; double sc, xv; };
__device__ __forceinline__ EpilogueColumn solve_epilogue_fetch(const SolveEpilogue& E, int col) {
  EpilogueColumn c;
  c.i = E.col_param[col]; c.k = 0; c.sc = 0.0; c.xv = 0.0;
  if (c.i < 0) return c;
  c.k = E.col_slot[col];
  const bool first = c.i < E.n0;
  c.sc = first ? E.scale0[c.i] : E.scale1[c.i - E.n0];
  c.xv = first ? E.cur0[c.k] : E.cur1[c.k];
  return c;
}
__device__ __forceinline__ void solve_epilogue_finish(const SolveEpilogue& E, const EpilogueColumn& c, double zv) {
  if (c.i < 0) return;
  const double xv = c.xv;
  E.z_out[c.i] = zv;
  if (!isfinite(zv)) atomicOr(E.fail, 4);
  const double cand = fma(-zv, c.sc, xv);   // (k_update_params' xv + (-zv) * sc, which the compiler contracts to this)
  (c.i < E.n0 ? E.dst0 : E.dst1)[c.k] = cand;
  const double d = cand - xv;
  E.dx2[c.i] = d * d * E.count_weight;  // replicated blocks are counted by the lead rank only
  E.x2[c.i] = xv * xv * E.count_weight;
}
