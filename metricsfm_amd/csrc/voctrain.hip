// Building the vocabulary tree (Database::BuildVocabularyTree, SfM/src/database.cc:655-677): hierarchical k-means over the
// float32 rows a descriptor set holds, one tree level at a time and every open node of a level in the same launches.
// include/msfm.h states the definitions; every quantity summed across features is a 64-bit integer, so no result depends on the
// order in which the device adds.
//
// The active features of a level lie in `perm`, the members of a node contiguous and in ascending feature number (one stable
// rocPRIM sort by child node at the end of a level), `node_of` beside them.  A node owns min(m, k) rows of `cent`, the
// centres in the descent's relayed layout [row][8][16].
//   k_init        the row pointer of every sampled feature and the integer maximum of the |value| bit patterns
//   k_prep_sizes  per node: rows, accumulation chunks (VT_CH members each), global accumulator rows (nodes of several chunks);
//                 four exclusive scans turn them and the member counts into offsets
//   k_node_init   small nodes (m <= k) take their members as rows; larger ones draw centre 0
//   k_seed_dist   eight lanes per member: distance to the newest centre, running minimum, integer weight; one inclusive u64 scan
//   k_seed_pick   one lane per node: W from the scan, the draw, a binary search for the first prefix above it
//   k_gather      copies the descriptor a row names into cent (relayed)
//   k_assign      the descent's inner loop against the centres of the member's own node; a changed assignment flags the node
//   k_accum       one workgroup per chunk, lane d owns element d: per-cluster int64 sums in LDS; a node of one chunk writes its
//                 centres at once, a node of several adds into its global rows with 64-bit integer atomics (k_finish divides)
//   k_mark        per node: iteration count, converged / capped, the count of nodes still open (the host's one wait per iteration)
//   k_rows        per row: leaf / open child; two exclusive scans number the level's leaves and the next level's nodes
//   k_emit        the level's blocks: compacted rows, links, weights, the child nodes' member counts
//   k_next_key    per member: its child's ordinal, or the sentinel that sorts a finished feature behind the active ones
#include <cmath>
#include <memory>

#define VOCTRAIN_HD __host__ __device__
#include "common.h"
#include "runs_device.h"
#include "voctrain_args.h"
#include "words_dist.h"

namespace voctrain {

typedef unsigned long long u64;
#define VT_CH 1024      // members per accumulation workgroup
#define VT_SMALL 0      // m <= k: a block of m leaves
#define VT_SINGLE 1     // the seeding ended with one centre: a block of one leaf
#define VT_SPLIT 2

struct NodeArrays {     // per node of the current level, device pointers
  int *nm, *nstart, *coff, *choff, *moff, *nc, *kind, *done, *iters, *changed, *capped;
};

__global__ __launch_bounds__(256) void k_init(int M, int ns, const int* __restrict__ samp_off, const float* const* __restrict__ samp_rows,
                                               const float** __restrict__ rowptr, int* __restrict__ perm, int* __restrict__ node_of,
                                               unsigned* __restrict__ maxbits) {
  const long e_l = (long)blockIdx.x * 8 + (threadIdx.x >> 5);
  const int l = threadIdx.x & 31;
  unsigned mb = 0;
  if (e_l < M) {
    const int e = (int)e_l;
    const int img = csr_segment_of(samp_off, ns, e);
    const float* row = samp_rows[img] + (size_t)(e - samp_off[img]) * WORDS_DIM;
    const float4 v = reinterpret_cast<const float4*>(row)[l];
    mb = max(max(__float_as_uint(v.x) & 0x7fffffffu, __float_as_uint(v.y) & 0x7fffffffu),
             max(__float_as_uint(v.z) & 0x7fffffffu, __float_as_uint(v.w) & 0x7fffffffu));
    if (l == 0) { rowptr[e] = row; perm[e] = e; node_of[e] = 0; }
  }
  for (int d = 32; d > 0; d >>= 1) mb = max(mb, (unsigned)__shfl_xor((int)mb, d));
  // a wave whose maximum the word already holds has nothing to add: one atomic per wave on one address took 11.6 of the call's
  // 80 ms at 2 048 000 features (the word only grows, so a stale read can only cause an atomic too many)
  if ((threadIdx.x & 63) == 0 && mb > *(volatile unsigned*)maxbits) atomicMax(maxbits, mb);
}

__global__ __launch_bounds__(256) void k_prep_sizes(int nn, int k, const int* __restrict__ nm, int* __restrict__ rows, int* __restrict__ chunks,
                                                     int* __restrict__ mrows) {
  const int o = blockIdx.x * 256 + threadIdx.x;
  if (o > nn) return;
  const int m = o < nn ? nm[o] : 0;   // entry nn closes the scans
  rows[o] = min(m, k);
  chunks[o] = m > k ? (m + VT_CH - 1) / VT_CH : 0;
  mrows[o] = m > VT_CH ? k : 0;
}

__global__ void k_totals(int nn, const int* __restrict__ nstart, const int* __restrict__ coff, const int* __restrict__ choff,
                         const int* __restrict__ moff, int* __restrict__ tot) {
  tot[0] = nstart[nn]; tot[1] = coff[nn]; tot[2] = choff[nn]; tot[3] = moff[nn];
}

__global__ __launch_bounds__(256) void k_node_init(int nn, int k, int level, uint64_t seed, NodeArrays A, const int* __restrict__ perm,
                                                    int* __restrict__ csrc) {
  const int o = blockIdx.x * 256 + threadIdx.x;
  if (o >= nn) return;
  const int b = A.nstart[o], m = A.nm[o], base = A.coff[o];
  A.iters[o] = 0; A.changed[o] = 0; A.capped[o] = 0;
  if (m <= k) {
    A.kind[o] = VT_SMALL; A.nc[o] = m; A.done[o] = 1;
    for (int i = 0; i < m; i++) csrc[base + i] = perm[b + i];
  } else {
    A.kind[o] = VT_SPLIT; A.nc[o] = 1; A.done[o] = 0;
    csrc[base] = perm[b + (int)(voctrain_draw(seed, level, o, 0) % (uint64_t)m)];
    for (int i = 1; i < k; i++) csrc[base + i] = -1;
  }
}

// row j of every node that has just been given one (j = 0: also all rows of the small nodes)
__global__ __launch_bounds__(128) void k_gather(int j, NodeArrays A, const int* __restrict__ csrc, const float* const* __restrict__ rowptr,
                                                 float* __restrict__ cent) {
  const int o = blockIdx.x, d = threadIdx.x;
  const int base = A.coff[o];
  if (A.kind[o] == VT_SMALL) {
    if (j != 0) return;
    for (int i = 0; i < A.nc[o]; i++) cent[(size_t)(base + i) * WORDS_DIM + relay_pos(d)] = rowptr[csrc[base + i]][d];
  } else if (A.nc[o] == j + 1) {
    cent[(size_t)(base + j) * WORDS_DIM + relay_pos(d)] = rowptr[csrc[base + j]][d];
  }
}

// lane j's sixteen elements of a feature's row
__device__ static inline void load_lane(float* f, const float* row, int j) {
#pragma unroll
  for (int t = 0; t < 16; t++) f[t] = row[j + 8 * t];
}

// Round j >= 1 of the seeding, for the nodes that still hold exactly j centres: eight lanes per member, as in k_assign.
__global__ __launch_bounds__(256) void k_seed_dist(int M, int j, double scale, NodeArrays A, const int* __restrict__ perm,
                                                    const int* __restrict__ node_of, const float* const* __restrict__ rowptr,
                                                    const float* __restrict__ cent, float* __restrict__ mind, u64* __restrict__ w) {
  const long p_l = (long)blockIdx.x * 32 + (threadIdx.x >> 3);
  const int lane = threadIdx.x & 7;
  const bool inside = p_l < M;
  const int p = inside ? (int)p_l : 0;
  const int o = node_of[p];
  const bool act = inside && A.kind[o] == VT_SPLIT && A.nc[o] == j;
  float f[16];
#pragma unroll
  for (int t = 0; t < 16; t++) f[t] = 0.f;
  float s = 0.f;
  if (__any(act)) {
    if (act) {
      load_lane(f, rowptr[perm[p]], lane);
      s = part16(f, cent + (size_t)(A.coff[o] + j - 1) * WORDS_DIM + lane * 16);
    }
    s = add8(s);
  }
  if (!inside || lane != 0) return;
  if (!act) { w[p] = 0; return; }
  const float d = j == 1 ? s : fminf(mind[p], s);
  mind[p] = d;
  w[p] = (u64)((double)d * scale);   // exact: a power of two, then truncation
}

__global__ __launch_bounds__(256) void k_seed_pick(int nn, int j, int level, uint64_t seed, NodeArrays A, const int* __restrict__ perm,
                                                    const u64* __restrict__ P, int* __restrict__ csrc) {
  const int o = blockIdx.x * 256 + threadIdx.x;
  if (o >= nn || A.kind[o] != VT_SPLIT || A.nc[o] != j) return;
  const int b = A.nstart[o], e = b + A.nm[o];
  const u64 below = b ? P[b - 1] : 0;
  const u64 W = P[e - 1] - below;
  if (W == 0) {                       // every member sits on a centre: the seeding ends with j centres
    if (j == 1) { A.kind[o] = VT_SINGLE; A.done[o] = 1; }
    return;
  }
  const u64 r = voctrain_draw(seed, level, o, j) % W;
  int lo = b, hi = e - 1;             // the first member whose inclusive prefix exceeds r (the last one's is W > r)
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (P[mid] - below > r) hi = mid; else lo = mid + 1;
  }
  csrc[A.coff[o] + j] = perm[lo];
  A.nc[o] = j + 1;
}

// Eight lanes per member, 32 members per workgroup: the loop of k_descend against the centres of the member's node.  Members of
// finished nodes idle; the loops run while any lane of the wave needs them, so whole waves reach the shuffles.
__global__ __launch_bounds__(256) void k_assign(int M, int k, NodeArrays A, const int* __restrict__ perm, const int* __restrict__ node_of,
                                                 const float* const* __restrict__ rowptr, const float* __restrict__ cent,
                                                 uint8_t* __restrict__ asg) {
  const long p_l = (long)blockIdx.x * 32 + (threadIdx.x >> 3);
  const int lane = threadIdx.x & 7;
  const bool inside = p_l < M;
  const int p = inside ? (int)p_l : 0;
  const int o = node_of[p];
  const bool act = inside && A.kind[o] == VT_SPLIT && !A.done[o];
  if (!__any(act)) return;
  float f[16];
#pragma unroll
  for (int t = 0; t < 16; t++) f[t] = 0.f;
  if (act) load_lane(f, rowptr[perm[p]], lane);
  const int N = act ? A.nc[o] : 0;
  const float* nb = cent + (size_t)A.coff[o] * WORDS_DIM + lane * 16;
  float best = 4294967296.0f;
  int best_i = -1;
  for (int i = 0; i < k; i++) {
    if (!__any(i < N)) break;
    float s = 0.f;
    if (i < N) s = part16(f, nb + (size_t)i * WORDS_DIM);
    s = add8(s);
    if (i < N && s < best) { best = s; best_i = i; }   // strict: a tie stays with the lower cluster
  }
  if (!act || lane != 0) return;
  if (asg[p] != (uint8_t)best_i) { asg[p] = (uint8_t)best_i; A.changed[o] = 1; }   // (every writer stores the same 1)
}

__device__ static inline float centre_value(long long sum, int count, double inv) {
  return (float)(((double)sum / (double)count) * inv);
}

// One workgroup per chunk of a node whose assignment changed; lane d owns element d of every cluster's sum, so the LDS needs no
// synchronisation.  Lane c of each wave counts cluster c.
__global__ __launch_bounds__(128) void k_accum(int nn, double sscale, double inv, NodeArrays A, const int* __restrict__ perm,
                                                const float* const* __restrict__ rowptr, const uint8_t* __restrict__ asg,
                                                float* __restrict__ cent, int* __restrict__ ccount, u64* __restrict__ gacc, int* __restrict__ gcnt) {
  extern __shared__ long long acc[];   // [nc][128]
  const int c = blockIdx.x, d = threadIdx.x;
  const int o = csr_segment_of(A.choff, nn, c);
  if (A.done[o] || !A.changed[o]) return;
  const int m = A.nm[o], N = A.nc[o];
  const int b = A.nstart[o] + (c - A.choff[o]) * VT_CH, e = min(b + VT_CH, A.nstart[o] + m);
  for (int i = 0; i < N; i++) acc[i * WORDS_DIM + d] = 0;
  const int cl = d & 63;
  int cnt = 0;
  if (cl < N)
    for (int p = b; p < e; p++) cnt += asg[p] == cl;
  int p = b;
  for (; p + 4 <= e; p += 4) {
    const int a0 = asg[p], a1 = asg[p + 1], a2 = asg[p + 2], a3 = asg[p + 3];
    const float x0 = rowptr[perm[p]][d], x1 = rowptr[perm[p + 1]][d], x2 = rowptr[perm[p + 2]][d], x3 = rowptr[perm[p + 3]][d];
    acc[a0 * WORDS_DIM + d] += (long long)((double)x0 * sscale);
    acc[a1 * WORDS_DIM + d] += (long long)((double)x1 * sscale);
    acc[a2 * WORDS_DIM + d] += (long long)((double)x2 * sscale);
    acc[a3 * WORDS_DIM + d] += (long long)((double)x3 * sscale);
  }
  for (; p < e; p++) acc[asg[p] * WORDS_DIM + d] += (long long)((double)rowptr[perm[p]][d] * sscale);
  const int base = A.coff[o];
  const bool multi = m > VT_CH;
  for (int i = 0; i < N; i++) {
    const int ci = __shfl(cnt, i);
    if (!multi) {
      if (ci > 0) cent[(size_t)(base + i) * WORDS_DIM + relay_pos(d)] = centre_value(acc[i * WORDS_DIM + d], ci, inv);   // an emptied cluster keeps its centre
      if (d == 0) ccount[base + i] = ci;
    } else if (ci > 0) {
      atomicAdd(&gacc[(size_t)(A.moff[o] + i) * WORDS_DIM + d], (u64)acc[i * WORDS_DIM + d]);   // two's complement: the sum is the signed sum
      if (d == 0) atomicAdd(&gcnt[A.moff[o] + i], ci);
    }
  }
}

__global__ __launch_bounds__(128) void k_finish(double inv, NodeArrays A, const u64* __restrict__ gacc, const int* __restrict__ gcnt,
                                                 float* __restrict__ cent, int* __restrict__ ccount) {
  const int o = blockIdx.x, d = threadIdx.x;
  if (A.nm[o] <= VT_CH || A.done[o] || !A.changed[o]) return;
  const int base = A.coff[o], mb = A.moff[o];
  for (int i = 0; i < A.nc[o]; i++) {
    const int ci = gcnt[mb + i];
    if (ci > 0) cent[(size_t)(base + i) * WORDS_DIM + relay_pos(d)] = centre_value((long long)gacc[(size_t)(mb + i) * WORDS_DIM + d], ci, inv);
    if (d == 0) ccount[base + i] = ci;
  }
}

__global__ __launch_bounds__(256) void k_mark(int nn, int max_iters, NodeArrays A, int* __restrict__ n_open) {
  const int o = blockIdx.x * 256 + threadIdx.x;
  if (o >= nn || A.kind[o] != VT_SPLIT || A.done[o]) return;
  const int it = ++A.iters[o];
  if (!A.changed[o]) A.done[o] = 1;                                   // the assignment of the iteration before: its centres stand
  else if (it == max_iters) { A.done[o] = 1; A.capped[o] = 1; }
  else atomicAdd(n_open, 1);
  A.changed[o] = 0;
}

// st: nodes iterated, largest iteration count, nodes stopped at max_iters
__global__ __launch_bounds__(256) void k_rows(int nn, int k, int R, int last, NodeArrays A, const int* __restrict__ ccount, int* __restrict__ fleaf,
                                               int* __restrict__ fopen, int* __restrict__ st) {
  const int o = blockIdx.x * 256 + threadIdx.x;
  if (o >= nn) return;
  if (o == 0) { fleaf[R] = 0; fopen[R] = 0; }
  const int base = A.coff[o], rows = min(A.nm[o], k), kind = A.kind[o];
  for (int i = 0; i < rows; i++) {
    int leaf, open = 0;
    if (kind == VT_SMALL) leaf = 1;
    else if (kind == VT_SINGLE) leaf = i == 0;
    else {
      const int cnt = i < A.nc[o] ? ccount[base + i] : 0;
      leaf = cnt > 0 && (last || cnt == 1);
      open = cnt > 0 && !leaf;
    }
    fleaf[base + i] = leaf; fopen[base + i] = open;
  }
  if (kind == VT_SPLIT) {
    atomicAdd(&st[0], 1);
    atomicMax(&st[1], A.iters[o]);
    if (A.capped[o]) atomicAdd(&st[2], 1);
  }
}

__global__ __launch_bounds__(128) void k_emit(int k, int word_base, int next_base, NodeArrays A, const float* __restrict__ cent,
                                               const int* __restrict__ ccount, const int* __restrict__ fleaf, const int* __restrict__ fopen,
                                               const int* __restrict__ leafidx, const int* __restrict__ openidx, uint16_t* __restrict__ out_n,
                                               float* __restrict__ out_desc, uint32_t* __restrict__ out_link, float* __restrict__ out_weight,
                                               int* __restrict__ nm_next) {
  const int o = blockIdx.x, d = threadIdx.x;
  const int base = A.coff[o], rows = min(A.nm[o], k);
  int n_out = 0;
  for (int i = 0; i < rows; i++) {
    const int leaf = fleaf[base + i], open = fopen[base + i];
    if (!leaf && !open) continue;
    const size_t dst = (size_t)o * k + n_out;
    out_desc[dst * WORDS_DIM + d] = cent[(size_t)(base + i) * WORDS_DIM + d];
    if (d == 0) {
      out_link[dst] = leaf ? (WORDS_LEAF | (uint32_t)(word_base + leafidx[base + i])) : (uint32_t)(next_base + openidx[base + i]);
      out_weight[dst] = leaf ? 1.0f : 0.0f;
      if (open) nm_next[openidx[base + i]] = ccount[base + i];
    }
    n_out++;
  }
  for (int i = n_out; i < k; i++) {
    const size_t dst = (size_t)o * k + i;
    out_desc[dst * WORDS_DIM + d] = 0.f;
    if (d == 0) { out_link[dst] = 0; out_weight[dst] = 0.f; }
  }
  if (d == 0) out_n[o] = (uint16_t)n_out;
}

__global__ __launch_bounds__(256) void k_next_key(int M, unsigned sentinel, NodeArrays A, const int* __restrict__ perm, const int* __restrict__ node_of,
                                                   const uint8_t* __restrict__ asg, const int* __restrict__ fopen, const int* __restrict__ openidx,
                                                   unsigned* __restrict__ key, int* __restrict__ val) {
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= M) return;
  const int o = node_of[p];
  unsigned kk = sentinel;
  if (A.kind[o] == VT_SPLIT) {
    const int row = A.coff[o] + asg[p];
    if (fopen[row]) kk = (unsigned)openidx[row];
  }
  key[p] = kk;
  val[p] = perm[p];
}

struct LevelOut {
  int nn = 0;
  DevBuf<uint16_t> n;
  DevBuf<float> desc, weight;
  DevBuf<uint32_t> link;
};

}  // namespace voctrain

#define VT_TRY(e) HIP_TRY(ctx, (e))

MSFM_API int msfm_descset_voctree_train(msfm_descset* set, int k_in, int n_levels, int max_iters, int image_step, uint64_t seed, msfm_voctree** out) {
  using namespace voctrain;
  const char* who = "msfm_descset_voctree_train";
  if (!set) return MSFM_E_INVAL;
  DescView V;
  descset_view(set, &V);
  msfm_ctx* ctx = V.ctx;
  if (!out) return msfm_set_error(ctx, MSFM_E_INVAL, "%s: null argument", who);
  *out = nullptr;
  const voctrain_options options = {k_in, n_levels, max_iters, image_step, seed};
  const voctrain_options* opt = &options;
  std::string bad = voctrain_check_options(opt);
  if (!bad.empty()) return msfm_set_error(ctx, MSFM_E_INVAL, "%s: %s", who, bad.c_str());
  std::vector<int> images, samp_off;
  bad = voctrain_sample(V.n_images, V.count.data(), opt->image_step, &images, &samp_off);
  if (!bad.empty()) return msfm_set_error(ctx, MSFM_E_INVAL, "%s: %s", who, bad.c_str());
  const int ns = (int)images.size(), M0 = samp_off[ns], k = opt->k;
  std::vector<const float*> samp_rows(ns);
  for (int i = 0; i < ns; i++) samp_rows[i] = V.f32[images[i]];   // (null only for an image without features: never dereferenced)
  voctrain_stats S;
  S.n_images = ns; S.n_features = M0;

  HIP_TRY(ctx, hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  // Every scratch array is sized once, from the sample: a level has at most M0 / 2 + 1 nodes (an open node has two members or
  // is the root), at most M0 rows, M0 / VT_CH + nodes chunks and (M0 / VT_CH) k accumulator rows.
  const size_t Mx = (size_t)M0, NN = Mx / 2 + 2, RR = Mx + 1, GR = (Mx / VT_CH + 1) * (size_t)k;
  DevBuf<int> d_samp_off, d_perm, d_perm2, d_node, d_csrc, d_ccount, d_fleaf, d_fopen, d_leafidx, d_openidx, d_small, d_gcnt;
  DevBuf<int> d_nm, d_nm2, d_nstart, d_coff, d_choff, d_moff, d_nc, d_kind, d_done, d_iters, d_changed, d_capped, d_t1, d_t2, d_t3;
  DevBuf<unsigned> d_key, d_key2;
  DevBuf<const float*> d_samp_rows, d_rowptr;
  DevBuf<float> d_cent, d_mind;
  DevBuf<uint8_t> d_asg;
  DevBuf<u64> d_w, d_P, d_gacc;
  PrimTmp tmp;
  std::vector<std::unique_ptr<LevelOut>> levels;
  Child<msfm_voctree> T = child_new<msfm_voctree>(ctx);
  DevScope sc(ctx);
  VT_TRY(sc.up(d_samp_off, samp_off)); VT_TRY(sc.up(d_samp_rows, samp_rows));
  VT_TRY(hip_first_error({d_perm.alloc(Mx), d_perm2.alloc(Mx), d_node.alloc(Mx), d_key.alloc(Mx), d_key2.alloc(Mx), d_rowptr.alloc(Mx),
                          d_mind.alloc(Mx), d_asg.alloc(Mx), d_w.alloc(Mx), d_P.alloc(Mx), d_csrc.alloc(RR), d_ccount.alloc(RR), d_fleaf.alloc(RR),
                          d_fopen.alloc(RR), d_leafidx.alloc(RR), d_openidx.alloc(RR), d_cent.alloc(RR * WORDS_DIM), d_small.alloc(16),
                          d_gacc.alloc(GR * WORDS_DIM), d_gcnt.alloc(GR)}));
  VT_TRY(hip_first_error({d_nm.alloc(NN), d_nm2.alloc(NN), d_nstart.alloc(NN), d_coff.alloc(NN), d_choff.alloc(NN), d_moff.alloc(NN), d_nc.alloc(NN),
                          d_kind.alloc(NN), d_done.alloc(NN), d_iters.alloc(NN), d_changed.alloc(NN), d_capped.alloc(NN), d_t1.alloc(NN),
                          d_t2.alloc(NN), d_t3.alloc(NN)}));
  const unsigned end_bit = (unsigned)bits_for((unsigned)M0);   // child ordinals are below M0 / 2, the sentinel is M0
  int* d_tot = d_small.p;         // [4] member, row, chunk and accumulator-row totals of a level
  int* d_st = d_small.p + 4;      // [3] k_rows' statistics
  int* d_nopen = d_small.p + 8;
  unsigned* d_maxbits = reinterpret_cast<unsigned*>(d_small.p + 9);

  // the values of the sample: their largest magnitude decides the two shifts
  VT_TRY(hipMemsetAsync(d_small.p, 0, sizeof(int) * 16, s));
  {
    KTimer t(ctx, "voctrain_scan");
    hipLaunchKernelGGL(k_init, dim3(cdiv(M0, 8)), dim3(256), 0, s, M0, ns, d_samp_off.p, d_samp_rows.p, d_rowptr.p, d_perm.p, d_node.p, d_maxbits);
  }
  VT_TRY(hipGetLastError());
  unsigned maxbits = 0;
  VT_TRY(sc.down(&maxbits, d_maxbits, 1));
  VT_TRY(hipStreamSynchronize(s));
  S.host_waits++;
  bad = voctrain_shifts(maxbits, &S.weight_shift, &S.sum_shift);
  if (!bad.empty()) return msfm_set_error(ctx, MSFM_E_INVAL, "%s: %s", who, bad.c_str());
  const double wscale = ldexp(1.0, S.weight_shift), sscale = ldexp(1.0, S.sum_shift), inv = ldexp(1.0, -S.sum_shift);

  NodeArrays A = {d_nm.p, d_nstart.p, d_coff.p, d_choff.p, d_moff.p, d_nc.p, d_kind.p, d_done.p, d_iters.p, d_changed.p, d_capped.p};
  int* nm_next = d_nm2.p;
  int nn = 1, M = M0, block_base = 0;
  int64_t word_base = 0;
  VT_TRY(hipMemcpyAsync(d_nm.p, &M0, sizeof(int), hipMemcpyHostToDevice, s));   // the root
  for (int level = 0; level < opt->levels && nn > 0; level++) {
    // offsets of the level's nodes, rows, chunks and accumulator rows
    int tot[4] = {0, 0, 0, 0};
    {
      KTimer t(ctx, "voctrain_level");
      hipLaunchKernelGGL(k_prep_sizes, dim3(cdiv(nn + 1, 256)), dim3(256), 0, s, nn, k, A.nm, d_t1.p, d_t2.p, d_t3.p);
      VT_TRY(hipMemsetAsync(A.nm + nn, 0, sizeof(int), s));   // a zero behind the member counts closes their scan
      VT_TRY(prim_scan_excl(tmp, A.nm, A.nstart, (size_t)nn + 1, s));
      VT_TRY(prim_scan_excl(tmp, d_t1.p, A.coff, (size_t)nn + 1, s));
      VT_TRY(prim_scan_excl(tmp, d_t2.p, A.choff, (size_t)nn + 1, s));
      VT_TRY(prim_scan_excl(tmp, d_t3.p, A.moff, (size_t)nn + 1, s));
      hipLaunchKernelGGL(k_totals, dim3(1), dim3(1), 0, s, nn, A.nstart, A.coff, A.choff, A.moff, d_tot);
    }
    VT_TRY(hipGetLastError());
    VT_TRY(sc.down(tot, d_tot, 4));
    VT_TRY(hipStreamSynchronize(s));
    S.host_waits++;
    M = tot[0];
    const int R = tot[1], n_chunks = tot[2], n_mrows = tot[3];
    if (M < 1 || M > M0 || R < 1 || R > M || (size_t)nn + 1 > NN || (size_t)n_mrows > GR)
      return msfm_set_error(ctx, MSFM_E_DEVICE, "%s: level %d has inconsistent sizes (%d members, %d rows, %d nodes)", who, level, M, R, nn);
    const int gM8 = cdiv(M, 32), gN = cdiv(nn, 256);
    {
      KTimer t(ctx, "voctrain_seed");
      hipLaunchKernelGGL(k_node_init, dim3(gN), dim3(256), 0, s, nn, k, level, opt->seed, A, d_perm.p, d_csrc.p);
      hipLaunchKernelGGL(k_gather, dim3(nn), dim3(128), 0, s, 0, A, d_csrc.p, d_rowptr.p, d_cent.p);
      for (int j = 1; j < k && n_chunks > 0; j++) {
        hipLaunchKernelGGL(k_seed_dist, dim3(gM8), dim3(256), 0, s, M, j, wscale, A, d_perm.p, d_node.p, d_rowptr.p, d_cent.p, d_mind.p, d_w.p);
        VT_TRY(prim_scan_incl(tmp, d_w.p, d_P.p, (size_t)M, s));
        hipLaunchKernelGGL(k_seed_pick, dim3(gN), dim3(256), 0, s, nn, j, level, opt->seed, A, d_perm.p, d_P.p, d_csrc.p);
        hipLaunchKernelGGL(k_gather, dim3(nn), dim3(128), 0, s, j, A, d_csrc.p, d_rowptr.p, d_cent.p);
      }
    }
    VT_TRY(hipGetLastError());
    if (n_chunks > 0) {
      VT_TRY(hipMemsetAsync(d_asg.p, 0xff, (size_t)M, s));   // no cluster: the first assignment differs everywhere
      for (int it = 0; it < opt->max_iters; it++) {
        {
          KTimer t(ctx, "voctrain_assign");
          hipLaunchKernelGGL(k_assign, dim3(gM8), dim3(256), 0, s, M, k, A, d_perm.p, d_node.p, d_rowptr.p, d_cent.p, d_asg.p);
        }
        {
          KTimer t(ctx, "voctrain_update");
          if (n_mrows > 0) {
            VT_TRY(hipMemsetAsync(d_gacc.p, 0, sizeof(u64) * (size_t)n_mrows * WORDS_DIM, s));
            VT_TRY(hipMemsetAsync(d_gcnt.p, 0, sizeof(int) * (size_t)n_mrows, s));
          }
          hipLaunchKernelGGL(k_accum, dim3(n_chunks), dim3(128), sizeof(long long) * (size_t)k * WORDS_DIM, s, nn, sscale, inv, A, d_perm.p, d_rowptr.p,
                             d_asg.p, d_cent.p, d_ccount.p, d_gacc.p, d_gcnt.p);
          if (n_mrows > 0) hipLaunchKernelGGL(k_finish, dim3(nn), dim3(128), 0, s, inv, A, d_gacc.p, d_gcnt.p, d_cent.p, d_ccount.p);
          VT_TRY(hipMemsetAsync(d_nopen, 0, sizeof(int), s));
          hipLaunchKernelGGL(k_mark, dim3(gN), dim3(256), 0, s, nn, opt->max_iters, A, d_nopen);
        }
        VT_TRY(hipGetLastError());
        int n_open = 0;
        VT_TRY(sc.down(&n_open, d_nopen, 1));   // the iteration's one wait: is a node of this level still open
        VT_TRY(hipStreamSynchronize(s));
        S.host_waits++;
        if (n_open == 0) break;
      }
    }
    // the level's blocks, its leaves' word ids and the next level's nodes
    std::unique_ptr<LevelOut> L(new LevelOut());
    L->nn = nn;
    VT_TRY(hip_first_error({L->n.alloc((size_t)nn), L->desc.alloc((size_t)nn * k * WORDS_DIM), L->link.alloc((size_t)nn * k),
                            L->weight.alloc((size_t)nn * k)}));
    const int last = level == opt->levels - 1;
    int tail[5] = {0, 0, 0, 0, 0};   // leaves and open children of the level, k_rows' three statistics
    {
      KTimer t(ctx, "voctrain_level");
      VT_TRY(hipMemsetAsync(d_st, 0, sizeof(int) * 3, s));
      hipLaunchKernelGGL(k_rows, dim3(gN), dim3(256), 0, s, nn, k, R, last, A, d_ccount.p, d_fleaf.p, d_fopen.p, d_st);
      VT_TRY(prim_scan_excl(tmp, d_fleaf.p, d_leafidx.p, (size_t)R + 1, s));
      VT_TRY(prim_scan_excl(tmp, d_fopen.p, d_openidx.p, (size_t)R + 1, s));
      hipLaunchKernelGGL(k_emit, dim3(nn), dim3(128), 0, s, k, (int)word_base, block_base + nn, A, d_cent.p, d_ccount.p, d_fleaf.p, d_fopen.p,
                         d_leafidx.p, d_openidx.p, L->n.p, L->desc.p, L->link.p, L->weight.p, nm_next);
      hipLaunchKernelGGL(k_next_key, dim3(cdiv(M, 256)), dim3(256), 0, s, M, (unsigned)M0, A, d_perm.p, d_node.p, d_asg.p, d_fopen.p, d_openidx.p,
                         d_key.p, d_perm2.p);
      VT_TRY(prim_sort_pairs(tmp, d_key.p, d_key2.p, d_perm2.p, d_perm.p, (size_t)M, 0u, end_bit, s));   // stable
      VT_TRY(hipMemcpyAsync(d_node.p, d_key2.p, sizeof(int) * (size_t)M, hipMemcpyDeviceToDevice, s));
    }
    VT_TRY(hipGetLastError());
    VT_TRY(sc.down(&tail[0], d_leafidx.p + R, 1)); VT_TRY(sc.down(&tail[1], d_openidx.p + R, 1)); VT_TRY(sc.down(&tail[2], d_st, 3));
    VT_TRY(hipStreamSynchronize(s));
    S.host_waits++;
    S.level_nodes[level] = nn; S.level_split[level] = tail[2]; S.level_max_iters[level] = tail[3]; S.level_capped[level] = tail[4];
    S.depth = level + 1;
    levels.push_back(std::move(L));
    block_base += nn;
    word_base += tail[0];
    nn = tail[1];
    if ((size_t)nn + 1 > NN) return msfm_set_error(ctx, MSFM_E_DEVICE, "%s: level %d opens %d nodes", who, level, nn);
    std::swap(A.nm, nm_next);   // the counts k_emit wrote are the next level's
  }
  // the tree: the levels' blocks back to back
  const int nb = block_base;
  T->k = k; T->n_blocks = nb; T->depth = S.depth; T->n_leaves = word_base; T->h2d_bytes = 0;
  VT_TRY(hip_first_error({T->d_n.alloc((size_t)nb), T->d_desc.alloc((size_t)nb * k * WORDS_DIM), T->d_link.alloc((size_t)nb * k),
                          T->d_weight.alloc((size_t)nb * k)}));
  size_t b0 = 0;
  for (const auto& L : levels) {
    const size_t n = (size_t)L->nn;
    VT_TRY(hipMemcpyAsync(T->d_n.p + b0, L->n.p, sizeof(uint16_t) * n, hipMemcpyDeviceToDevice, s));
    VT_TRY(hipMemcpyAsync(T->d_desc.p + b0 * k * WORDS_DIM, L->desc.p, sizeof(float) * n * k * WORDS_DIM, hipMemcpyDeviceToDevice, s));
    VT_TRY(hipMemcpyAsync(T->d_link.p + b0 * k, L->link.p, sizeof(uint32_t) * n * k, hipMemcpyDeviceToDevice, s));
    VT_TRY(hipMemcpyAsync(T->d_weight.p + b0 * k, L->weight.p, sizeof(float) * n * k, hipMemcpyDeviceToDevice, s));
    b0 += n;
  }
  VT_TRY(sc.finish());
  S.host_waits++;
  S.n_blocks = nb; S.n_leaves = word_base;
  T->trained = true; T->train = S;
  *out = T.release();
  return MSFM_OK;
}

MSFM_API int msfm_voctree_train_stats(const msfm_voctree* T, int* n_images, int64_t* n_features, int* n_blocks, int64_t* n_leaves, int* depth,
                                      int* weight_shift, int* sum_shift, int* host_waits, int32_t* level_nodes, int32_t* level_split,
                                      int32_t* level_max_iters, int32_t* level_capped) {
  if (!T) return MSFM_E_INVAL;
  if (!T->trained) return msfm_set_error(T->ctx, MSFM_E_INVAL, "msfm_voctree_train_stats: the tree was uploaded, not trained");
  const voctrain_stats& S = T->train;
  if (n_images) *n_images = S.n_images;
  if (n_features) *n_features = S.n_features;
  if (n_blocks) *n_blocks = S.n_blocks;
  if (n_leaves) *n_leaves = S.n_leaves;
  if (depth) *depth = S.depth;
  if (weight_shift) *weight_shift = S.weight_shift;
  if (sum_shift) *sum_shift = S.sum_shift;
  if (host_waits) *host_waits = S.host_waits;
  if (level_nodes) std::copy(S.level_nodes, S.level_nodes + VOCTRAIN_MAX_LEVELS, level_nodes);
  if (level_split) std::copy(S.level_split, S.level_split + VOCTRAIN_MAX_LEVELS, level_split);
  if (level_max_iters) std::copy(S.level_max_iters, S.level_max_iters + VOCTRAIN_MAX_LEVELS, level_max_iters);
  if (level_capped) std::copy(S.level_capped, S.level_capped + VOCTRAIN_MAX_LEVELS, level_capped);
  return MSFM_OK;
}
