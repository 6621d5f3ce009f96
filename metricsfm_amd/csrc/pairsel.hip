// Which image pairs are matched at all: the hypotheses of
//   InitialMatchingGraph::match_graph_feature       SfM/src/graph/initial_matching_graph.cc:164-294
//   SimilarityGraph::SimilarityGraphInvFile         SfM/src/graph/similarity_graph.cc:47-117
// from the word id of every feature (include/msfm.h states the semantics, quirks included).
//
// msfm_wordset_create, once per image set, everything resident afterwards.  It is its checks, the upload of the four arrays and
// wordset_create_dev, the device-array core that msfm_wordset_create_from_words (words.hip) calls on word ids and keypoints that
// never left the device; k_heads / k_put_heads / k_map_off live in runs_device.h, which words.hip includes too:
//   k_keys        one thread per feature: key (image << 32 | word), value = the feature index; one stable rocPRIM radix sort, so
//                 the features of a group (a run of equal keys) stay ascending
//   k_heads / k_put_heads   group heads by flag + scan + scatter (the group count stays on the device); k_groups marks per group
//                 "enters the inverted file" and "enters the word table" from the sizes of the group and of its predecessor and
//                 from its place in the image; k_emit compacts both lists (a scan each)
//   similarity    the inverted entries sorted by (word << 32 | image) are the bins; the same two head kernels find them;
//                 k_sim_short gives a bin of up to 16 images a group of 16 lanes, k_sim_long a workgroup.  Integer atomicAdd on
//                 S[a][b] and S[b][a]: order-free, so deterministic
//   ranking       per image the keys (~S << 32 | j), the diagonal left out: k_rank_lds (bitonic, one workgroup per image) up to
//                 PS_RANK_LDS images, a rocPRIM segmented radix sort of the n x n keys above.  Same total order.
// msfm_pair_select, per chunk of rows:
//   k_join        one workgroup per hypothesis (row, slot) walks image i's table in pieces of 256 entries; each thread binary-
//                 searches its entry's word in image j's table.  The count pass sums, the fill pass (after one exclusive scan)
//                 writes the hits in table order - ballot + prefix inside a wave, the four wave counts, and a running base
//                 across the pieces - and gathers both keypoints for geo_fransac_dev.
//   geo_fransac_dev (geo.hip) on those arrays: the kernels of msfm_fundamental_ransac_batch, not copies of them
//   k_gate        one workgroup walks the hypotheses in order: verdict, and the kept pairs compacted in (row, slot) order
#include <climits>
#include <cstring>
#include <memory>

#include "common.h"
#include "pairsel_args.h"
#include "runs_device.h"

struct msfm_wordset {
  msfm_ctx* ctx = nullptr;
  int n = 0, K = 0, num_words = 0;
  int64_t n_inverted = 0, n_mapped = 0, h2d_bytes = 0;
  std::vector<int> feat_off, map_off;   // [n + 1] each
  DevBuf<int> d_feat_off, d_map_off;    // the same on the device
  DevBuf<int> d_map_word, d_map_feat;   // [n_mapped]
  DevBuf<float> d_kp;                   // [feat_off[n]][2]
  DevBuf<int> d_S;                      // [n][n]
  DevBuf<int> d_hyp_img, d_hyp_sim;     // [n][K]
};

struct msfm_pair_set {   // host memory only
  int n_rows = 0, K = 0, n_kept = 0;
  std::vector<int> n_init, n_inliers, pairs, init_off, init_matches;
  std::vector<uint8_t> verdict, init_inlier;
  std::vector<double> F;
};

namespace pairsel {

using namespace runs;   // u64, k_heads, k_put_heads, k_map_off
#define PS_RANK_LDS 2048   // images whose ranking keys (8 bytes each, padded to a power of two) k_rank_lds sorts in LDS
#define PS_SHORT_BIN 16    // images of a bin that one lane group of k_sim_short pairs up

__global__ __launch_bounds__(256) void k_keys(int total, int n, const int* __restrict__ feat_off, const int* __restrict__ word_id,
                                               u64* __restrict__ key, int* __restrict__ val) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= total) return;
  const int img = csr_segment_of(feat_off, n, e);
  key[e] = ((u64)img << 32) | (unsigned)word_id[e];
  val[e] = e - feat_off[img];
}

// per group: does it enter the inverted file, does it enter the word table (0 for g in [G, cap])
__global__ __launch_bounds__(256) void k_groups(int cap, const int* __restrict__ G_p, const int* __restrict__ start, const u64* __restrict__ key,
                                                 const uint8_t* __restrict__ has_words, int* __restrict__ f_inv, int* __restrict__ f_tab) {
  const int g = blockIdx.x * 256 + threadIdx.x;
  if (g > cap) return;
  const int G = *G_p;
  int inv = 0, tab = 0;
  if (g < G) {
    const int b = start[g];
    const int img = (int)(key[b] >> 32);
    if (has_words[img]) {
      const bool first = g == 0 || (int)(key[start[g - 1]] >> 32) != img;
      const bool last = g == G - 1 || (int)(key[start[g + 1]] >> 32) != img;
      inv = (start[g + 1] - b == 1 && !first && !last) ? 1 : 0;   // keep_unique_vector: never g0, never gm
      if (!first) {                                             // keep_unique_idx_vector: g_(k-1) single and not g0
        const int pb = start[g - 1];
        const bool prev_first = g - 1 == 0 || (int)(key[start[g - 2]] >> 32) != img;
        tab = (b - pb == 1 && !prev_first) ? 1 : 0;
      }
    }
  }
  f_inv[g] = inv;
  f_tab[g] = tab;
}

__global__ __launch_bounds__(256) void k_emit(int cap, const int* __restrict__ G_p, const int* __restrict__ start, const u64* __restrict__ key,
                                               const int* __restrict__ val, const int* __restrict__ f_inv, const int* __restrict__ p_inv,
                                               const int* __restrict__ f_tab, const int* __restrict__ p_tab, u64* __restrict__ inv_key,
                                               int* __restrict__ tab_img, int* __restrict__ tab_word, int* __restrict__ tab_feat) {
  const int g = blockIdx.x * 256 + threadIdx.x;
  if (g >= cap || g >= *G_p) return;
  const int b = start[g];
  const int img = (int)(key[b] >> 32), word = (int)(unsigned)key[b];
  if (f_inv[g]) inv_key[p_inv[g]] = ((u64)(unsigned)word << 32) | (unsigned)img;
  if (f_tab[g]) {
    const int t = p_tab[g];
    tab_img[t] = img; tab_word[t] = word; tab_feat[t] = val[b];   // the sort is stable: the lowest feature of the group
  }
}

__device__ static inline void sim_add(int* __restrict__ S, int n, int a, int b) {
  atomicAdd(&S[(size_t)a * n + b], 1);
  atomicAdd(&S[(size_t)b * n + a], 1);
}

// bins of 2 .. PS_SHORT_BIN images: a group of 16 lanes each, the pairs of the bin dealt round
__global__ __launch_bounds__(256) void k_sim_short(const int* __restrict__ B_p, const int* __restrict__ start, const u64* __restrict__ inv_key, int stop,
                                                    int n, int* __restrict__ S) {
  const int B = *B_p;
  const int l = threadIdx.x & 15;
  const int groups = gridDim.x * 16;
  for (int bin = blockIdx.x * 16 + (threadIdx.x >> 4); bin < B; bin += groups) {
    const int b = start[bin], s = start[bin + 1] - b;
    if (s < 2 || s > stop || s > PS_SHORT_BIN) continue;
    for (int p = l; p < s * (s - 1) / 2; p += 16) {
      int a = 0, rem = p;
      while (rem >= s - 1 - a) { rem -= s - 1 - a; a++; }
      sim_add(S, n, (int)(unsigned)inv_key[b + a], (int)(unsigned)inv_key[b + a + 1 + rem]);
    }
  }
}

// longer bins: a workgroup each
__global__ __launch_bounds__(256) void k_sim_long(const int* __restrict__ B_p, const int* __restrict__ start, const u64* __restrict__ inv_key, int stop,
                                                   int n, int* __restrict__ S) {
  const int B = *B_p;
  for (int bin = blockIdx.x; bin < B; bin += gridDim.x) {
    const int b = start[bin], s = start[bin + 1] - b;
    if (s <= PS_SHORT_BIN || s > stop) continue;
    for (int a = 0; a < s - 1; a++) {
      const int ia = (int)(unsigned)inv_key[b + a];
      for (int c = a + 1 + threadIdx.x; c < s; c += 256) sim_add(S, n, ia, (int)(unsigned)inv_key[b + c]);
    }
  }
}

__device__ static inline u64 rank_key(const int* __restrict__ S, int n, int i, int j) {
  return j == i ? ~0ull : (((u64)(~(unsigned)S[(size_t)i * n + j])) << 32) | (unsigned)j;   // similarity descending, then image ascending
}

// one workgroup per image: bitonic sort of P >= n keys in LDS (the padding and the diagonal are all ones and end up last)
__global__ __launch_bounds__(256) void k_rank_lds(int n, int P, int K, const int* __restrict__ S, int* __restrict__ hyp_img, int* __restrict__ hyp_sim) {
  extern __shared__ u64 keys[];
  const int i = blockIdx.x;
  for (int t = threadIdx.x; t < P; t += 256) keys[t] = t < n ? rank_key(S, n, i, t) : ~0ull;
  __syncthreads();
  for (int k = 2; k <= P; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int t = threadIdx.x; t < P; t += 256) {
        const int x = t ^ j;
        if (x > t) {
          const u64 a = keys[t], b = keys[x];
          if (((t & k) == 0) ? (a > b) : (a < b)) { keys[t] = b; keys[x] = a; }
        }
      }
      __syncthreads();
    }
  for (int s = threadIdx.x; s < K; s += 256) {
    hyp_img[(size_t)i * K + s] = (int)(unsigned)keys[s];
    hyp_sim[(size_t)i * K + s] = (int)~(unsigned)(keys[s] >> 32);
  }
}

__global__ __launch_bounds__(256) void k_rank_keys(int n, const int* __restrict__ S, u64* __restrict__ key) {
  const int j = blockIdx.x * 256 + threadIdx.x, i = blockIdx.y;
  if (j < n) key[(size_t)i * n + j] = rank_key(S, n, i, j);
}

__global__ __launch_bounds__(256) void k_rank_take(int n, int K, const u64* __restrict__ key, int* __restrict__ hyp_img, int* __restrict__ hyp_sim) {
  const int s = blockIdx.x * 256 + threadIdx.x, i = blockIdx.y;
  if (s >= K) return;
  const u64 k = key[(size_t)i * n + s];
  hyp_img[(size_t)i * K + s] = (int)(unsigned)k;
  hyp_sim[(size_t)i * K + s] = (int)~(unsigned)(k >> 32);
}

__global__ __launch_bounds__(256) void k_seg_off(int n, int* __restrict__ off) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i <= n) off[i] = i * n;
}

// the feature of image j's table entry with this word, or -1
__device__ static inline int table_find(const int* __restrict__ word, const int* __restrict__ feat, int b, int e, int w) {
  int lo = b, hi = e;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (word[mid] < w) lo = mid + 1; else hi = mid;
  }
  return (lo < e && word[lo] == w) ? feat[lo] : -1;
}

// One workgroup per hypothesis h = r * Ks + s.  FILL = false: count[h] and the 64-bit sum of all counts.  FILL = true: the
// hits in table order into [off[h], off[h + 1]) of matches / pt1 / pt2.
template <bool FILL>
__global__ __launch_bounds__(256) void k_join(int first, int Ks, int K, const int* __restrict__ hyp_img, const int* __restrict__ map_off,
                                               const int* __restrict__ map_word, const int* __restrict__ map_feat, const int* __restrict__ feat_off,
                                               const float2* __restrict__ kp, const int* __restrict__ off, int* __restrict__ count,
                                               u64* __restrict__ total, int2* __restrict__ matches, float2* __restrict__ pt1, float2* __restrict__ pt2) {
  __shared__ int part[4];
  const int h = blockIdx.x;
  const int i = first + h / Ks, j = hyp_img[(size_t)i * K + h % Ks];
  const int bi = map_off[i], ni = map_off[i + 1] - bi, bj = map_off[j], ej = map_off[j + 1];
  const size_t o = FILL ? (size_t)off[h] : 0;
  int base = 0;
  for (int c0 = 0; c0 < ni; c0 += 256) {   // (uniform trip count: the barriers below are reached by every thread)
    const int t = c0 + threadIdx.x;
    int fi = -1, fj = -1;
    if (t < ni) {
      fi = map_feat[bi + t];
      fj = table_find(map_word, map_feat, bj, ej, map_word[bi + t]);
    }
    const bool hit = fj >= 0;
    int piece;
    const int before = wg_rank<4>(hit, part, piece);
    if (FILL && hit) {
      const size_t e = o + base + before;
      matches[e] = make_int2(fi, fj);
      pt1[e] = kp[(size_t)feat_off[i] + fi];
      pt2[e] = kp[(size_t)feat_off[j] + fj];
    }
    base += piece;
  }
  if (!FILL && threadIdx.x == 0) {
    count[h] = base;
    atomicAdd(total, (u64)base);
  }
}

// one workgroup of 1024 walks the hypotheses in order
__global__ __launch_bounds__(1024) void k_gate(int H, int first, int Ks, int K, const int* __restrict__ hyp_img, const int* __restrict__ off,
                                                const uint8_t* __restrict__ ok, const int* __restrict__ n_in, int th_init, int th_inl,
                                                uint8_t* __restrict__ verdict, int2* __restrict__ pairs, int* __restrict__ n_kept) {
  __shared__ int part[16];
  int base = 0;
  for (int c0 = 0; c0 < H; c0 += 1024) {
    const int h = c0 + threadIdx.x;
    int v = -1;
    if (h < H) {
      const int ni = off[h + 1] - off[h];
      v = ni < th_init ? 1 : !ok[h] ? 2 : !(n_in[h] > th_inl) ? 3 : 0;   // :254, :270, :274
      verdict[h] = (uint8_t)v;
    }
    int piece;
    const int before = wg_rank<16>(v == 0, part, piece);
    if (v == 0) {
      const int i = first + h / Ks;
      pairs[base + before] = make_int2(i, hyp_img[(size_t)i * K + h % Ks]);
    }
    base += piece;
  }
  if (threadIdx.x == 0) *n_kept = base;
}

}  // namespace pairsel

#define PS_TRY(e) HIP_TRY(ctx, (e))

MSFM_API void msfm_pair_select_default_options(msfm_pair_select_options* o) {
  if (!o) return;
  o->th_init_matches = 30;
  o->th_inliers = 20;
  o->max_hypotheses = 0;
  msfm_fransac_default_options(&o->fransac);
}

MSFM_API int msfm_wordset_create(msfm_ctx* ctx, int n, const int* n_features, const uint8_t* has_words, const int32_t* word_id, int num_words,
                                 const float* keypoints, int max_hypotheses, msfm_wordset** out) {
  using namespace pairsel;
  const char* who = "msfm_wordset_create";
  if (!ctx) return MSFM_E_INVAL;
  if (!out) return msfm_set_error(ctx, MSFM_E_INVAL, "%s: null argument", who);
  *out = nullptr;
  int K = 0;
  long total_l = 0;
  const std::string bad = pairsel_check_create(n, n_features, has_words, word_id, num_words, keypoints, max_hypotheses, &K, &total_l);
  if (!bad.empty()) return msfm_set_error(ctx, MSFM_E_INVAL, "%s: %s", who, bad.c_str());
  const size_t total = (size_t)total_l;
  std::vector<int> feat_off(n + 1, 0);
  for (int i = 0; i < n; i++) feat_off[i + 1] = feat_off[i] + n_features[i];
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  DevBuf<int> d_feat_off, d_word;
  DevBuf<float> d_kp;
  DevBuf<uint8_t> d_hw;
  DevScope sc(ctx);
  PS_TRY(sc.up(d_feat_off, feat_off)); PS_TRY(sc.up(d_hw, has_words, (size_t)n)); PS_TRY(sc.up(d_word, word_id, total));
  PS_TRY(sc.up(d_kp, keypoints, 2 * total));
  MSFM_TRY(wordset_create_dev(ctx, n, K, num_words, feat_off, d_feat_off, d_hw.p, d_word.p, d_kp, sc.h2d, out));
  sc.dismiss();   // behind the core's finish()
  return MSFM_OK;
}

int wordset_create_dev(msfm_ctx* ctx, int n, int K, int num_words, const std::vector<int>& feat_off, DevBuf<int>& d_feat_off, const uint8_t* d_hw,
                       const int* d_word, DevBuf<float>& d_kp, int64_t h2d_bytes, msfm_wordset** out) {
  using namespace pairsel;
  const int total = feat_off[n];
  Child<msfm_wordset> W = child_new<msfm_wordset>(ctx);
  W->n = n; W->K = K; W->num_words = num_words;
  W->feat_off = feat_off;
  W->map_off.assign(n + 1, 0);
  hipStream_t s = ctx->stream;
  const size_t cap = (size_t)total + 1;   // runs of a sorted array of `total` keys, plus the closing entry
  DevBuf<int> d_map_off, d_map_word, d_map_feat, d_S, d_hyp_img, d_hyp_sim;
  DevBuf<int> d_val, d_val_s, d_flag, d_pos, d_start, d_finv, d_pinv, d_ftab, d_ptab, d_tab_img, d_seg;
  DevBuf<u64> d_key, d_key_s, d_inv, d_inv_s, d_rk, d_rk_s;
  PrimTmp tmp;
  DevScope sc(ctx);
  PS_TRY(d_key.alloc(cap)); PS_TRY(d_key_s.alloc(cap)); PS_TRY(d_val.alloc(cap)); PS_TRY(d_val_s.alloc(cap));
  PS_TRY(d_flag.alloc(cap)); PS_TRY(d_pos.alloc(cap)); PS_TRY(d_start.alloc(cap + 1));
  PS_TRY(d_finv.alloc(cap)); PS_TRY(d_pinv.alloc(cap)); PS_TRY(d_ftab.alloc(cap)); PS_TRY(d_ptab.alloc(cap));
  PS_TRY(d_inv.alloc(cap)); PS_TRY(d_inv_s.alloc(cap)); PS_TRY(d_tab_img.alloc(cap)); PS_TRY(d_map_word.alloc(cap)); PS_TRY(d_map_feat.alloc(cap));
  PS_TRY(d_map_off.alloc((size_t)n + 1));
  PS_TRY(d_S.alloc((size_t)n * n)); PS_TRY(d_hyp_img.alloc((size_t)n * K)); PS_TRY(d_hyp_sim.alloc((size_t)n * K));
  PS_TRY(hipMemsetAsync(d_S.p, 0, sizeof(int) * (size_t)n * n, s));
  const int gcap = cdiv((long)cap, 256);
  const int* d_G = d_pos.p + total;   // runs found by the scan over [0, total]
  int n_inv = 0, n_tab = 0;
  if (total) {
    {
      KTimer t(ctx, "pairsel_keys");
      hipLaunchKernelGGL(k_keys, dim3(cdiv(total, 256)), dim3(256), 0, s, total, n, d_feat_off.p, d_word, d_key.p, d_val.p);
    }
    {
      const unsigned end_bit = 32u + (unsigned)bits_for((unsigned)(n - 1));
      KTimer t(ctx, "pairsel_sort_words");
      PS_TRY(prim_sort_pairs(tmp, d_key.p, d_key_s.p, d_val.p, d_val_s.p, (size_t)total, 0u, end_bit, s));   // stable
    }
    {
      KTimer t(ctx, "pairsel_groups");
      hipLaunchKernelGGL(k_heads, dim3(gcap), dim3(256), 0, s, total, d_key_s.p, 0, d_flag.p);
      PS_TRY(prim_scan_excl(tmp, d_flag.p, d_pos.p, cap, s));
      hipLaunchKernelGGL(k_put_heads, dim3(gcap), dim3(256), 0, s, total, d_flag.p, d_pos.p, d_start.p);
      hipLaunchKernelGGL(k_groups, dim3(gcap), dim3(256), 0, s, total, d_G, d_start.p, d_key_s.p, d_hw, d_finv.p, d_ftab.p);
      PS_TRY(prim_scan_excl(tmp, d_finv.p, d_pinv.p, cap, s));
      PS_TRY(prim_scan_excl(tmp, d_ftab.p, d_ptab.p, cap, s));
      hipLaunchKernelGGL(k_emit, dim3(gcap), dim3(256), 0, s, total, d_G, d_start.p, d_key_s.p, d_val_s.p, d_finv.p, d_pinv.p, d_ftab.p, d_ptab.p,
                         d_inv.p, d_tab_img.p, d_map_word.p, d_map_feat.p);
    }
    PS_TRY(hipGetLastError());
    // the two list lengths size the second sort and the resident tables: the one read-back of the set-up
    PS_TRY(hipMemcpyAsync(&n_inv, d_pinv.p + total, sizeof(int), hipMemcpyDeviceToHost, s));
    PS_TRY(hipMemcpyAsync(&n_tab, d_ptab.p + total, sizeof(int), hipMemcpyDeviceToHost, s));
    PS_TRY(hipStreamSynchronize(s));
  }
  W->n_inverted = n_inv; W->n_mapped = n_tab;
  hipLaunchKernelGGL(k_map_off, dim3(cdiv(n + 1, 256)), dim3(256), 0, s, n, n_tab, d_tab_img.p, d_map_off.p);
  if (n_inv > 1 && num_words / 100 >= 2) {
    {
      const unsigned end_bit = 32u + (unsigned)bits_for((unsigned)num_words);
      KTimer t(ctx, "pairsel_sort_bins");
      PS_TRY(prim_sort_keys(tmp, d_inv.p, d_inv_s.p, (size_t)n_inv, 0u, end_bit, s));
    }
    KTimer t(ctx, "pairsel_similarity");
    const int icap = cdiv((long)n_inv + 1, 256);
    hipLaunchKernelGGL(k_heads, dim3(icap), dim3(256), 0, s, n_inv, d_inv_s.p, 32, d_flag.p);
    PS_TRY(prim_scan_excl(tmp, d_flag.p, d_pos.p, (size_t)n_inv + 1, s));
    hipLaunchKernelGGL(k_put_heads, dim3(icap), dim3(256), 0, s, n_inv, d_flag.p, d_pos.p, d_start.p);
    const int* d_B = d_pos.p + n_inv;
    const int stop = num_words / 100;   // :109
    hipLaunchKernelGGL(k_sim_short, dim3(std::min(4096, cdiv(n_inv, 32))), dim3(256), 0, s, d_B, d_start.p, d_inv_s.p, stop, n, d_S.p);
    if (stop > PS_SHORT_BIN) hipLaunchKernelGGL(k_sim_long, dim3(std::min(2048, cdiv(n_inv, PS_SHORT_BIN))), dim3(256), 0, s, d_B, d_start.p, d_inv_s.p, stop, n, d_S.p);
  }
  if (n <= PS_RANK_LDS) {
    int P = 2;
    while (P < n) P <<= 1;
    KTimer t(ctx, "pairsel_rank_lds");
    hipLaunchKernelGGL(k_rank_lds, dim3(n), dim3(256), sizeof(u64) * (size_t)P, s, n, P, K, d_S.p, d_hyp_img.p, d_hyp_sim.p);
  } else {
    PS_TRY(d_rk.alloc((size_t)n * n)); PS_TRY(d_rk_s.alloc((size_t)n * n)); PS_TRY(d_seg.alloc((size_t)n + 1));
    KTimer t(ctx, "pairsel_rank_rocprim");
    hipLaunchKernelGGL(k_seg_off, dim3(cdiv(n + 1, 256)), dim3(256), 0, s, n, d_seg.p);
    hipLaunchKernelGGL(k_rank_keys, dim3(cdiv(n, 256), n), dim3(256), 0, s, n, d_S.p, d_rk.p);
    PS_TRY(prim_seg_sort_keys(tmp, d_rk.p, d_rk_s.p, (unsigned)((size_t)n * n), (unsigned)n, d_seg.p, d_seg.p + 1, 0, 64, s));
    hipLaunchKernelGGL(k_rank_take, dim3(cdiv(K, 256), n), dim3(256), 0, s, n, K, d_rk_s.p, d_hyp_img.p, d_hyp_sim.p);
  }
  PS_TRY(hipGetLastError());
  PS_TRY(sc.down(W->map_off.data(), d_map_off.p, (size_t)n + 1));
  PS_TRY(sc.finish());
  W->h2d_bytes = h2d_bytes;
  W->d_feat_off.swap(d_feat_off); W->d_map_off.swap(d_map_off); W->d_map_word.swap(d_map_word); W->d_map_feat.swap(d_map_feat);
  W->d_kp.swap(d_kp); W->d_S.swap(d_S); W->d_hyp_img.swap(d_hyp_img); W->d_hyp_sim.swap(d_hyp_sim);
  *out = W.release();
  return MSFM_OK;
}

MSFM_API int msfm_wordset_size(const msfm_wordset* W, int* n_images, int* n_hypotheses, int64_t* n_inverted, int64_t* n_mapped, int64_t* h2d_bytes) {
  if (!W) return MSFM_E_INVAL;
  if (n_images) *n_images = W->n;
  if (n_hypotheses) *n_hypotheses = W->K;
  if (n_inverted) *n_inverted = W->n_inverted;
  if (n_mapped) *n_mapped = W->n_mapped;
  if (h2d_bytes) *h2d_bytes = W->h2d_bytes;
  return MSFM_OK;
}

MSFM_API int msfm_wordset_fetch(const msfm_wordset* W, int32_t* similarity, int32_t* hyp_img, int32_t* hyp_sim, int32_t* map_off, int32_t* map_word,
                                int32_t* map_feat) {
  if (!W) return MSFM_E_INVAL;
  msfm_ctx* ctx = W->ctx;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  DevScope sc(ctx);
  const size_t n = (size_t)W->n;
  PS_TRY(sc.down(similarity, W->d_S.p, n * n));
  PS_TRY(sc.down(hyp_img, W->d_hyp_img.p, n * W->K));
  PS_TRY(sc.down(hyp_sim, W->d_hyp_sim.p, n * W->K));
  PS_TRY(sc.down(map_word, W->d_map_word.p, (size_t)W->n_mapped));
  PS_TRY(sc.down(map_feat, W->d_map_feat.p, (size_t)W->n_mapped));
  PS_TRY(sc.finish());
  if (map_off) std::copy(W->map_off.begin(), W->map_off.end(), map_off);
  return MSFM_OK;
}

MSFM_API void msfm_wordset_destroy(msfm_wordset* W) { msfm_child_destroy(W); }

MSFM_API int msfm_pair_select(msfm_wordset* W, int first, int n_rows, const msfm_pair_select_options* opt_in, msfm_pair_set** out) {
  using namespace pairsel;
  const char* who = "msfm_pair_select";
  if (!W) return MSFM_E_INVAL;
  msfm_ctx* ctx = W->ctx;
  if (!out) return msfm_set_error(ctx, MSFM_E_INVAL, "%s: null argument", who);
  *out = nullptr;
  msfm_pair_select_options opt;
  if (opt_in) opt = *opt_in; else msfm_pair_select_default_options(&opt);
  int Ks = 0;
  const std::string bad = pairsel_check_select(W->n, W->K, first, n_rows, &opt, &Ks);
  if (!bad.empty()) return msfm_set_error(ctx, MSFM_E_INVAL, "%s: %s", who, bad.c_str());
  const int H = n_rows * Ks, K = W->K;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  std::unique_ptr<msfm_pair_set> R(new msfm_pair_set());
  R->n_rows = n_rows; R->K = Ks;
  R->init_off.assign((size_t)H + 1, 0);
  DevBuf<int> d_count, d_off, d_nin, d_nkept;
  DevBuf<u64> d_total;
  DevBuf<int2> d_match, d_pairs;
  DevBuf<float2> d_p1, d_p2;
  DevBuf<double> d_F;
  DevBuf<uint8_t> d_in, d_ok, d_verdict;
  PrimTmp tmp;
  DevScope sc(ctx);
  PS_TRY(d_count.alloc((size_t)H + 1)); PS_TRY(d_off.alloc((size_t)H + 1)); PS_TRY(d_total.alloc(1));
  PS_TRY(hipMemsetAsync(d_count.p + H, 0, sizeof(int), s)); PS_TRY(hipMemsetAsync(d_total.p, 0, sizeof(u64), s));
  const float2* kp = reinterpret_cast<const float2*>(W->d_kp.p);
  {
    KTimer t(ctx, "pairsel_join_count");
    hipLaunchKernelGGL(k_join<false>, dim3(H), dim3(256), 0, s, first, Ks, K, W->d_hyp_img.p, W->d_map_off.p, W->d_map_word.p, W->d_map_feat.p,
                       W->d_feat_off.p, kp, (const int*)nullptr, d_count.p, d_total.p, (int2*)nullptr, (float2*)nullptr, (float2*)nullptr);
    PS_TRY(prim_scan_excl(tmp, d_count.p, d_off.p, (size_t)H + 1, s));
  }
  PS_TRY(hipGetLastError());
  // the first wait: geo_fransac_dev wants the offsets on the host, and the match arrays are sized by their last entry
  u64 total64 = 0;
  PS_TRY(hipMemcpyAsync(&total64, d_total.p, sizeof(u64), hipMemcpyDeviceToHost, s));
  PS_TRY(sc.down(R->init_off.data(), d_off.p, (size_t)H + 1));
  PS_TRY(hipStreamSynchronize(s));
  if (total64 > (u64)INT_MAX)
    return msfm_set_error(ctx, MSFM_E_INVAL, "%s: the %d rows join %llu matches, more than 2^31 - 1: use smaller chunks", who, n_rows, total64);
  const int total = (int)total64;
  const size_t tx = (size_t)std::max(1, total);
  PS_TRY(d_match.alloc(tx)); PS_TRY(d_p1.alloc(tx)); PS_TRY(d_p2.alloc(tx)); PS_TRY(d_in.alloc(tx));
  PS_TRY(d_F.alloc(9 * (size_t)H)); PS_TRY(d_nin.alloc(H)); PS_TRY(d_ok.alloc(H)); PS_TRY(d_verdict.alloc(H)); PS_TRY(d_pairs.alloc(H));
  PS_TRY(d_nkept.alloc(1));
  if (total) {
    KTimer t(ctx, "pairsel_join_fill");
    hipLaunchKernelGGL(k_join<true>, dim3(H), dim3(256), 0, s, first, Ks, K, W->d_hyp_img.p, W->d_map_off.p, W->d_map_word.p, W->d_map_feat.p,
                       W->d_feat_off.p, kp, d_off.p, (int*)nullptr, (u64*)nullptr, d_match.p, d_p1.p, d_p2.p);
  }
  PS_TRY(hipGetLastError());
  MSFM_TRY(geo_fransac_dev(ctx, H, R->init_off.data(), d_off.p, reinterpret_cast<const float*>(d_p1.p), reinterpret_cast<const float*>(d_p2.p),
                           &opt.fransac, d_F.p, d_in.p, d_nin.p, d_ok.p));
  {
    KTimer t(ctx, "pairsel_gate");
    hipLaunchKernelGGL(k_gate, dim3(1), dim3(1024), 0, s, H, first, Ks, K, W->d_hyp_img.p, d_off.p, d_ok.p, d_nin.p, (int)opt.th_init_matches,
                       (int)opt.th_inliers, d_verdict.p, d_pairs.p, d_nkept.p);
  }
  PS_TRY(hipGetLastError());
  R->n_inliers.resize(H); R->verdict.resize(H); R->F.resize(9 * (size_t)H); R->pairs.resize(2 * (size_t)H);
  R->init_matches.resize(2 * (size_t)total); R->init_inlier.resize(total);
  PS_TRY(sc.down(R->n_inliers.data(), d_nin.p, (size_t)H)); PS_TRY(sc.down(R->verdict.data(), d_verdict.p, (size_t)H));
  PS_TRY(sc.down(R->F.data(), d_F.p, 9 * (size_t)H));
  PS_TRY(sc.down(R->pairs.data(), reinterpret_cast<const int*>(d_pairs.p), 2 * (size_t)H));
  PS_TRY(sc.down(R->init_matches.data(), reinterpret_cast<const int*>(d_match.p), 2 * (size_t)total));
  PS_TRY(sc.down(R->init_inlier.data(), d_in.p, (size_t)total));
  PS_TRY(sc.down(&R->n_kept, d_nkept.p, 1));
  PS_TRY(sc.finish());   // the second wait; the scratch above is released on return
  R->pairs.resize(2 * (size_t)R->n_kept);
  R->n_init.resize(H);
  for (int h = 0; h < H; h++) R->n_init[h] = R->init_off[h + 1] - R->init_off[h];
  *out = R.release();
  return MSFM_OK;
}

MSFM_API int msfm_pair_set_size(const msfm_pair_set* R, int* n_rows, int* n_hypotheses, int* n_kept, int64_t* n_init_total) {
  if (!R) return MSFM_E_INVAL;
  if (n_rows) *n_rows = R->n_rows;
  if (n_hypotheses) *n_hypotheses = R->K;
  if (n_kept) *n_kept = R->n_kept;
  if (n_init_total) *n_init_total = R->init_off.back();
  return MSFM_OK;
}

MSFM_API int msfm_pair_set_fetch(const msfm_pair_set* R, int32_t* n_init, int32_t* n_inliers, uint8_t* verdict, int32_t* pairs, double* F,
                                 int32_t* init_off, int32_t* init_matches, uint8_t* init_inlier) {
  if (!R) return MSFM_E_INVAL;
  if (n_init) std::copy(R->n_init.begin(), R->n_init.end(), n_init);
  if (n_inliers) std::copy(R->n_inliers.begin(), R->n_inliers.end(), n_inliers);
  if (verdict) std::copy(R->verdict.begin(), R->verdict.end(), verdict);
  if (pairs) std::copy(R->pairs.begin(), R->pairs.end(), pairs);
  if (F) std::copy(R->F.begin(), R->F.end(), F);
  if (init_off) std::copy(R->init_off.begin(), R->init_off.end(), init_off);
  if (init_matches) std::copy(R->init_matches.begin(), R->init_matches.end(), init_matches);
  if (init_inlier) std::copy(R->init_inlier.begin(), R->init_inlier.end(), init_inlier);
  return MSFM_OK;
}

MSFM_API void msfm_pair_set_destroy(msfm_pair_set* R) { delete R; }
