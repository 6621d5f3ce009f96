// The visual word of every feature: the vocabulary-tree descent of
//   Database::BuildWords / GenerateWordsForImage          SfM/src/database.cc:745-867
//   fbow::Vocabulary::_transform<L2_avx_generic>          SfM/thirdparty/fbow/include/fbow/fbow.h:247-261, :417-452
// on the float32 rows a descriptor set already holds (include/msfm.h states the semantics, quirks included).
//
// msfm_voctree_create   the checks of words_args.h, one upload, and k_relay: a node's 128 floats are stored as 8 runs of 16, run j
//                       holding the elements j, j + 8, ... - what lane j of the descent reads with four 16-byte loads
// msfm_descset_words    k_descend: eight lanes per feature, lane j keeps partial sum j of the reference's eight-wide register and
//                       the feature's elements j, j + 8, ... for the whole descent; per node 16 subtract / multiply / add steps
//                       (never fused) and a butterfly over 1, 2, 4, which is the reference's hadd tree in every lane because a
//                       binary32 addition is commutative.  The winner is kept with a strict < in node order.  Lane 0 writes the
//                       word, the leaf weight, the sort key (image << 32 | word, value = the flat feature index) and raises the
//                       image's maximum with an integer atomicMax.
//                       bags: one stable rocPRIM radix sort, the group heads of runs_device.h, and k_bags: one lane per group adds
//                       the leaf weights in feature order.  Features without a word sort behind the last image and are dropped.
// msfm_wordset_create_from_words   device copies of the set's keypoints into one flat array, then pairsel.hip's core
#include <climits>
#include <memory>

#include "common.h"
#include "pairsel_args.h"
#include "runs_device.h"
#include "words_args.h"
#include "words_dist.h"

struct msfm_word_result {
  msfm_ctx* ctx = nullptr;
  const msfm_descset* set = nullptr;   // compared, never read
  unsigned long generation = 0;
  int n = 0, num_words = 0;
  int64_t total = 0, n_bow = 0, n_unassigned = 0;
  std::vector<int> feat_off, bow_off, image_max;   // [n + 1], [n + 1], [n]
  std::vector<uint8_t> has_words;                  // [n]
  DevBuf<uint8_t> d_hw;                            // [n]
  DevBuf<int> d_word;                              // [total], -1: no word
  DevBuf<float> d_leaf_w;                          // [total]
  DevBuf<int> d_image_max, d_bow_off;              // [n], [n + 1]
  DevBuf<int> d_bow_word;                          // [n_bow] (blocks of `total` entries)
  DevBuf<float> d_bow_weight;
};

namespace words {

using namespace runs;

__global__ __launch_bounds__(256) void k_relay(size_t n_floats, const float* __restrict__ raw, float* __restrict__ out) {
  const size_t o = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (o >= n_floats) return;
  const size_t node = o >> 7;
  const int r = (int)(o & 127), j = r >> 4, t = r & 15;
  out[o] = raw[node * WORDS_DIM + j + 8 * t];
}

__global__ __launch_bounds__(256) void k_unrelay(size_t n_floats, const float* __restrict__ relayed, float* __restrict__ out) {
  const size_t o = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (o >= n_floats) return;
  out[o] = relayed[(o >> 7) * WORDS_DIM + relay_pos((int)(o & 127))];
}

// Eight lanes per feature e, 32 features per workgroup.  The loops run while any lane of the wave needs them, so the shuffles
// are reached by whole waves; what a finished or idle group computes is discarded.
__global__ __launch_bounds__(256) void k_descend(int total, int n, int k, const int* __restrict__ feat_off, const float* const* __restrict__ rows,
                                                  const uint8_t* __restrict__ has_words, const uint16_t* __restrict__ block_n,
                                                  const float* __restrict__ desc, const uint32_t* __restrict__ link, const float* __restrict__ weight,
                                                  int* __restrict__ word_id, float* __restrict__ leaf_w, u64* __restrict__ key, int* __restrict__ val,
                                                  int* __restrict__ image_max, int* __restrict__ n_unassigned) {
  const long e_l = (long)blockIdx.x * 32 + (threadIdx.x >> 3);
  const int j = threadIdx.x & 7;
  const bool inside = e_l < total;
  const int e = inside ? (int)e_l : 0;
  int img = 0;
  bool go = false;
  float f[16];
#pragma unroll
  for (int t = 0; t < 16; t++) f[t] = 0.f;
  if (inside) {
    img = csr_segment_of(feat_off, n, e);
    go = has_words[img] != 0;
    if (go) {
      const float* row = rows[img] + (size_t)(e - feat_off[img]) * WORDS_DIM;
#pragma unroll
      for (int t = 0; t < 16; t++) f[t] = row[j + 8 * t];
    }
  }
  const bool counted = go;
  int blk = 0, word = -1;
  float wt = 0.f;
  for (int level = 0; level < WORDS_MAX_DEPTH; level++) {
    if (!__any(go)) break;
    const int N = go ? (int)block_n[blk] : 0;
    const float* nb = desc + ((size_t)blk * k) * WORDS_DIM + j * 16;
    float best = 4294967296.0f;   // numeric_limits<uint32_t>::max() as a float
    int best_i = -1;
    for (int i = 0; i < k; i++) {
      if (!__any(i < N)) break;
      float s = 0.f;
      if (i < N) s = part16(f, nb + (size_t)i * WORDS_DIM);
      s = add8(s);
      if (i < N && s < best) { best = s; best_i = i; }   // strict: a tie stays with the lower node, a NaN never wins
    }
    if (go) {
      if (best_i < 0) go = false;   // no node won: no word (the departure include/msfm.h states)
      else {
        const uint32_t l = link[(size_t)blk * k + best_i];
        if (l & WORDS_LEAF) { word = (int)(l & 0x7fffffffu); wt = weight[(size_t)blk * k + best_i]; go = false; }
        else if (l == 0) go = false;   // while (!leaf && id != 0)
        else blk = (int)l;
      }
    }
  }
  if (!inside || j != 0) return;
  word_id[e] = word;
  leaf_w[e] = wt;
  val[e] = e;
  key[e] = word >= 0 ? (((u64)img << 32) | (unsigned)word) : ((u64)n << 32);
  if (word >= 0) atomicMax(&image_max[img], word);
  else if (counted) atomicAdd(n_unassigned, 1);
}

// per group of the sorted keys: its image (n: the features without a word), its word, the sum of its leaf weights in feature order
__global__ __launch_bounds__(256) void k_bags(int cap, int n, const int* __restrict__ G_p, const int* __restrict__ start, const u64* __restrict__ key,
                                               const int* __restrict__ val, const float* __restrict__ leaf_w, int* __restrict__ grp_img,
                                               int* __restrict__ bow_word, float* __restrict__ bow_weight) {
  const int g = blockIdx.x * 256 + threadIdx.x;
  if (g >= cap || g >= *G_p) return;
  const int b = start[g], e = start[g + 1];
  const int img = (int)(key[b] >> 32);
  grp_img[g] = img;
  if (img >= n) return;
  float w = 0.0f;
  for (int x = b; x < e; x++) w = w + leaf_w[val[x]];   // the sort is stable: ascending feature
  bow_word[g] = (int)(unsigned)key[b];
  bow_weight[g] = w;
}

// bow_off[i] = groups of images below i (the groups without a word carry image n and come last)
__global__ __launch_bounds__(256) void k_bow_off(int n, const int* __restrict__ G_p, const int* __restrict__ grp_img, int* __restrict__ bow_off) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i > n) return;
  int lo = 0, hi = *G_p;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (grp_img[mid] < i) lo = mid + 1; else hi = mid;
  }
  bow_off[i] = lo;
}

}  // namespace words

#define WD_TRY(e) HIP_TRY(ctx, (e))

MSFM_API int msfm_voctree_create(msfm_ctx* ctx, int k, int n_blocks, const uint16_t* block_n, const float* node_desc, const uint32_t* node_link,
                                 const float* node_weight, msfm_voctree** out) {
  using namespace words;
  const char* who = "msfm_voctree_create";
  if (!ctx) return MSFM_E_INVAL;
  if (!out) return msfm_set_error(ctx, MSFM_E_INVAL, "%s: null argument", who);
  *out = nullptr;
  int depth = 0;
  int64_t n_leaves = 0;
  const std::string bad = words_check_tree(k, n_blocks, block_n, node_desc, node_link, node_weight, &depth, &n_leaves);
  if (!bad.empty()) return msfm_set_error(ctx, MSFM_E_INVAL, "%s: %s", who, bad.c_str());
  Child<msfm_voctree> T = child_new<msfm_voctree>(ctx);
  T->k = k; T->n_blocks = n_blocks; T->depth = depth; T->n_leaves = n_leaves;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  const size_t nodes = (size_t)n_blocks * k;
  DevBuf<float> d_raw;
  DevScope sc(ctx);
  WD_TRY(sc.up(T->d_n, block_n, (size_t)n_blocks)); WD_TRY(sc.up(T->d_link, node_link, nodes)); WD_TRY(sc.up(T->d_weight, node_weight, nodes));
  WD_TRY(sc.up(d_raw, node_desc, nodes * WORDS_DIM));
  WD_TRY(T->d_desc.alloc(nodes * WORDS_DIM));
  {
    KTimer t(ctx, "words_relay");
    hipLaunchKernelGGL(k_relay, dim3(cdiv((long)(nodes * WORDS_DIM), 256)), dim3(256), 0, s, nodes * WORDS_DIM, d_raw.p, T->d_desc.p);
  }
  WD_TRY(hipGetLastError());
  WD_TRY(sc.finish());
  T->h2d_bytes = sc.h2d;
  *out = T.release();
  return MSFM_OK;
}

MSFM_API int msfm_voctree_size(const msfm_voctree* T, int* k, int* n_blocks, int* depth, int64_t* n_leaves, int64_t* h2d_bytes) {
  if (!T) return MSFM_E_INVAL;
  if (k) *k = T->k;
  if (n_blocks) *n_blocks = T->n_blocks;
  if (depth) *depth = T->depth;
  if (n_leaves) *n_leaves = T->n_leaves;
  if (h2d_bytes) *h2d_bytes = T->h2d_bytes;
  return MSFM_OK;
}

MSFM_API int msfm_voctree_fetch(const msfm_voctree* T, uint16_t* block_n, float* node_desc, uint32_t* node_link, float* node_weight,
                                uint16_t* block_leaf, uint32_t* block_parent) {
  using namespace words;
  if (!T) return MSFM_E_INVAL;
  msfm_ctx* ctx = T->ctx;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  const size_t nb = (size_t)T->n_blocks, nodes = nb * T->k;
  std::vector<uint16_t> n(nb);
  std::vector<uint32_t> link(nodes);
  DevBuf<float> d_raw;
  DevScope sc(ctx);
  if (node_desc) {
    WD_TRY(d_raw.alloc(nodes * WORDS_DIM));
    hipLaunchKernelGGL(k_unrelay, dim3(cdiv((long)(nodes * WORDS_DIM), 256)), dim3(256), 0, ctx->stream, nodes * WORDS_DIM, T->d_desc.p, d_raw.p);
    WD_TRY(hipGetLastError());
    WD_TRY(sc.down(node_desc, d_raw.p, nodes * WORDS_DIM));
  }
  WD_TRY(sc.down(n.data(), T->d_n.p, nb)); WD_TRY(sc.down(link.data(), T->d_link.p, nodes));
  WD_TRY(sc.down(node_weight, T->d_weight.p, nodes));
  WD_TRY(sc.finish());
  if (block_n) std::copy(n.begin(), n.end(), block_n);
  if (node_link) std::copy(link.begin(), link.end(), node_link);
  for (size_t b = 0; b < nb; b++) {
    if (block_leaf) block_leaf[b] = 1;
    if (block_parent) block_parent[b] = 0;
  }
  for (size_t b = 0; b < nb; b++)
    for (int i = 0; i < n[b]; i++) {
      const uint32_t l = link[b * T->k + i];
      if (l & WORDS_LEAF) continue;
      if (block_leaf) block_leaf[b] = 0;
      if (block_parent && l != 0 && l < nb) block_parent[l] = (uint32_t)b;
    }
  return MSFM_OK;
}

MSFM_API void msfm_voctree_destroy(msfm_voctree* T) { msfm_child_destroy(T); }

MSFM_API int msfm_descset_words(msfm_descset* set, const msfm_voctree* T, int min_features, msfm_word_result** out) {
  using namespace words;
  const char* who = "msfm_descset_words";
  if (!set) return MSFM_E_INVAL;
  DescView V;
  descset_view(set, &V);
  msfm_ctx* ctx = V.ctx;
  if (!T || !out) return msfm_set_error(ctx, MSFM_E_INVAL, "%s: null argument", who);
  *out = nullptr;
  if (T->ctx != ctx) return msfm_set_error(ctx, MSFM_E_INVAL, "%s: the tree belongs to another context", who);
  if (min_features < 0) return msfm_set_error(ctx, MSFM_E_INVAL, "%s: min_features = %d is negative", who, min_features);
  const int n = V.n_images;
  Child<msfm_word_result> R = child_new<msfm_word_result>(ctx);
  R->set = set; R->generation = V.generation; R->n = n;
  R->feat_off.assign(n + 1, 0); R->bow_off.assign(n + 1, 0); R->image_max.assign(n, 0); R->has_words.assign(n, 0);
  long total_l = 0;
  for (int i = 0; i < n; i++) {
    total_l += V.count[i];
    if (total_l > 0x7fffffffL) return msfm_set_error(ctx, MSFM_E_INVAL, "%s: more than 2^31 features", who);
    R->feat_off[i + 1] = (int)total_l;
    R->has_words[i] = V.count[i] > min_features ? 1 : 0;   // database.cc:798, strict
  }
  const int total = (int)total_l;
  R->total = total;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  const size_t cap = (size_t)total + 1, tx = (size_t)std::max(1, total);
  DevBuf<int> d_feat_off, d_val, d_val_s, d_flag, d_pos, d_start, d_grp_img, d_nun;
  DevBuf<const float*> d_rows;
  DevBuf<u64> d_key, d_key_s;
  PrimTmp tmp;
  DevScope sc(ctx);
  WD_TRY(sc.up(d_feat_off, R->feat_off)); WD_TRY(sc.up(R->d_hw, R->has_words)); WD_TRY(sc.up(d_rows, V.f32));
  WD_TRY(R->d_word.alloc(tx)); WD_TRY(R->d_leaf_w.alloc(tx)); WD_TRY(R->d_image_max.alloc(n)); WD_TRY(R->d_bow_off.alloc((size_t)n + 1));
  WD_TRY(R->d_bow_word.alloc(tx)); WD_TRY(R->d_bow_weight.alloc(tx));
  WD_TRY(d_key.alloc(cap)); WD_TRY(d_key_s.alloc(cap)); WD_TRY(d_val.alloc(cap)); WD_TRY(d_val_s.alloc(cap));
  WD_TRY(d_flag.alloc(cap)); WD_TRY(d_pos.alloc(cap)); WD_TRY(d_start.alloc(cap + 1)); WD_TRY(d_grp_img.alloc(cap)); WD_TRY(d_nun.alloc(1));
  WD_TRY(hipMemsetAsync(R->d_image_max.p, 0, sizeof(int) * (size_t)n, s));   // max(0, largest word id), database.cc:864-866
  WD_TRY(hipMemsetAsync(R->d_bow_off.p, 0, sizeof(int) * ((size_t)n + 1), s));
  WD_TRY(hipMemsetAsync(d_nun.p, 0, sizeof(int), s));
  int n_unassigned = 0;
  if (total) {
    {
      KTimer t(ctx, "words_descend");
      hipLaunchKernelGGL(k_descend, dim3(cdiv(total, 32)), dim3(256), 0, s, total, n, T->k, d_feat_off.p, d_rows.p, R->d_hw.p, T->d_n.p, T->d_desc.p,
                         T->d_link.p, T->d_weight.p, R->d_word.p, R->d_leaf_w.p, d_key.p, d_val.p, R->d_image_max.p, d_nun.p);
    }
    {
      const unsigned end_bit = 32u + (unsigned)bits_for((unsigned)n);   // image n: the features without a word
      KTimer t(ctx, "words_sort");
      WD_TRY(prim_sort_pairs(tmp, d_key.p, d_key_s.p, d_val.p, d_val_s.p, (size_t)total, 0u, end_bit, s));   // stable
    }
    {
      KTimer t(ctx, "words_bags");
      const int gcap = cdiv((long)cap, 256);
      const int* d_G = d_pos.p + total;   // runs found by the scan over [0, total]
      hipLaunchKernelGGL(k_heads, dim3(gcap), dim3(256), 0, s, total, d_key_s.p, 0, d_flag.p);
      WD_TRY(prim_scan_excl(tmp, d_flag.p, d_pos.p, cap, s));
      hipLaunchKernelGGL(k_put_heads, dim3(gcap), dim3(256), 0, s, total, d_flag.p, d_pos.p, d_start.p);
      hipLaunchKernelGGL(k_bags, dim3(gcap), dim3(256), 0, s, total, n, d_G, d_start.p, d_key_s.p, d_val_s.p, R->d_leaf_w.p, d_grp_img.p,
                         R->d_bow_word.p, R->d_bow_weight.p);
      hipLaunchKernelGGL(k_bow_off, dim3(cdiv(n + 1, 256)), dim3(256), 0, s, n, d_G, d_grp_img.p, R->d_bow_off.p);
    }
    WD_TRY(hipGetLastError());
  }
  // the one wait: the bag sizes, with the per-image maxima and the count of features without a word
  WD_TRY(sc.down(R->bow_off.data(), R->d_bow_off.p, (size_t)n + 1));
  WD_TRY(sc.down(R->image_max.data(), R->d_image_max.p, (size_t)n));
  WD_TRY(sc.down(&n_unassigned, d_nun.p, 1));
  WD_TRY(sc.finish());
  R->n_bow = R->bow_off[n];
  R->n_unassigned = n_unassigned;
  for (int i = 0; i < n; i++) R->num_words = std::max(R->num_words, R->image_max[i]);   // the last running max_words_id_
  *out = R.release();
  return MSFM_OK;
}

MSFM_API int msfm_word_result_size(const msfm_word_result* R, int* n_images, int64_t* n_features, int64_t* n_bow, int* num_words,
                                   int64_t* n_unassigned) {
  if (!R) return MSFM_E_INVAL;
  if (n_images) *n_images = R->n;
  if (n_features) *n_features = R->total;
  if (n_bow) *n_bow = R->n_bow;
  if (num_words) *num_words = R->num_words;
  if (n_unassigned) *n_unassigned = R->n_unassigned;
  return MSFM_OK;
}

MSFM_API int msfm_word_result_fetch(const msfm_word_result* R, int32_t* feat_off, uint8_t* has_words, int32_t* word_id, int32_t* image_max_id,
                                    int32_t* bow_off, int32_t* bow_word, float* bow_weight) {
  if (!R) return MSFM_E_INVAL;
  msfm_ctx* ctx = R->ctx;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  DevScope sc(ctx);
  WD_TRY(sc.down(word_id, R->d_word.p, (size_t)R->total));
  WD_TRY(sc.down(bow_word, R->d_bow_word.p, (size_t)R->n_bow));
  WD_TRY(sc.down(bow_weight, R->d_bow_weight.p, (size_t)R->n_bow));
  WD_TRY(sc.finish());
  if (feat_off) std::copy(R->feat_off.begin(), R->feat_off.end(), feat_off);
  if (has_words) std::copy(R->has_words.begin(), R->has_words.end(), has_words);
  if (image_max_id) std::copy(R->image_max.begin(), R->image_max.end(), image_max_id);
  if (bow_off) std::copy(R->bow_off.begin(), R->bow_off.end(), bow_off);
  return MSFM_OK;
}

MSFM_API void msfm_word_result_destroy(msfm_word_result* R) { msfm_child_destroy(R); }

MSFM_API int msfm_wordset_create_from_words(msfm_descset* set, const msfm_word_result* R, int max_hypotheses, msfm_wordset** out) {
  const char* who = "msfm_wordset_create_from_words";
  if (!set) return MSFM_E_INVAL;
  DescView V;
  descset_view(set, &V);
  msfm_ctx* ctx = V.ctx;
  if (!R || !out) return msfm_set_error(ctx, MSFM_E_INVAL, "%s: null argument", who);
  *out = nullptr;
  if (R->set != set || R->generation != V.generation)
    return msfm_set_error(ctx, MSFM_E_INVAL, "%s: the words were computed before the set's last descriptor upload (or from another set)", who);
  const int n = R->n;
  std::vector<int> n_features(n);
  for (int i = 0; i < n; i++) n_features[i] = R->feat_off[i + 1] - R->feat_off[i];
  int K = 0;
  long total_l = 0;
  const std::string bad = pairsel_check_counts(n, n_features.data(), R->num_words, max_hypotheses, &K, &total_l);
  if (!bad.empty()) return msfm_set_error(ctx, MSFM_E_INVAL, "%s: %s", who, bad.c_str());
  if (R->n_unassigned > 0)
    return msfm_set_error(ctx, MSFM_E_INVAL, "%s: %lld features of images with words have no word (the reference would index its inverted file at -1)",
                          who, (long long)R->n_unassigned);
  for (int i = 0; i < n; i++)
    if (R->has_words[i] && !V.kp[i])
      return msfm_set_error(ctx, MSFM_E_INVAL, "%s: image %d has words but no keypoints (msfm_descset_upload_keypoints)", who, i);
  const size_t total = (size_t)total_l;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  DevBuf<int> d_feat_off;
  DevBuf<float> d_kp;
  DevScope sc(ctx);
  WD_TRY(sc.up(d_feat_off, R->feat_off));
  WD_TRY(d_kp.alloc(std::max<size_t>(1, 2 * total)));
  for (int i = 0; i < n; i++) {   // an image without keypoints has no words: its rows are never read, and are zero
    if (!n_features[i]) continue;
    float* dst = d_kp.p + 2 * (size_t)R->feat_off[i];
    const size_t bytes = sizeof(float) * 2 * (size_t)n_features[i];
    if (V.kp[i]) WD_TRY(hipMemcpyAsync(dst, V.kp[i], bytes, hipMemcpyDeviceToDevice, s));
    else WD_TRY(hipMemsetAsync(dst, 0, bytes, s));
  }
  MSFM_TRY(wordset_create_dev(ctx, n, K, R->num_words, R->feat_off, d_feat_off, R->d_hw.p, R->d_word.p, d_kp, sc.h2d, out));
  sc.dismiss();   // behind the core's finish()
  return MSFM_OK;
}
