// The argument checks of msfm_voctree_create (metricsfm_amd/csrc/words_args.h, the code the library refuses with) on bad and
// good trees.  Needs neither the library nor a device; tests/test_words_abi.py builds it with the host sanitizers.
#include <cstdio>
#include <vector>

#include "../metricsfm_amd/csrc/words_args.h"

static int fail(const char* what) {
  std::printf("words_host_check FAILED: %s\n", what);
  return 1;
}

int main() {
  const int k = 3, nb = 4;
  const uint32_t L = WORDS_LEAF;
  // block 0: a leaf, block 1, block 2; block 1: two leaves; block 2: block 3, a link to block 0; block 3: one leaf
  std::vector<uint16_t> n = {3, 2, 2, 1};
  std::vector<uint32_t> link = {L | 5, 1, 2, L | 6, L | 7, 0, 3, 0, 0, L | 9, 0, 0};
  std::vector<float> desc((size_t)nb * k * WORDS_DIM, 1.0f), w((size_t)nb * k, 0.5f);
  int depth = -1;
  int64_t leaves = -1;
  auto check = [&](int kk, int blocks) { return words_check_tree(kk, blocks, n.data(), desc.data(), link.data(), w.data(), &depth, &leaves); };
  if (!check(k, nb).empty() || depth != 3 || leaves != 4) return fail("a good tree is refused, or its depth and leaves are wrong");
  if (check(1, nb).empty() || check(65, nb).empty() || check(k, 0).empty()) return fail("k or n_blocks out of range accepted");
  if (words_check_tree(k, nb, nullptr, desc.data(), link.data(), w.data(), &depth, &leaves).empty() ||
      words_check_tree(k, nb, n.data(), nullptr, link.data(), w.data(), &depth, &leaves).empty() ||
      words_check_tree(k, nb, n.data(), desc.data(), nullptr, w.data(), &depth, &leaves).empty() ||
      words_check_tree(k, nb, n.data(), desc.data(), link.data(), nullptr, &depth, &leaves).empty())
    return fail("a null array accepted");
  n[1] = 4;
  if (check(k, nb).empty()) return fail("block_n above k accepted");
  n[1] = 0;
  if (check(k, nb).empty()) return fail("a reached block without nodes accepted");
  n[1] = 2;
  link[2] = 4;
  if (check(k, nb).empty()) return fail("a child block outside the tree accepted");
  link[2] = 1;
  if (check(k, nb).empty()) return fail("a block reached twice accepted");
  link[2] = 2;
  link[9] = 2;   // block 3 links back to block 2
  if (check(k, nb).empty()) return fail("a cycle accepted");
  link[9] = L | 9;
  n[3] = 0;      // block 3 is linked from block 2: reached
  if (check(k, nb).empty()) return fail("an empty leaf block accepted");
  link[6] = L | 1;   // no longer linked: an unreached block may be empty
  if (!check(k, nb).empty() || depth != 2) return fail("an unreached empty block refused");
  // a chain: block b's node 0 links block b + 1
  for (int len : {WORDS_MAX_DEPTH, WORDS_MAX_DEPTH + 1}) {
    std::vector<uint16_t> cn(len, 1);
    std::vector<uint32_t> cl((size_t)len * 2, 0);
    for (int b = 0; b < len; b++) cl[(size_t)b * 2] = b + 1 < len ? (uint32_t)(b + 1) : (L | 1);
    std::vector<float> cd((size_t)len * 2 * WORDS_DIM, 0.f), cw((size_t)len * 2, 1.f);
    const bool ok = words_check_tree(2, len, cn.data(), cd.data(), cl.data(), cw.data(), &depth, &leaves).empty();
    if (ok != (len == WORDS_MAX_DEPTH)) return fail("the depth limit");
    if (ok && (depth != WORDS_MAX_DEPTH || leaves != 1)) return fail("the chain's depth");
  }
  std::printf("words_host_check ok\n");
  return 0;
}
