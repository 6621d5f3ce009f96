// The argument checks of words.hip that need no device: plain C++, so a host-only program (tests/words_host_check.cc, built
// with sanitizers there) compiles exactly the code the library runs.  Every function returns an empty string or the refusal's
// text.
#pragma once
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#define WORDS_DIM 128          // floats of a descriptor
#define WORDS_MAX_K 64
#define WORDS_MAX_DEPTH 32     // blocks on a path from block 0
#define WORDS_LEAF 0x80000000u // msb of id_or_childblock (fbow.h:129-137)

static inline std::string words_fmt(const char* fmt, long a = 0, long b = 0, long c = 0) {
  char buf[256];
  snprintf(buf, sizeof buf, fmt, a, b, c);
  return buf;
}

// msfm_voctree_create: the tree is walked from block 0, as Vocabulary::_transform can (fbow.h:417-452).  A non-leaf link to
// block 0 ends the reference's loop and is legal; every other block may be linked once (a second link, or a link back up, is a
// cycle or a shared subtree: the reference would loop for ever on the first).  Blocks that no link reaches are not looked at
// beyond their node count.  *depth = blocks on the longest path, *n_leaves = leaf nodes of the reached blocks.
static inline std::string words_check_tree(int k, int n_blocks, const uint16_t* block_n, const float* node_desc, const uint32_t* node_link,
                                           const float* node_weight, int* depth, int64_t* n_leaves) {
  if (k < 2 || k > WORDS_MAX_K) return words_fmt("k = %ld outside [2, %ld]", k, WORDS_MAX_K);
  if (n_blocks < 1) return words_fmt("n_blocks = %ld: at least block 0", n_blocks);
  if (!block_n || !node_desc || !node_link || !node_weight) return "null argument";
  if ((int64_t)n_blocks * k > 0x7fffffffL) return "more than 2^31 nodes";
  for (int b = 0; b < n_blocks; b++)
    if (block_n[b] > k) return words_fmt("block %ld holds %ld nodes, more than k = %ld", b, block_n[b], k);
  std::vector<int> level(n_blocks, 0);   // 0: not reached
  std::vector<int> queue;
  queue.reserve(n_blocks);
  queue.push_back(0);
  level[0] = 1;
  int deepest = 1;
  int64_t leaves = 0;
  for (size_t q = 0; q < queue.size(); q++) {
    const int b = queue[q];
    if (block_n[b] == 0) return words_fmt("block %ld is reached and holds no node", b);
    for (int i = 0; i < block_n[b]; i++) {
      const uint32_t link = node_link[(size_t)b * k + i];
      if (link & WORDS_LEAF) { leaves++; continue; }
      if (link == 0) continue;   // ends the descent without a word
      if (link >= (uint32_t)n_blocks) return words_fmt("node %ld of block %ld links block %ld, outside the tree", i, b, (long)link);
      if (level[link]) return words_fmt("block %ld is reached twice (again from block %ld)", (long)link, b);
      if (level[b] + 1 > WORDS_MAX_DEPTH) return words_fmt("block %ld lies deeper than %ld blocks", (long)link, WORDS_MAX_DEPTH);
      level[link] = level[b] + 1;
      if (level[link] > deepest) deepest = level[link];
      queue.push_back((int)link);
    }
  }
  *depth = deepest;
  *n_leaves = leaves;
  return "";
}
