// What msfm_descset_voctree_train decides without a device: the option and sample checks, the two fixed-point shifts and the
// counter-based draw of the seeding (include/msfm.h states all of them).  Plain C++, so a host-only program
// (tests/voctrain_host_check.cc, built with sanitizers there) compiles exactly the code the library runs; voctrain.hip defines
// VOCTRAIN_HD so that the draw is also a device function.  Every check returns an empty string or the refusal's text.
#pragma once
#include <cstring>

#include "words_args.h"

#ifndef VOCTRAIN_HD
#define VOCTRAIN_HD
#endif

#define VOCTRAIN_MAX_FEATURES (1L << 23)
#define VOCTRAIN_MAX_LEVELS 32          // = WORDS_MAX_DEPTH, the length of the per-level arrays of msfm_voctree_train_stats
#define VOCTRAIN_VALUE_BOUND 2896.0f    // |value| below it: 128 (2 * 2896)^2 < 2^32, the descent's starting `best`
#define VOCTRAIN_SALT 0x766F637472616E31ull

struct voctrain_options {   // the arguments of msfm_descset_voctree_train
  int k, levels, max_iters, image_step;
  uint64_t seed;
};

static inline void voctrain_defaults(voctrain_options* o) {   // the reference's values (fbow's Params; database.cc:658, :673)
  o->k = 10; o->levels = 6; o->max_iters = 11; o->image_step = 1; o->seed = 0;
}

static inline std::string voctrain_check_options(const voctrain_options* o) {
  if (!o) return "null argument";
  if (o->k < 2 || o->k > WORDS_MAX_K) return words_fmt("k = %ld outside [2, %ld]", o->k, WORDS_MAX_K);
  if (o->levels < 1 || o->levels > VOCTRAIN_MAX_LEVELS) return words_fmt("levels = %ld outside [1, %ld]", o->levels, VOCTRAIN_MAX_LEVELS);
  if (o->max_iters < 1) return words_fmt("max_iters = %ld: at least 1", o->max_iters);
  if (o->image_step < 1) return words_fmt("image_step = %ld: at least 1", o->image_step);
  return "";
}

// the sampled images 0, step, 2 step, ... and the first feature number of each: off has images.size() + 1 entries
static inline std::string voctrain_sample(int n_images, const int* count, int image_step, std::vector<int>* images, std::vector<int>* off) {
  images->clear();
  off->assign(1, 0);
  long total = 0;
  for (int i = 0; i < n_images; i += image_step) {
    if (count[i] < 0) return words_fmt("image %ld has a negative feature count", i);
    total += count[i];
    if (total > VOCTRAIN_MAX_FEATURES) return words_fmt("more than 2^23 sampled features (image %ld brings them to %ld)", i, total);
    images->push_back(i);
    off->push_back((int)total);
  }
  if (total == 0) return "no sampled feature";
  return "";
}

// maxbits: the largest bit pattern of |value| over the sample.  *e = the smallest integer with maxabs < 2^e as the exponent
// field gives it; weight_shift = 40 - (9 + 2 e), sum_shift = 39 - e.
static inline std::string voctrain_shifts(uint32_t maxbits, int* weight_shift, int* sum_shift) {
  float bound = VOCTRAIN_VALUE_BOUND;
  uint32_t bound_bits;
  std::memcpy(&bound_bits, &bound, sizeof bound_bits);
  if (maxbits >= 0x7f800000u) return "a sampled value is not finite";
  if (maxbits >= bound_bits) return "a sampled value has |value| >= 2896";
  const int e = (int)(maxbits >> 23) - 126;
  *weight_shift = 40 - (9 + 2 * e);
  *sum_shift = 39 - e;
  return "";
}

VOCTRAIN_HD static inline uint64_t voctrain_next(uint64_t& x) {   // splitmix64: common.h's sm64, restated because this header compiles without HIP
  x += 0x9E3779B97F4A7C15ull;
  uint64_t z = x;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

VOCTRAIN_HD static inline uint64_t voctrain_draw(uint64_t seed, int level, int ordinal, int j) {
  uint64_t x = seed ^ VOCTRAIN_SALT;
  uint64_t h = voctrain_next(x);
  x = h ^ (((uint64_t)level << 40) | (uint64_t)(uint32_t)ordinal);
  h = voctrain_next(x);
  x = h ^ (uint64_t)j;
  return voctrain_next(x);
}
