// The argument checks of pairsel.hip that need no device: plain C++, so a host-only program (tests/pairselect_host_check.cc,
// built with sanitizers there) compiles exactly the code the library runs.  Every function returns an empty string or the
// refusal's text.
#pragma once
#include <cstdint>
#include <cstdio>
#include <string>

#include "../../include/msfm.h"

// th_num_match of InitialMatchingGraph::match_graph_feature (initial_matching_graph.cc:168-169)
static inline int pairsel_rule_k(int n_images) {
  int k = n_images / 10 > 200 ? n_images / 10 : 200;
  if (k > n_images - 1) k = n_images - 1;
  if (k > 500) k = 500;
  return k;
}

#define PAIRSEL_MAX_IMAGES 46340   // n * n similarity entries are indexed with int

static inline std::string pairsel_fmt(const char* fmt, long a = 0, long b = 0, long c = 0) {
  char buf[256];
  snprintf(buf, sizeof buf, fmt, a, b, c);
  return buf;
}

// What msfm_wordset_create and msfm_wordset_create_from_words (whose word ids never visit the host) check alike: the counts.
// *K = hypotheses per image, *total = features of all images
static inline std::string pairsel_check_counts(int n_images, const int* n_features, int num_words, int max_hypotheses, int* K, long* total) {
  if (n_images < 2) return pairsel_fmt("n_images = %ld: at least 2 images", n_images);
  if (n_images > PAIRSEL_MAX_IMAGES) return pairsel_fmt("n_images = %ld above %ld", n_images, PAIRSEL_MAX_IMAGES);
  if (!n_features) return "null argument";
  if (num_words < 0) return pairsel_fmt("num_words = %ld is negative", num_words);
  if (max_hypotheses < 0 || max_hypotheses > n_images - 1)
    return pairsel_fmt("max_hypotheses = %ld outside [0, n_images - 1 = %ld]", max_hypotheses, n_images - 1);
  long t = 0;
  for (int i = 0; i < n_images; i++) {
    if (n_features[i] < 0) return pairsel_fmt("image %ld has a negative feature count", i);
    t += n_features[i];
    if (t > 0x7fffffffL) return "more than 2^31 features";
  }
  *K = max_hypotheses > 0 ? max_hypotheses : pairsel_rule_k(n_images);
  *total = t;
  return "";
}

// msfm_wordset_create: the counts, and every word id of an image with words
static inline std::string pairsel_check_create(int n_images, const int* n_features, const uint8_t* has_words, const int32_t* word_id, int num_words,
                                               const float* keypoints, int max_hypotheses, int* K, long* total) {
  if (n_images >= 2 && n_images <= PAIRSEL_MAX_IMAGES && (!n_features || !has_words)) return "null argument";
  long t = 0;
  const std::string bad = pairsel_check_counts(n_images, n_features, num_words, max_hypotheses, K, &t);
  if (!bad.empty()) return bad;
  if (t > 0 && (!word_id || !keypoints)) return "null argument";
  t = 0;
  for (int i = 0; i < n_images; i++) {
    if (has_words[i])
      for (int f = 0; f < n_features[i]; f++) {
        const int w = word_id[t + f];
        if (w < 0 || w > num_words) return pairsel_fmt("word id %ld of image %ld outside [0, num_words = %ld]", w, i, num_words);
      }
    t += n_features[i];
  }
  *K = max_hypotheses > 0 ? max_hypotheses : pairsel_rule_k(n_images);
  *total = t;
  return "";
}

// msfm_pair_select: *Ks = slots per row of this call
static inline std::string pairsel_check_select(int n_images, int K, int first_image, int n_rows, const msfm_pair_select_options* opt, int* Ks) {
  if (first_image < 0 || n_rows < 1 || first_image > n_images - n_rows)
    return pairsel_fmt("rows [%ld, %ld) outside the set's %ld images", first_image, (long)first_image + n_rows, n_images);
  if (opt->max_hypotheses < 0 || opt->max_hypotheses > K)
    return pairsel_fmt("max_hypotheses = %ld outside [0, %ld], the hypotheses the set ranked", opt->max_hypotheses, K);
  if (opt->th_init_matches < 0 || opt->th_inliers < 0) return "a threshold is negative";
  if (opt->fransac.max_iterations < 1 || opt->fransac.max_iterations > 65536 || !(opt->fransac.threshold > 0.0)) return "bad fransac options";
  *Ks = opt->max_hypotheses > 0 ? opt->max_hypotheses : K;
  if ((long)n_rows * *Ks > 0x7ffffffeL) return "more than 2^31 hypotheses in one call";
  return "";
}
