// SLAMGPS::FeatureMatching step 2 from one binary file, written as the <i>_match files and graph_matching.txt
// (slam_gps.cc:425-555 through msfm_match_pairs_slam + msfm_chain_create + msfm_chain_verify_slam, then WriteOutMatches
// :1776-1801 and WriteOutMatchGraph :1803-1819).
//   test_slam_match <input.bin> <output_fold> [resize_ratio]
// resize_ratio (default 0.5, slam_gps.cc:55) scales the gate thresholds: 2.0 / r and 5.0 / r px.
// input.bin (little endian): int32 n_images, per image int32 n, float32 descriptors [n][128], float32 keypoints [n][2]
// (centred pixels); then int32 n_pairs and per pair {int32 i, int32 j, float64 F[9], float64 H[9]} grouped by i ascending
// (the kept pairs of step 1, what feature/prior.txt holds).  output_fold must exist; the match files are appended to.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>

#include "objectsfm.h"

using namespace objectsfm;

int main(int argc, char** argv) {
  if (argc != 3 && argc != 4) {
    std::fprintf(stderr, "usage: %s <input.bin> <output_fold> [resize_ratio]\n", argv[0]);
    return 2;
  }
  double resize_ratio = 0.5;
  if (argc == 4) {
    char* end = nullptr;
    resize_ratio = std::strtod(argv[3], &end);
    if (!end || *end || !(resize_ratio > 0.0)) {
      std::fprintf(stderr, "bad resize_ratio %s\n", argv[3]);
      return 2;
    }
  }
  std::ifstream in(argv[1], std::ios::binary);
  int32_t n_img = 0;
  in.read(reinterpret_cast<char*>(&n_img), 4);
  if (!in || n_img < 0 || n_img > (1 << 20)) {
    std::fprintf(stderr, "cannot read %s\n", argv[1]);
    return 1;
  }
  std::vector<std::vector<float>> descriptors(n_img);
  std::vector<std::vector<Point2f>> keypoints(n_img);
  for (int i = 0; i < n_img; i++) {
    int32_t n = 0;
    in.read(reinterpret_cast<char*>(&n), 4);
    if (!in || n < 0 || n > (1 << 24)) {
      std::fprintf(stderr, "image %d: bad feature count\n", i);
      return 1;
    }
    descriptors[i].resize(128 * (size_t)n);
    in.read(reinterpret_cast<char*>(descriptors[i].data()), sizeof(float) * descriptors[i].size());
    std::vector<float> xy(2 * (size_t)n);
    in.read(reinterpret_cast<char*>(xy.data()), sizeof(float) * xy.size());
    keypoints[i].resize(n);
    for (int k = 0; k < n; k++) { keypoints[i][k].x = xy[2 * k]; keypoints[i][k].y = xy[2 * k + 1]; }
  }
  int32_t n_pairs = 0;
  in.read(reinterpret_cast<char*>(&n_pairs), 4);
  if (!in || n_pairs < 0) {
    std::fprintf(stderr, "truncated %s\n", argv[1]);
    return 1;
  }
  std::vector<std::vector<int>> ids(n_img);
  std::vector<std::vector<Mat3>> Fs(n_img), Hs(n_img);
  int last = 0;
  for (int p = 0; p < n_pairs; p++) {
    char rec[8 + 144];
    in.read(rec, sizeof rec);
    int32_t i, j;
    Mat3 f, h;
    std::memcpy(&i, rec, 4);
    std::memcpy(&j, rec + 4, 4);
    std::memcpy(f.m, rec + 8, 72);
    std::memcpy(h.m, rec + 80, 72);
    if (!in || i < last || i >= n_img || j < 0 || j >= n_img) {
      std::fprintf(stderr, "pair %d: truncated, out of range or not grouped by the first image\n", p);
      return 1;
    }
    last = i;
    ids[i].push_back(j);
    Fs[i].push_back(f);
    Hs[i].push_back(h);
  }
  SLAMGPS slam;
  slam.resize_ratio = resize_ratio;
  std::vector<std::vector<std::vector<std::pair<int, int>>>> matches;
  std::vector<std::vector<int>> match_graph;
  slam.FeatureMatching(descriptors, keypoints, ids, Fs, Hs, matches, match_graph);
  const std::string fold = argv[2];
  long total = 0;
  for (int i = 0; i < n_img; i++)
    for (size_t j = 0; j < ids[i].size(); j++) {
      WriteOutMatches(fold, i, ids[i][j], matches[i][j]);   // (an empty list writes nothing, :1779-1782)
      total += (long)matches[i][j].size();
    }
  WriteOutMatchGraph(fold, match_graph);
  std::printf("%d images, %d pairs: %ld matches kept\n", n_img, n_pairs, total);
  return 0;
}
