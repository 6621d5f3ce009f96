// SLAMGPS::FeatureMatching step 1 from a binary SLAM point file, written as feature/prior.txt
// (slam_gps.cc:323-423 through msfm_slam_priors, then WriteOutPriorInfo :1821-1847).
//   test_slam_priors <points.bin> <prior.txt> [resize_ratio]
// resize_ratio (default 0.5, as SLAMGPS::SLAMGPS sets it, slam_gps.cc:55) scales the thresholds: 2.0 / r and 5.0 / r px.
// points.bin (little endian): int32 n_cams, int32 n_points, then per point int32 n_obs and n_obs records
// {int32 camera index, float64 x, float64 y} (centred pixels, as Point3D::pts2d_).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>

#include "objectsfm.h"

using namespace objectsfm;

int main(int argc, char** argv) {
  if (argc != 3 && argc != 4) {
    std::fprintf(stderr, "usage: %s <points.bin> <prior.txt> [resize_ratio]\n", argv[0]);
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
  int32_t n_cams = 0, n_points = 0;
  in.read(reinterpret_cast<char*>(&n_cams), 4);
  in.read(reinterpret_cast<char*>(&n_points), 4);
  if (!in || n_cams < 0 || n_points < 0) {
    std::fprintf(stderr, "cannot read %s\n", argv[1]);
    return 1;
  }
  std::vector<Camera> cams(n_cams);
  std::vector<Point3D> pts(n_points);
  SLAMGPS slam;
  slam.resize_ratio = resize_ratio;
  for (int c = 0; c < n_cams; c++) {
    cams[c].SetID(c);
    slam.cams_.push_back(&cams[c]);
  }
  for (int p = 0; p < n_points; p++) {
    int32_t n = 0;
    in.read(reinterpret_cast<char*>(&n), 4);
    for (int k = 0; k < n; k++) {
      char rec[20];
      in.read(rec, 20);
      int32_t c;
      double x, y;
      std::memcpy(&c, rec, 4);
      std::memcpy(&x, rec + 4, 8);
      std::memcpy(&y, rec + 12, 8);
      if (c < 0 || c >= n_cams) {
        std::fprintf(stderr, "point %d: camera %d out of range\n", p, c);
        return 1;
      }
      pts[p].AddObservation(&cams[c], x, y, c);
    }
    pts[p].id_ = p;
    slam.pts_.push_back(&pts[p]);
  }
  if (!in) {
    std::fprintf(stderr, "truncated %s\n", argv[1]);
    return 1;
  }
  std::vector<std::vector<int>> ids;
  std::vector<std::vector<Mat3>> Fs, Hs;
  slam.FeatureMatchingPriors(ids, Fs, Hs);
  SLAMGPS::WriteOutPriorInfo(argv[2], ids, Fs, Hs);
  size_t kept = 0;
  for (auto& v : ids) kept += v.size();
  std::printf("%d cameras, %d points: %zu pairs kept\n", n_cams, n_points, kept);
  return 0;
}
