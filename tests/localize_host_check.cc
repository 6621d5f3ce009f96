// Driver for tests/test_gpu_localize_host.py and scripts/localize_bench.py.  Reads one localisation round from argv[1] (all int32
// unless noted): n_images, n_features[n_images], n_pairs, pair_img[n_pairs][2], match_off[n_pairs+1], matches[M][2], n_cams,
// cam_img[n_cams], feat_point[sum of the registered images' features], n_points, pt_bad[n_points], pt_views[n_points],
// pt_mse[n_points] (double), fail_times[n_images].  Builds the host mirror's cameras and points from it, runs
// IncrementalSfM::FindImageToLocalize (host/objectsfm.cc; reference sfm_incremental.cc:417-563) and the std::map walk
// FindImageToLocalizeHost, requires both to agree and writes the result to argv[2]: n, image_ids[n], then per image n_corr,
// (feature, point)[n_corr], n_visible, visible[n_visible].
// argv[3] = "time": prints the milliseconds of SetMatches, of the library round (median of 9) and of the std::map walk (best of 3).
#include <algorithm>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "objectsfm.h"

using namespace objectsfm;

static bool read_ints(FILE* in, std::vector<int>& v, size_t n) {
  v.resize(n);
  return n == 0 || std::fread(v.data(), 4, n, in) == n;
}

static double now_ms() {
  return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

int main(int argc, char** argv) {
  if (argc < 3) return 2;
  FILE* in = std::fopen(argv[1], "rb");
  if (!in) return 2;
  std::vector<int> one, n_features, pair_img, match_off, matches, cam_img, feat_point, pt_bad, pt_views, fail;
  std::vector<double> pt_mse;
  if (!read_ints(in, one, 1)) return 2;
  const int n_images = one[0];
  if (!read_ints(in, n_features, n_images) || !read_ints(in, one, 1)) return 2;
  const int n_pairs = one[0];
  if (!read_ints(in, pair_img, 2 * (size_t)n_pairs) || !read_ints(in, match_off, (size_t)n_pairs + 1)) return 2;
  if (!read_ints(in, matches, 2 * (size_t)match_off[n_pairs]) || !read_ints(in, one, 1)) return 2;
  const int n_cams = one[0];
  if (!read_ints(in, cam_img, n_cams)) return 2;
  size_t fp = 0;
  for (int c = 0; c < n_cams; c++) fp += n_features[cam_img[c]];
  if (!read_ints(in, feat_point, fp) || !read_ints(in, one, 1)) return 2;
  const int n_points = one[0];
  if (!read_ints(in, pt_bad, n_points) || !read_ints(in, pt_views, n_points)) return 2;
  pt_mse.resize(n_points);
  if (n_points && std::fread(pt_mse.data(), 8, n_points, in) != (size_t)n_points) return 2;
  if (!read_ints(in, fail, n_images)) return 2;
  std::fclose(in);

  // the objects of the reference: a point knows its id, mse, badness and (here only as a count) its cameras
  std::vector<Point3D> pts(n_points);
  std::vector<Camera> cams(n_cams);
  IncrementalSfM sfm;
  for (int i = 0; i < n_points; i++) {
    pts[i].id_ = i; pts[i].mse_ = pt_mse[i]; pts[i].is_bad_estimated_ = pt_bad[i] != 0;
    for (int k = 0; k < pt_views[i]; k++) pts[i].cams_.insert(std::make_pair(k, (Camera*)nullptr));
    sfm.pts_.push_back(&pts[i]);
  }
  const bool timing = argc > 3 && std::strcmp(argv[3], "time") == 0;
  const double t0 = now_ms();
  sfm.SetMatches(n_features, pair_img, match_off, matches);
  const double ms_store = now_ms() - t0;
  size_t at = 0;
  for (int c = 0; c < n_cams; c++) {
    const int img = cam_img[c];
    cams[c].id_img_ = img; cams[c].SetID(c);
    for (int f = 0; f < n_features[img]; f++)
      if (feat_point[at + f] >= 0) cams[c].AddPoints(&pts[feat_point[at + f]], f + sfm.options_.idx_max_per_image * img);
    at += n_features[img];
    sfm.cams_.push_back(&cams[c]);
    sfm.is_img_processed_[img] = true;
    sfm.img_cam_map_[img] = c;
  }
  sfm.localize_fail_times_ = fail;

  std::vector<int> ids, ids_h;
  std::vector<std::vector<std::pair<int, int>>> corres, corres_h;
  std::vector<std::vector<int>> visible, visible_h;
  sfm.FindImageToLocalize(ids, corres, visible);
  sfm.FindImageToLocalizeHost(ids_h, corres_h, visible_h);
  if (ids != ids_h || corres != corres_h || visible != visible_h) { std::printf("FAIL: the library round and the std::map walk differ\n"); return 1; }
  if (timing) {
    std::vector<double> lap;
    for (int r = 0; r < 9; r++) { const double a = now_ms(); sfm.FindImageToLocalize(ids, corres, visible); lap.push_back(now_ms() - a); }
    std::sort(lap.begin(), lap.end());
    double best = 1e300;
    for (int r = 0; r < 3; r++) { const double a = now_ms(); sfm.FindImageToLocalizeHost(ids_h, corres_h, visible_h); best = std::min(best, now_ms() - a); }
    std::printf("timing_ms store %.3f library_round %.3f map_walk %.3f\n", ms_store, lap[4], best);
  }
  FILE* out = std::fopen(argv[2], "wb");
  if (!out) return 2;
  auto put = [&](int v) { std::fwrite(&v, 4, 1, out); };
  put((int)ids.size());
  for (int id : ids) put(id);
  for (size_t i = 0; i < ids.size(); i++) {
    put((int)corres[i].size());
    for (auto& e : corres[i]) { put(e.first); put(e.second); }
    put((int)visible[i].size());
    for (int v : visible[i]) put(v);
  }
  std::fclose(out);
  std::printf("localize_host_check ok: %zu images\n", ids.size());
  return 0;
}
