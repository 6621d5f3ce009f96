// Driver for tests/test_gpu_seed_host.py and scripts/seed_bench.py.  Reads an image set from argv[1]: int32 n_images,
// n_features[n_images], n_pairs, pair_img[n_pairs][2], match_off[n_pairs+1], matches[M][2], image_model[n_images], seed_chunk,
// then double image_focal[n_images] and float keypoints[sum of n_features][2].  Runs the host mirror's
// IncrementalSfM::FindSeedPairThenReconstruct (one msfm_seed_hypotheses call per chunk; host/objectsfm.cc, reference
// sfm_incremental.cc:224-415) and its one-at-a-time walk FindSeedPairThenReconstructHost, both stopped behind the gates, and
// requires them to agree: same pair, same number of visited hypotheses, same cameras bit for bit, the same points with X and
// mse to 1e-9 (the walk triangulates through msfm_triangulate_midpoint_batch, which is compiled with fused multiply-adds).
// A third run with the adjustment checks FullBundleAdjustment / RemovePointOutliers and the bookkeeping of :401-408.
// Writes to argv[2]: int32 found, id_img1, id_img2, n_visited, n_points, n_models, global feature ids [n_points][2]; double
// f[n_models], R[9], t[3], c[3], X[n_points][3], mse[n_points] - of the batched run.
// argv[3] = "time": prints the milliseconds of the batched search and of the walk (median of 5 each, no adjustment).
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <string>
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

struct Input {
  std::vector<int> n_features, pair_img, match_off, matches, image_model;
  std::vector<double> image_focal;
  std::vector<float> keypoints;
  int seed_chunk = 64;
};

static void setup(IncrementalSfM& s, const Input& in, bool adjust) {
  s.SetMatches(in.n_features, in.pair_img, in.match_off, in.matches);
  s.SetKeypoints(in.keypoints);
  s.image_focal_ = in.image_focal;
  s.image_model_ = in.image_model;
  s.seed_chunk_ = in.seed_chunk;
  s.seed_adjust_ = adjust;
  s.found_seed_ = false;
  s.bundle_full_options_.minimizer_progress_to_stdout = false;
}

static int fail(const char* what) {
  std::printf("seed_host_check FAILED: %s\n", what);
  return 1;
}

int main(int argc, char** argv) {
  if (argc < 3) return 2;
  FILE* f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  Input in;
  std::vector<int> one;
  if (!read_ints(f, one, 1)) return 2;
  const int n_images = one[0];
  if (!read_ints(f, in.n_features, n_images) || !read_ints(f, one, 1)) return 2;
  const int n_pairs = one[0];
  if (!read_ints(f, in.pair_img, 2 * (size_t)n_pairs) || !read_ints(f, in.match_off, (size_t)n_pairs + 1)) return 2;
  if (!read_ints(f, in.matches, 2 * (size_t)in.match_off[n_pairs]) || !read_ints(f, in.image_model, n_images) || !read_ints(f, one, 1)) return 2;
  in.seed_chunk = one[0];
  in.image_focal.resize(n_images);
  if (std::fread(in.image_focal.data(), 8, n_images, f) != (size_t)n_images) return 2;
  size_t rows = 0;
  for (int v : in.n_features) rows += v;
  in.keypoints.resize(2 * rows);
  if (rows && std::fread(in.keypoints.data(), 4, 2 * rows, f) != 2 * rows) return 2;
  std::fclose(f);

  IncrementalSfM dev, host, full;
  setup(dev, in, false); setup(host, in, false); setup(full, in, true);
  const bool found = dev.FindSeedPairThenReconstruct();
  const bool found_h = host.FindSeedPairThenReconstructHost();
  if (found != found_h) return fail("one of the two found a seed pair, the other did not");
  if (dev.seed_hyps_visited_ != host.seed_hyps_visited_) return fail("visited hypotheses");
  if (found) {
    if (dev.cams_.size() != 2 || host.cams_.size() != 2) return fail("two cameras");
    if (dev.cam_models_.size() != host.cam_models_.size() || dev.pts_.size() != host.pts_.size()) return fail("model or point count");
    for (int k = 0; k < 2; k++) {
      if (dev.cams_[k]->id_img_ != host.cams_[k]->id_img_) return fail("images");
      if (dev.cams_[k]->cam_model_->f_ != host.cams_[k]->cam_model_->f_) return fail("focal length");
      for (int q = 0; q < 9; q++) if (dev.cams_[k]->pos_rt_.R.m[q] != host.cams_[k]->pos_rt_.R.m[q]) return fail("R");
      for (int q = 0; q < 3; q++)
        if (dev.cams_[k]->pos_rt_.t[q] != host.cams_[k]->pos_rt_.t[q] || dev.cams_[k]->pos_ac_.c[q] != host.cams_[k]->pos_ac_.c[q]) return fail("t or c");
      if (dev.cams_[k]->pts_.size() != dev.pts_.size()) return fail("camera points");
    }
    for (size_t i = 0; i < dev.pts_.size(); i++) {
      const Point3D *a = dev.pts_[i], *b = host.pts_[i];
      if (a->cams_.begin()->first != b->cams_.begin()->first || a->cams_.rbegin()->first != b->cams_.rbegin()->first) return fail("observations");
      for (int q = 0; q < 3; q++)
        if (std::fabs(a->data[q] - b->data[q]) > 1e-9 + 1e-9 * std::fabs(b->data[q])) return fail("X beyond 1e-9");
      if (std::fabs(a->mse_ - b->mse_) > 1e-9 + 1e-7 * std::fabs(b->mse_)) return fail("mse");
    }
    if (!dev.is_img_processed_[dev.cams_[0]->id_img_] || !dev.is_img_processed_[dev.cams_[1]->id_img_]) return fail("is_img_processed_");
    if (dev.img_cam_map_.size() != 2 || dev.cams_[0]->visible_cams_ != std::vector<int>({0, 1}) || dev.cams_[1]->visible_cams_ != std::vector<int>({1, 0}))
      return fail("bookkeeping of :401-408");
    // with the adjustment: the cost does not rise, no point is left marked as new
    if (!full.FindSeedPairThenReconstruct()) return fail("the run with the adjustment found no pair");
    if (full.cams_[0]->id_img_ != dev.cams_[0]->id_img_ || full.pts_.size() != dev.pts_.size()) return fail("the run with the adjustment differs");
    if (!(full.summary_.final_cost <= full.summary_.initial_cost)) return fail("FullBundleAdjustment raised the cost");
    for (Point3D* p : full.pts_) if (p->is_new_added_) return fail("RemovePointOutliers did not run");
    std::printf("adjusted: %d iterations, cost %.6e -> %.6e\n", full.summary_.num_iterations, full.summary_.initial_cost, full.summary_.final_cost);
  }

  FILE* out = std::fopen(argv[2], "wb");
  if (!out) return 2;
  const int n_points = (int)dev.pts_.size(), n_models = (int)dev.cam_models_.size();
  const int head[6] = {found ? 1 : 0, found ? dev.cams_[0]->id_img_ : -1, found ? dev.cams_[1]->id_img_ : -1, dev.seed_hyps_visited_, n_points, n_models};
  std::fwrite(head, 4, 6, out);
  for (Point3D* p : dev.pts_) { const int g[2] = {p->cams_.begin()->first, p->cams_.rbegin()->first}; std::fwrite(g, 4, 2, out); }
  for (CameraModel* m : dev.cam_models_) std::fwrite(&m->f_, 8, 1, out);
  if (found) {
    std::fwrite(dev.cams_[1]->pos_rt_.R.m, 8, 9, out);
    for (int q = 0; q < 3; q++) std::fwrite(&dev.cams_[1]->pos_rt_.t[q], 8, 1, out);
    for (int q = 0; q < 3; q++) std::fwrite(&dev.cams_[1]->pos_ac_.c[q], 8, 1, out);
  }
  for (Point3D* p : dev.pts_) std::fwrite(p->data, 8, 3, out);
  for (Point3D* p : dev.pts_) std::fwrite(&p->mse_, 8, 1, out);
  std::fclose(out);

  if (argc > 3 && std::string(argv[3]) == "time") {
    std::vector<double> td, th;
    for (int rep = 0; rep < 6; rep++) {   // (the first repetition warms up)
      IncrementalSfM a, b;
      setup(a, in, false); setup(b, in, false);
      double t0 = now_ms();
      a.FindSeedPairThenReconstruct();
      double t1 = now_ms();
      b.FindSeedPairThenReconstructHost();
      double t2 = now_ms();
      if (rep) { td.push_back(t1 - t0); th.push_back(t2 - t1); }
    }
    std::sort(td.begin(), td.end()); std::sort(th.begin(), th.end());
    std::printf("time_ms batched %.3f walk %.3f visited %d\n", td[td.size() / 2], th[th.size() / 2], dev.seed_hyps_visited_);
  }
  std::printf("seed_host_check ok: found %d, pair (%d, %d), %d visited, %d points\n", head[0], head[1], head[2], head[3], head[4]);
  return 0;
}
