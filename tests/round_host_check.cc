// Driver for tests/test_gpu_round_host.py and scripts/round_bench.py.  Reads a model from argv[1] (tests/round_data.py::write_model):
// int32 n_images, n_features[n_images], n_cams, cam_img[n_cams], feat_point[sum of the cameras' features], n_points, n_obs,
// obs_point / obs_cam / obs_feat[n_obs], n_models, cam_model_of_cam[n_cams], new_cam, n_visible, visible[n_visible],
// pt_bad / pt_mutable / pt_new_added[n_points]; then double cam_pose[n_cams][6], cam_model[n_models][3], point_xyz[n_points][3],
// pt_mse[n_points] and float keypoints[sum of n_features][2].
// Builds the object graph twice and runs the host mirror's IncrementalSfM::AdjustRound (one msfm_round_adjust call;
// host/objectsfm.cc, reference sfm_incremental.cc:172-186) on one copy and its own PartialBundleAdjustment ->
// RemovePointOutliers on the other, and requires: the same accept / reject sequence and iteration count, costs to rtol 1e-11,
// parameters to 1e-9 absolute, the same bad flags.  Both paths hand the solver the same compact problem (the mirror's
// BundleAdjuster::RunOptimizetion drops the rows and points without a residual block too), and the two solves do come out bitwise
// equal - costs, cameras, models, points: that is required as well, behind the tolerances, which then say how far off a failure is.
// Writes to argv[2] what AdjustRound left: double cam_pose, cam_model, point_xyz, pt_mse; int32 pt_bad, pt_mutable, pt_new_added,
// counts[3], adjust[2][2], solved[2].
// argv[3] = "time": prints the milliseconds of AdjustRound and of the object-graph path (median of 9 each after a warm-up).
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "objectsfm.h"

using namespace objectsfm;

static bool read_ints(FILE* in, std::vector<int>& v, size_t n) {
  v.resize(n);
  return n == 0 || std::fread(v.data(), 4, n, in) == n;
}
static bool read_doubles(FILE* in, std::vector<double>& v, size_t n) {
  v.resize(n);
  return n == 0 || std::fread(v.data(), 8, n, in) == n;
}
static double now_ms() {
  return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

struct Input {
  std::vector<int> n_features, cam_img, feat_point, obs_point, obs_cam, obs_feat, model_of_cam, visible, bad, mut, added;
  std::vector<double> pose, model, xyz, mse;
  std::vector<float> keypoints;
  int n_points = 0, new_cam = 0;
};

struct Model {
  IncrementalSfM s;
  std::vector<std::unique_ptr<Camera>> cams;
  std::vector<std::unique_ptr<CameraModel>> models;
  std::vector<std::unique_ptr<Point3D>> pts;
};

// cams_ / cam_models_ / pts_ as a round leaves them in front of its adjustment
static void setup(Model& m, const Input& in) {
  IncrementalSfM& s = m.s;
  std::vector<int> two;
  for (size_t i = 0; i < in.n_features.size() && two.size() < 2; i++) if (in.n_features[i] > 0) two.push_back((int)i);
  s.SetMatches(in.n_features, two, {0, 1}, {0, 0});   // (the call reads n_features of the store, nothing else)
  s.SetKeypoints(in.keypoints);
  s.options_.th_mse_outliers = 1.0;
  s.bundle_partial_options_.max_num_iterations = 100; s.bundle_partial_options_.minimizer_progress_to_stdout = false;
  s.bundle_full_options_ = s.bundle_partial_options_;
  std::vector<size_t> first(in.n_features.size() + 1, 0);
  for (size_t i = 0; i < in.n_features.size(); i++) first[i + 1] = first[i] + in.n_features[i];
  for (size_t k = 0; k < in.model.size() / 3; k++) {
    m.models.emplace_back(new CameraModel);
    CameraModel* cm = m.models.back().get();
    cm->id_ = (int)k; cm->f_ = in.model[3 * k]; cm->k1_ = in.model[3 * k + 1]; cm->k2_ = in.model[3 * k + 2];
    cm->UpdateDataFromModel();
    s.cam_models_.push_back(cm);
  }
  for (int i = 0; i < in.n_points; i++) {
    m.pts.emplace_back(new Point3D);
    Point3D* p = m.pts.back().get();
    p->id_ = i;
    for (int q = 0; q < 3; q++) p->data[q] = in.xyz[3 * (size_t)i + q];
    p->mse_ = in.mse[i]; p->is_bad_estimated_ = in.bad[i] != 0; p->is_mutable_ = in.mut[i] != 0; p->is_new_added_ = in.added[i] != 0;
    s.pts_.push_back(p);
  }
  size_t at = 0;
  for (size_t k = 0; k < in.cam_img.size(); k++) {
    m.cams.emplace_back(new Camera);
    Camera* cam = m.cams.back().get();
    cam->SetID((int)k);
    cam->AssociateImage(in.cam_img[k]);
    cam->AssociateCamereModel(s.cam_models_[in.model_of_cam[k]]);
    s.cam_models_[in.model_of_cam[k]]->AddCamera((int)k);
    for (int q = 0; q < 6; q++) cam->data[q] = in.pose[6 * k + q];
    cam->UpdatePoseFromData();
    const int img = in.cam_img[k], nf = in.n_features[img];
    for (int f = 0; f < nf; f++)
      if (in.feat_point[at + f] >= 0) cam->AddPoints(s.pts_[in.feat_point[at + f]], f + img * s.options_.idx_max_per_image);
    at += nf;
    s.cams_.push_back(cam);
    s.img_cam_map_[img] = (int)k;
    s.is_img_processed_[img] = true;
  }
  for (size_t r = 0; r < in.obs_point.size(); r++) {   // Point3D::AddObservation in row order
    Camera* cam = s.cams_[in.obs_cam[r]];
    const size_t row = first[cam->id_img_] + in.obs_feat[r];
    s.pts_[in.obs_point[r]]->AddObservation(cam, in.keypoints[2 * row], in.keypoints[2 * row + 1],
                                            in.obs_feat[r] + cam->id_img_ * s.options_.idx_max_per_image);
  }
  s.cams_[in.new_cam]->visible_cams_ = in.visible;
}

static int fail(const char* what) {
  std::printf("round_host_check FAILED: %s\n", what);
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
  const int n_cams = one[0];
  if (n_cams < 1 || !read_ints(f, in.cam_img, n_cams)) return 2;
  size_t fp = 0, rows = 0;
  for (int img : in.cam_img) fp += in.n_features[img];
  for (int v : in.n_features) rows += v;
  if (!read_ints(f, in.feat_point, fp) || !read_ints(f, one, 2)) return 2;
  in.n_points = one[0];
  const int n_obs = one[1];
  if (!read_ints(f, in.obs_point, n_obs) || !read_ints(f, in.obs_cam, n_obs) || !read_ints(f, in.obs_feat, n_obs) || !read_ints(f, one, 1)) return 2;
  const int n_models = one[0];
  if (!read_ints(f, in.model_of_cam, n_cams) || !read_ints(f, one, 2)) return 2;
  in.new_cam = one[0];
  if (!read_ints(f, in.visible, one[1])) return 2;
  const size_t np = (size_t)in.n_points;
  if (!read_ints(f, in.bad, np) || !read_ints(f, in.mut, np) || !read_ints(f, in.added, np)) return 2;
  if (!read_doubles(f, in.pose, 6 * (size_t)n_cams) || !read_doubles(f, in.model, 3 * (size_t)n_models) || !read_doubles(f, in.xyz, 3 * np) ||
      !read_doubles(f, in.mse, np))
    return 2;
  in.keypoints.resize(2 * rows);
  if (rows && std::fread(in.keypoints.data(), 4, 2 * rows, f) != 2 * rows) return 2;
  std::fclose(f);

  Model dev, obj;
  setup(dev, in); setup(obj, in);
  dev.s.AdjustRound(in.new_cam, false);
  obj.s.PartialBundleAdjustment(in.new_cam);
  const msfm_ba_summary so = obj.s.summary_;
  const std::vector<msfm_ba_iteration> io = obj.s.iterations_;
  obj.s.RemovePointOutliers();
  const msfm_ba_summary& sd = dev.s.round_summary_[0];
  if (!dev.s.round_solved_[0]) return fail("the partial stage did not solve");
  if (sd.num_iterations != so.num_iterations || sd.termination != so.termination) return fail("iteration count / termination");
  bool bitwise = sd.initial_cost == so.initial_cost && sd.final_cost == so.final_cost;
  for (int k = 0; k <= sd.num_iterations; k++) {
    const msfm_ba_iteration &a = dev.s.round_iterations_[0][k], &b = io[k];
    if (a.step_is_successful != b.step_is_successful || a.step_is_valid != b.step_is_valid) return fail("accept / reject sequence");
    if (std::fabs(a.cost - b.cost) > 1e-11 * std::fabs(b.cost)) return fail("cost beyond rtol 1e-11");
    bitwise = bitwise && a.cost == b.cost;
  }
  double worst = 0;
  for (size_t k = 0; k < dev.s.cams_.size(); k++) {
    for (int q = 0; q < 6; q++) worst = std::max(worst, std::fabs(dev.s.cams_[k]->data[q] - obj.s.cams_[k]->data[q]));
    for (int q = 0; q < 9; q++) worst = std::max(worst, std::fabs(dev.s.cams_[k]->pos_rt_.R.m[q] - obj.s.cams_[k]->pos_rt_.R.m[q]));
    for (int q = 0; q < 3; q++) worst = std::max(worst, std::fabs(dev.s.cams_[k]->pos_ac_.c[q] - obj.s.cams_[k]->pos_ac_.c[q]));
    if (dev.s.cams_[k]->is_mutable_ != obj.s.cams_[k]->is_mutable_) return fail("camera is_mutable_");
  }
  for (size_t k = 0; k < dev.s.cam_models_.size(); k++)
    for (int q = 0; q < 3; q++) worst = std::max(worst, std::fabs(dev.s.cam_models_[k]->data[q] - obj.s.cam_models_[k]->data[q]));
  int n_bad = 0;
  for (size_t i = 0; i < np; i++) {
    const Point3D *a = dev.s.pts_[i], *b = obj.s.pts_[i];
    for (int q = 0; q < 3; q++) worst = std::max(worst, std::fabs(a->data[q] - b->data[q]));
    if (a->is_bad_estimated_ != b->is_bad_estimated_) return fail("bad flags");
    if (a->is_mutable_ != b->is_mutable_) return fail("point is_mutable_");
    if (a->is_new_added_ != b->is_new_added_) return fail("is_new_added_");
    n_bad += a->is_bad_estimated_ ? 1 : 0;
  }
  if (!(worst <= 1e-9)) return fail("parameters beyond 1e-9");
  bitwise = bitwise && worst == 0.0;
  if (!bitwise) return fail("inside the tolerances, but the solve is not bitwise equal to the object-graph path");

  FILE* out = std::fopen(argv[2], "wb");
  if (!out) return 2;
  for (Camera* c : dev.s.cams_) std::fwrite(c->data, 8, 6, out);
  for (CameraModel* c : dev.s.cam_models_) std::fwrite(c->data, 8, 3, out);
  for (Point3D* p : dev.s.pts_) std::fwrite(p->data, 8, 3, out);
  for (Point3D* p : dev.s.pts_) std::fwrite(&p->mse_, 8, 1, out);
  std::vector<int> flags;
  for (Point3D* p : dev.s.pts_) flags.push_back(p->is_bad_estimated_);
  for (Point3D* p : dev.s.pts_) flags.push_back(p->is_mutable_);
  for (Point3D* p : dev.s.pts_) flags.push_back(p->is_new_added_);
  flags.insert(flags.end(), dev.s.round_counts_, dev.s.round_counts_ + 3);
  flags.insert(flags.end(), &dev.s.round_adjust_[0][0], &dev.s.round_adjust_[0][0] + 4);
  flags.insert(flags.end(), dev.s.round_solved_, dev.s.round_solved_ + 2);
  std::fwrite(flags.data(), 4, flags.size(), out);
  std::fclose(out);

  if (argc > 3 && std::string(argv[3]) == "time") {
    std::vector<double> td, to;
    for (int rep = 0; rep < 10; rep++) {   // (the first repetition warms up)
      Model a, b;
      setup(a, in); setup(b, in);
      const double t0 = now_ms();
      a.s.AdjustRound(in.new_cam, false);
      const double t1 = now_ms();
      b.s.PartialBundleAdjustment(in.new_cam);
      b.s.RemovePointOutliers();
      const double t2 = now_ms();
      if (rep) { td.push_back(t1 - t0); to.push_back(t2 - t1); }
    }
    std::sort(td.begin(), td.end()); std::sort(to.begin(), to.end());
    std::printf("time_ms adjust_round %.3f object_graph %.3f\n", td[td.size() / 2], to[to.size() / 2]);
  }
  std::printf("round_host_check ok: %d iterations, %d bad of %zu, worst parameter difference %.3g, solve bitwise equal: %s\n", sd.num_iterations, n_bad,
              np, worst, bitwise ? "yes" : "no");
  return 0;
}
