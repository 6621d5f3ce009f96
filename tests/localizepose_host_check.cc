// Driver for tests/test_gpu_localizepose_host.py and scripts/localizepose_bench.py.  Reads a model from argv[1]: int32 n_images,
// n_features[n_images], n_pairs, pair_img[n_pairs][2], match_off[n_pairs+1], matches[M][2], n_cams, cam_img[n_cams],
// feat_point[sum of the cameras' features], n_points, pt_bad[n_points], pt_views[n_points], pt_new_added[n_points],
// fail_times[n_images], image_model[n_images]; then double pt_mse[n_points], point_xyz[n_points][3], cam_R[n_cams][9], cam_t,
// cam_c, cam_fk[n_cams][3], image_focal[n_images], image_focal_init[n_images]; then float keypoints[sum of n_features][2].
// Runs one round of IncrementalSfM::Run (reference sfm_incremental.cc:126-167) in the host mirror on two copies of the model:
//   batched  LocalizeNextImage (msfm_localize_candidates + msfm_localize_poses), GenerateNew3DPoints
//   walk     FindImageToLocalize, the loop of :146-159 over LocalizeImage (one image per call, as problem i behind empty problems),
//            GenerateNew3DPoints
// and requires them to agree bit for bit: the same fail counters, the same new camera (image, model, focal length, pose,
// points, visible cameras), the same bad / new-added flags and view counts of every point, the same new points.
// Writes to argv[2], of the batched run: int32 image (-1: none), n_failed, failed[n_failed], feat_point row of the new camera
// [n_features[image]], pt_bad, pt_views, pt_new_added [n_points], n_visible, visible[n_visible], n_new, per new point (global id 1,
// global id 2, camera 2); double f, R[9], t[3], c[3], X[n_new][3], mse[n_new].
// argv[3] = "time": prints the milliseconds of the batched localisation and of the walk (median of 9 each after a warm-up).
#include <algorithm>
#include <chrono>
#include <cstdint>
#include <cstdio>
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
  std::vector<int> n_features, pair_img, match_off, matches, cam_img, feat_point, pt_bad, pt_views, pt_new_added, fail_times, image_model;
  std::vector<double> pt_mse, xyz, R, t, c, fk, image_focal, image_focal_init;
  std::vector<float> keypoints;
  int n_points = 0;
};

// cams_ / cam_models_ / pts_ of the registered part (one model per camera).  A point's view count is the size of its cams_:
// pt_views placeholders under negative keys stand for the observations the round does not read.
struct Model {
  IncrementalSfM s;
  std::vector<std::unique_ptr<Camera>> cams;
  std::vector<std::unique_ptr<CameraModel>> models;
  std::vector<std::unique_ptr<Point3D>> pts;
};

static void setup(Model& m, const Input& in) {
  IncrementalSfM& s = m.s;
  s.SetMatches(in.n_features, in.pair_img, in.match_off, in.matches);
  s.SetKeypoints(in.keypoints);
  s.image_focal_ = in.image_focal; s.image_focal_init_ = in.image_focal_init; s.image_model_ = in.image_model;
  s.localize_fail_times_ = in.fail_times;
  size_t at = 0;
  for (size_t k = 0; k < in.cam_img.size(); k++) {
    m.models.emplace_back(new CameraModel);
    CameraModel* cm = m.models.back().get();
    cm->id_ = (int)k;
    cm->f_ = in.fk[3 * k]; cm->k1_ = in.fk[3 * k + 1]; cm->k2_ = in.fk[3 * k + 2];
    cm->UpdateDataFromModel();
    cm->AddCamera((int)k);
    m.cams.emplace_back(new Camera);
    Camera* cam = m.cams.back().get();
    cam->SetID((int)k);
    cam->AssociateImage(in.cam_img[k]);
    cam->AssociateCamereModel(cm);
    for (int q = 0; q < 9; q++) cam->pos_rt_.R.m[q] = in.R[9 * k + q];
    for (int q = 0; q < 3; q++) { cam->pos_rt_.t[q] = in.t[3 * k + q]; cam->pos_ac_.c[q] = in.c[3 * k + q]; }
    s.cams_.push_back(cam);
    s.cam_models_.push_back(cm);
    s.img_cam_map_[in.cam_img[k]] = (int)k;
    s.is_img_processed_[in.cam_img[k]] = true;
  }
  for (int i = 0; i < in.n_points; i++) {
    m.pts.emplace_back(new Point3D);
    Point3D* pt = m.pts.back().get();
    pt->id_ = i;
    pt->is_new_added_ = in.pt_new_added[i] != 0;
    pt->is_bad_estimated_ = in.pt_bad[i] != 0;
    pt->mse_ = in.pt_mse[i];
    for (int q = 0; q < 3; q++) pt->data[q] = in.xyz[3 * (size_t)i + q];
    for (int v = 0; v < in.pt_views[i]; v++) pt->cams_[-1 - v] = s.cams_[v % s.cams_.size()];
    s.pts_.push_back(pt);
  }
  for (size_t k = 0; k < in.cam_img.size(); k++) {
    const int img = in.cam_img[k], nf = in.n_features[img];
    for (int f = 0; f < nf; f++)
      if (in.feat_point[at + f] >= 0) s.cams_[k]->AddPoints(s.pts_[in.feat_point[at + f]], f + img * s.options_.idx_max_per_image);
    at += nf;
  }
}

// the loop of Run :146-159 over the one-image form
static bool localize_walk(IncrementalSfM& s) {
  std::vector<int> image_ids;
  std::vector<std::vector<std::pair<int, int>>> corres_2d3d;
  std::vector<std::vector<int>> visible_cams;
  s.FindImageToLocalize(image_ids, corres_2d3d, visible_cams);
  for (size_t i = 0; i < image_ids.size(); ++i) {
    if ((int)corres_2d3d[i].size() < s.options_.th_min_2d3d_corres) continue;
    s.localize_row_ = (int)i;
    if (s.LocalizeImage(image_ids[i], corres_2d3d[i], visible_cams[i])) return true;
  }
  return false;
}

static int fail(const char* what) {
  std::printf("localizepose_host_check FAILED: %s\n", what);
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
  if (!read_ints(f, in.matches, 2 * (size_t)in.match_off[n_pairs]) || !read_ints(f, one, 1)) return 2;
  const int n_cams = one[0];
  if (n_cams < 1 || !read_ints(f, in.cam_img, n_cams)) return 2;
  size_t fp = 0;
  for (int img : in.cam_img) fp += in.n_features[img];
  if (!read_ints(f, in.feat_point, fp) || !read_ints(f, one, 1)) return 2;
  const int np = in.n_points = one[0];
  if (!read_ints(f, in.pt_bad, np) || !read_ints(f, in.pt_views, np) || !read_ints(f, in.pt_new_added, np)) return 2;
  if (!read_ints(f, in.fail_times, n_images) || !read_ints(f, in.image_model, n_images)) return 2;
  if (!read_doubles(f, in.pt_mse, np) || !read_doubles(f, in.xyz, 3 * (size_t)np) || !read_doubles(f, in.R, 9 * (size_t)n_cams) ||
      !read_doubles(f, in.t, 3 * (size_t)n_cams) || !read_doubles(f, in.c, 3 * (size_t)n_cams) || !read_doubles(f, in.fk, 3 * (size_t)n_cams) ||
      !read_doubles(f, in.image_focal, n_images) || !read_doubles(f, in.image_focal_init, n_images))
    return 2;
  size_t rows = 0;
  for (int v : in.n_features) rows += v;
  in.keypoints.resize(2 * rows);
  if (rows && std::fread(in.keypoints.data(), 4, 2 * rows, f) != 2 * rows) return 2;
  std::fclose(f);

  Model dev, host;
  setup(dev, in); setup(host, in);
  const bool ok_d = dev.s.LocalizeNextImage();
  const bool ok_h = localize_walk(host.s);
  if (ok_d != ok_h) return fail("one localised an image, the other did not");
  if (dev.s.localize_fail_times_ != host.s.localize_fail_times_) return fail("fail counters");
  if (dev.s.cams_.size() != host.s.cams_.size() || dev.s.cam_models_.size() != host.s.cam_models_.size()) return fail("camera / model counts");
  const int n_new_cams = (int)dev.s.cams_.size() - n_cams;
  if (n_new_cams != (ok_d ? 1 : 0)) return fail("cams_ did not grow by the localised image");
  for (int i = 0; i < np; i++) {
    const Point3D *a = dev.s.pts_[i], *b = host.s.pts_[i];
    if (a->is_bad_estimated_ != b->is_bad_estimated_) return fail("bad flags");
    if (a->is_new_added_ != b->is_new_added_) return fail("new-added flags");
    if (a->cams_.size() != b->cams_.size()) return fail("view counts");
  }
  if (ok_d) {
    const Camera *a = dev.s.cams_.back(), *b = host.s.cams_.back();
    if (a->id_img_ != b->id_img_ || a->id_ != b->id_ || a->id_ != n_cams) return fail("the new camera's image / id");
    if (a->cam_model_->id_ != b->cam_model_->id_ || a->cam_model_->f_ != b->cam_model_->f_ || a->cam_model_->num_cams_ != b->cam_model_->num_cams_)
      return fail("the new camera's model");
    for (int q = 0; q < 9; q++) if (a->pos_rt_.R.m[q] != b->pos_rt_.R.m[q]) return fail("R");
    for (int q = 0; q < 3; q++) if (a->pos_rt_.t[q] != b->pos_rt_.t[q] || a->pos_ac_.c[q] != b->pos_ac_.c[q]) return fail("t / c");
    if (a->visible_cams_ != b->visible_cams_) return fail("visible cameras");
    if (a->pts_.size() != b->pts_.size() || (int)a->pts_.size() != dev.s.localize_count_inliers_ ||
        dev.s.localize_count_inliers_ != host.s.localize_count_inliers_)
      return fail("inlier counts");
    auto ib = b->pts_.begin();
    for (auto ia = a->pts_.begin(); ia != a->pts_.end(); ++ia, ++ib) {
      if (ia->first != ib->first || ia->second->id_ != ib->second->id_) return fail("the new camera's points");
      const Point3D *pa = ia->second, *pb = ib->second;
      if (pa->cams_.at(ia->first) != a || pb->cams_.at(ib->first) != b) return fail("observation -> camera");
      if (pa->pts2d_.at(ia->first).x != pb->pts2d_.at(ib->first).x || pa->pts2d_.at(ia->first).y != pb->pts2d_.at(ib->first).y) return fail("keypoints");
    }
    for (int k = 0; k < n_cams; k++)
      if (dev.s.cams_[k]->visible_cams_ != host.s.cams_[k]->visible_cams_) return fail("visible graph");
    dev.s.GenerateNew3DPoints();
    host.s.GenerateNew3DPoints();
    if (dev.s.num_new_points_ != host.s.num_new_points_) return fail("number of new points");
    for (int i = 0; i < dev.s.num_new_points_; i++)
      for (int q = 0; q < 3; q++)
        if (dev.s.pts_[np + i]->data[q] != host.s.pts_[np + i]->data[q]) return fail("new points");
  }

  FILE* out = std::fopen(argv[2], "wb");
  if (!out) return 2;
  auto put = [&](const std::vector<int>& v) { if (!v.empty()) std::fwrite(v.data(), 4, v.size(), out); };
  const Camera* cam = ok_d ? dev.s.cams_.back() : nullptr;
  const int idx_max = dev.s.options_.idx_max_per_image;
  put({cam ? cam->id_img_ : -1, (int)dev.s.localize_failed_.size()});
  put(dev.s.localize_failed_);
  if (cam) {
    std::vector<int> row(in.n_features[cam->id_img_], -1);
    for (auto& kv : cam->pts_) if (kv.second->id_ < np) row[kv.first - cam->id_img_ * idx_max] = kv.second->id_;
    put(row);
  }
  std::vector<int> bad(np), views(np), added(np);
  for (int i = 0; i < np; i++) {
    int v = 0;   // (without the new points' cameras: the state behind LocalizeImage)
    for (auto& kv : dev.s.pts_[i]->cams_) v += kv.first < 0 || kv.second == cam;
    bad[i] = dev.s.pts_[i]->is_bad_estimated_; views[i] = v; added[i] = dev.s.pts_[i]->is_new_added_;
  }
  put(bad); put(views); put(added);
  const int n_new = cam ? dev.s.num_new_points_ : 0;
  if (cam) { put({(int)cam->visible_cams_.size()}); put(cam->visible_cams_); } else put({0});
  put({n_new});
  for (int i = 0; i < n_new; i++) {
    const Point3D* pt = dev.s.pts_[np + i];
    int g1 = -1, g2 = -1, c2 = -1;
    for (auto& kv : pt->cams_) { if (kv.second == cam) g1 = kv.first; else { g2 = kv.first; c2 = kv.second->id_; } }
    put({g1, g2, c2});
  }
  if (cam) {
    std::fwrite(&cam->cam_model_->f_, 8, 1, out);
    std::fwrite(cam->pos_rt_.R.m, 8, 9, out);
    for (int q = 0; q < 3; q++) { const double v = cam->pos_rt_.t[q]; std::fwrite(&v, 8, 1, out); }
    for (int q = 0; q < 3; q++) { const double v = cam->pos_ac_.c[q]; std::fwrite(&v, 8, 1, out); }
  }
  for (int i = 0; i < n_new; i++) std::fwrite(dev.s.pts_[np + i]->data, 8, 3, out);
  for (int i = 0; i < n_new; i++) std::fwrite(&dev.s.pts_[np + i]->mse_, 8, 1, out);
  std::fclose(out);

  if (argc > 3 && std::string(argv[3]) == "time") {
    std::vector<double> td, th;
    for (int rep = 0; rep < 10; rep++) {   // (the first repetition warms up)
      Model a, b;
      setup(a, in); setup(b, in);
      const double t0 = now_ms();
      a.s.LocalizeNextImage();
      const double t1 = now_ms();
      localize_walk(b.s);
      const double t2 = now_ms();
      if (rep) { td.push_back(t1 - t0); th.push_back(t2 - t1); }
    }
    std::sort(td.begin(), td.end()); std::sort(th.begin(), th.end());
    std::printf("time_ms batched %.3f walk %.3f\n", td[td.size() / 2], th[th.size() / 2]);
  }
  std::printf("localizepose_host_check ok: image %d, %d failed before it, %d inliers, %d new points\n", cam ? cam->id_img_ : -1,
              (int)dev.s.localize_failed_.size(), dev.s.localize_count_inliers_, n_new);
  return 0;
}
