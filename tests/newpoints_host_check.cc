// Driver for tests/test_gpu_newpoints_host.py and scripts/newpoints_bench.py.  Reads a model from argv[1]: int32 n_images,
// n_features[n_images], n_pairs, pair_img[n_pairs][2], match_off[n_pairs+1], matches[M][2], n_cams, cam_img[n_cams],
// feat_point[sum of the cameras' features], n_points, n_visible, visible[n_visible] (the visible_cams_ of the newest camera,
// n_cams - 1); then double cam_R[n_cams][9], cam_t, cam_c, cam_fk[n_cams][3] and float keypoints[sum of n_features][2].
// Runs the host mirror's IncrementalSfM::GenerateNew3DPoints (one msfm_new_points call; host/objectsfm.cc, reference
// sfm_incremental.cc:755-915) and its walk GenerateNew3DPointsHost (one Trianglate2 per candidate) on two copies of the
// model and requires them to agree: the same points in the same order with the same observations and the same inserts into
// the cameras, X and mse to 1e-9 (the walk triangulates through msfm_triangulate_midpoint_batch, which is compiled with fused
// multiply-adds).
// Writes to argv[2]: int32 n_new, then per point (global id 1, global id 2, camera 2, takes 1, takes 2), then the feat_point
// table of the model afterwards; double X[n_new][3], mse[n_new] - of the batched run.
// argv[3] = "time": prints the milliseconds of the batched call and of the walk (median of 9 each after a warm-up).
#include <algorithm>
#include <chrono>
#include <cmath>
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
  std::vector<int> n_features, pair_img, match_off, matches, cam_img, feat_point, visible;
  std::vector<double> R, t, c, fk;
  std::vector<float> keypoints;
  int n_points = 0;
};

// cams_ / cam_models_ / pts_ as LocalizeImage leaves them (one model per camera; the existing points carry no observations:
// GenerateNew3DPoints reads only which features hold one)
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
  for (int i = 0; i < in.n_points; i++) {
    m.pts.emplace_back(new Point3D);
    m.pts.back()->id_ = i;
    m.pts.back()->is_new_added_ = false;
    s.pts_.push_back(m.pts.back().get());
  }
  size_t at = 0;
  for (size_t k = 0; k < in.cam_img.size(); k++) {
    m.models.emplace_back(new CameraModel);
    CameraModel* cm = m.models.back().get();
    cm->f_ = in.fk[3 * k]; cm->k1_ = in.fk[3 * k + 1]; cm->k2_ = in.fk[3 * k + 2];
    cm->UpdateDataFromModel();
    m.cams.emplace_back(new Camera);
    Camera* cam = m.cams.back().get();
    cam->SetID((int)k);
    cam->AssociateImage(in.cam_img[k]);
    cam->AssociateCamereModel(cm);
    for (int q = 0; q < 9; q++) cam->pos_rt_.R.m[q] = in.R[9 * k + q];
    for (int q = 0; q < 3; q++) { cam->pos_rt_.t[q] = in.t[3 * k + q]; cam->pos_ac_.c[q] = in.c[3 * k + q]; }
    const int img = in.cam_img[k], nf = in.n_features[img];
    for (int f = 0; f < nf; f++)
      if (in.feat_point[at + f] >= 0) cam->AddPoints(s.pts_[in.feat_point[at + f]], f + img * s.options_.idx_max_per_image);
    at += nf;
    s.cams_.push_back(cam);
    s.cam_models_.push_back(cm);
    s.img_cam_map_[img] = (int)k;
    s.is_img_processed_[img] = true;
  }
  s.cams_.back()->visible_cams_ = in.visible;
}

static int fail(const char* what) {
  std::printf("newpoints_host_check FAILED: %s\n", what);
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
  in.n_points = one[0];
  if (!read_ints(f, one, 1) || !read_ints(f, in.visible, one[0])) return 2;
  if (!read_doubles(f, in.R, 9 * (size_t)n_cams) || !read_doubles(f, in.t, 3 * (size_t)n_cams) || !read_doubles(f, in.c, 3 * (size_t)n_cams) ||
      !read_doubles(f, in.fk, 3 * (size_t)n_cams))
    return 2;
  size_t rows = 0;
  for (int v : in.n_features) rows += v;
  in.keypoints.resize(2 * rows);
  if (rows && std::fread(in.keypoints.data(), 4, 2 * rows, f) != 2 * rows) return 2;
  std::fclose(f);

  Model dev, host;
  setup(dev, in); setup(host, in);
  dev.s.GenerateNew3DPoints();
  host.s.GenerateNew3DPointsHost();
  const int n = dev.s.num_new_points_;
  if (n != host.s.num_new_points_ || dev.s.pts_.size() != host.s.pts_.size()) return fail("number of new points");
  if ((int)dev.s.pts_.size() != in.n_points + n) return fail("pts_ did not grow by the new points");
  const Camera* c1 = dev.s.cams_.back();
  std::vector<int> rec;
  for (int i = 0; i < n; i++) {
    const Point3D *a = dev.s.pts_[in.n_points + i], *b = host.s.pts_[in.n_points + i];
    if (a->id_ != in.n_points + i || b->id_ != a->id_ || !a->is_new_added_ || a->cams_.size() != 2 || b->cams_.size() != 2) return fail("point record");
    int ga[2] = {0, 0}, ca[2] = {0, 0};
    int k = 0;
    auto ib = b->cams_.begin();
    for (auto ia = a->cams_.begin(); ia != a->cams_.end(); ++ia, ++ib, ++k) {
      if (ia->first != ib->first || ia->second->id_ != ib->second->id_) return fail("observations");
      if (a->pts2d_.at(ia->first).x != b->pts2d_.at(ib->first).x || a->pts2d_.at(ia->first).y != b->pts2d_.at(ib->first).y) return fail("keypoints");
      ga[k] = ia->first; ca[k] = ia->second->id_;
    }
    const int s1 = ca[0] == c1->id_ ? 0 : 1;   // which of the two observations is the new camera's
    if (ca[s1] != c1->id_) return fail("no observation in the new camera");
    int takes[2];
    for (int q = 0; q < 2; q++) {
      const bool td = dev.s.cams_[ca[q]]->pts_.at(ga[q]) == a, th = host.s.cams_[ca[q]]->pts_.at(ga[q]) == b;
      if (td != th) return fail("inserts into the cameras");
      takes[q] = td ? 1 : 0;
    }
    for (int q = 0; q < 3; q++)
      if (std::fabs(a->data[q] - b->data[q]) > 1e-9 + 1e-9 * std::fabs(b->data[q])) return fail("X beyond 1e-9");
    if (std::fabs(a->mse_ - b->mse_) > 1e-9 + 1e-9 * std::fabs(b->mse_)) return fail("mse beyond 1e-9");
    const int r[5] = {ga[s1], ga[1 - s1], ca[1 - s1], takes[s1], takes[1 - s1]};
    rec.insert(rec.end(), r, r + 5);
  }
  for (size_t k = 0; k < dev.s.cams_.size(); k++)
    if (dev.s.cams_[k]->pts_.size() != host.s.cams_[k]->pts_.size()) return fail("camera point counts");

  FILE* out = std::fopen(argv[2], "wb");
  if (!out) return 2;
  std::fwrite(&n, 4, 1, out);
  if (n) std::fwrite(rec.data(), 4, rec.size(), out);
  for (size_t k = 0; k < dev.s.cams_.size(); k++) {   // feat_point afterwards
    const int img = in.cam_img[k];
    std::vector<int> row(in.n_features[img], -1);
    for (auto& kv : dev.s.cams_[k]->pts_) row[kv.first - img * dev.s.options_.idx_max_per_image] = kv.second->id_;
    if (!row.empty()) std::fwrite(row.data(), 4, row.size(), out);
  }
  for (int i = 0; i < n; i++) std::fwrite(dev.s.pts_[in.n_points + i]->data, 8, 3, out);
  for (int i = 0; i < n; i++) std::fwrite(&dev.s.pts_[in.n_points + i]->mse_, 8, 1, out);
  std::fclose(out);

  if (argc > 3 && std::string(argv[3]) == "time") {
    std::vector<double> td, th;
    for (int rep = 0; rep < 10; rep++) {   // (the first repetition warms up)
      Model a, b;
      setup(a, in); setup(b, in);
      const double t0 = now_ms();
      a.s.GenerateNew3DPoints();
      const double t1 = now_ms();
      b.s.GenerateNew3DPointsHost();
      const double t2 = now_ms();
      if (rep) { td.push_back(t1 - t0); th.push_back(t2 - t1); }
    }
    std::sort(td.begin(), td.end()); std::sort(th.begin(), th.end());
    std::printf("time_ms batched %.3f walk %.3f points %d\n", td[td.size() / 2], th[th.size() / 2], n);
  }
  std::printf("newpoints_host_check ok: %d new points behind %d\n", n, in.n_points);
  return 0;
}
