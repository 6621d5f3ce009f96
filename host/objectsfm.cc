// See objectsfm.h.  Host-side glue only: gather -> C ABI -> scatter.
#include "objectsfm.h"

#include <algorithm>
#include <cstdio>
#include <fstream>
#include <iomanip>
#include <cstdlib>
#include <limits>
#include <numeric>
#include <stdexcept>

namespace objectsfm {

// ---- rotation (SfM/src/utils/basic_funcs.cc:25-158) --------------------------------------
void rotation::AngleAxisToRotationMatrix(const Vec3& aa, Mat3& R) {
  const double theta2 = aa[0] * aa[0] + aa[1] * aa[1] + aa[2] * aa[2];
  if (theta2 > std::numeric_limits<double>::epsilon()) {
    const double theta = std::sqrt(theta2);
    const double wx = aa[0] / theta, wy = aa[1] / theta, wz = aa[2] / theta;
    const double c = std::cos(theta), s = std::sin(theta);
    R(0, 0) = c + wx * wx * (1 - c);       R(1, 0) = wz * s + wx * wy * (1 - c);  R(2, 0) = -wy * s + wx * wz * (1 - c);
    R(0, 1) = wx * wy * (1 - c) - wz * s;  R(1, 1) = c + wy * wy * (1 - c);       R(2, 1) = wx * s + wy * wz * (1 - c);
    R(0, 2) = wy * s + wx * wz * (1 - c);  R(1, 2) = -wx * s + wy * wz * (1 - c); R(2, 2) = c + wz * wz * (1 - c);
  } else {
    R(0, 0) = 1; R(1, 0) = aa[2]; R(2, 0) = -aa[1];
    R(0, 1) = -aa[2]; R(1, 1) = 1; R(2, 1) = aa[0];
    R(0, 2) = aa[1]; R(1, 2) = -aa[0]; R(2, 2) = 1;
  }
}

void rotation::RotationMatrixToAngleAxis(const Mat3& R, Vec3& axis) {
  double q[4];
  const double trace = R(0, 0) + R(1, 1) + R(2, 2);
  if (trace >= 0.0) {
    double t = std::sqrt(trace + 1.0);
    q[0] = 0.5 * t; t = 0.5 / t;
    q[1] = (R(2, 1) - R(1, 2)) * t; q[2] = (R(0, 2) - R(2, 0)) * t; q[3] = (R(1, 0) - R(0, 1)) * t;
  } else {
    int i = 0;
    if (R(1, 1) > R(0, 0)) i = 1;
    if (R(2, 2) > R(i, i)) i = 2;
    const int j = (i + 1) % 3, k = (j + 1) % 3;
    double t = std::sqrt(R(i, i) - R(j, j) - R(k, k) + 1.0);
    q[i + 1] = 0.5 * t; t = 0.5 / t;
    q[0] = (R(k, j) - R(j, k)) * t; q[j + 1] = (R(j, i) + R(i, j)) * t; q[k + 1] = (R(k, i) + R(i, k)) * t;
  }
  const double s2 = q[1] * q[1] + q[2] * q[2] + q[3] * q[3];
  double k = 2.0;
  if (s2 > 0.0) {
    const double s = std::sqrt(s2);
    k = 2.0 * ((q[0] < 0.0) ? std::atan2(-s, -q[0]) : std::atan2(s, q[0])) / s;
  }
  axis[0] = q[1] * k; axis[1] = q[2] * k; axis[2] = q[3] * k;
}

// ---- CameraModel / Camera ------------------------------------------------------------------
CameraModel::CameraModel(int id, int h, int w, double f_mm, double f, std::string cam_maker, std::string cam_model) {
  f_mm_ = f_mm; f_ = f; f_hyp_ = (w > h ? w : h) * 1.2; w_ = w; h_ = h; px_ = w / 2.0; py_ = h / 2.0;
  id_ = id; cam_maker_ = cam_maker; cam_model_ = cam_model;
  UpdateDataFromModel();
}

void Camera::SetRTPose(const Mat3& R, const Vec3& t) {
  pos_rt_.R = R; pos_rt_.t = t;
  rotation::RotationMatrixToAngleAxis(pos_rt_.R, pos_ac_.a);
  const Vec3 c = transpose(R) * t;  // c = -R^-1 t
  for (int i = 0; i < 3; i++) pos_ac_.c[i] = -c[i];
  UpdateDataFromPose();
}

void Camera::SetACPose(const Vec3& a, const Vec3& c) {
  pos_ac_.a = a; pos_ac_.c = c;
  rotation::AngleAxisToRotationMatrix(pos_ac_.a, pos_rt_.R);
  const Vec3 t = pos_rt_.R * c;
  for (int i = 0; i < 3; i++) pos_rt_.t[i] = -t[i];
  UpdateDataFromPose();
}

void Camera::UpdateDataFromPose() {
  for (int i = 0; i < 3; i++) { data[i] = pos_ac_.a[i]; data[3 + i] = pos_rt_.t[i]; }
  for (int r = 0; r < 3; r++) { for (int c = 0; c < 3; c++) M[4 * r + c] = pos_rt_.R(r, c); M[4 * r + 3] = pos_rt_.t[r]; }
}

void Camera::UpdatePoseFromData() {
  for (int i = 0; i < 3; i++) { pos_ac_.a[i] = data[i]; pos_rt_.t[i] = data[3 + i]; }
  rotation::AngleAxisToRotationMatrix(pos_ac_.a, pos_rt_.R);
  const Vec3 c = transpose(pos_rt_.R) * pos_rt_.t;
  for (int i = 0; i < 3; i++) pos_ac_.c[i] = -c[i];
  for (int r = 0; r < 3; r++) { for (int cc = 0; cc < 3; cc++) M[4 * r + cc] = pos_rt_.R(r, cc); M[4 * r + 3] = pos_rt_.t[r]; }
}

// ---- context ---------------------------------------------------------------------------------
static msfm_ctx* g_ctx = nullptr;
static void destroy_ctx() { if (g_ctx) msfm_ctx_destroy(g_ctx); g_ctx = nullptr; }
msfm_ctx* Context() {
  if (!g_ctx) {
    if (msfm_ctx_create(-1, &g_ctx) != MSFM_OK) throw std::runtime_error("libmsfm: no usable MI355X (there is no CPU fallback)");
    std::atexit(destroy_ctx);
  }
  return g_ctx;
}
static void check(int rc, const char* what) {
  if (rc != MSFM_OK) throw std::runtime_error(std::string(what) + ": " + msfm_last_error(g_ctx));
}
// Several GPUs from the one process the reference is (test_sfm.cc:22-70 `main`): msfm_ctx_create_multi owns a context and a
// host thread per device and the communicator; the calls below that shard (matching, triangulation / reprojection, bundle
// adjustment) go through it, everything else through its rank-0 context.
static msfm_multi* g_multi = nullptr;
static void destroy_multi() { if (g_multi) msfm_multi_destroy(g_multi); g_multi = nullptr; g_ctx = nullptr; }
void UseGpus(int n_gpus, bool share_device_0) {
  if (g_multi || g_ctx) throw std::runtime_error("UseGpus: call before the first GPU call");
  if (n_gpus <= 1) return;
  std::vector<int> dev(n_gpus);
  for (int i = 0; i < n_gpus; i++) dev[i] = share_device_0 ? 0 : i;
  if (msfm_ctx_create_multi(n_gpus, dev.data(), &g_multi) != MSFM_OK) throw std::runtime_error("msfm_ctx_create_multi failed");
  g_ctx = msfm_multi_ctx(g_multi, 0);
  std::atexit(destroy_multi);
}
static void check_multi(int rc, const char* what) {
  if (rc != MSFM_OK) throw std::runtime_error(std::string(what) + ": " + msfm_multi_last_error(g_multi));
}

// ---- Point3D ------------------------------------------------------------------------------------
void Point3D::AddObservation(Camera* cam, double x, double y, int idx) {
  cams_.insert(std::make_pair(idx, cam));
  Vec2 p; p.x = x; p.y = y;
  pts2d_.insert(std::make_pair(idx, p));
}

namespace {
// Flatten a set of points into msfm_tracks (std::map key order, as every reference loop iterates).
struct Flat {
  std::vector<int32_t> off, cam;
  std::vector<double> xy, R, t, c, fk;
  std::map<Camera*, int> index;
  msfm_tracks tr;
  explicit Flat(const std::vector<Point3D*>& pts) {
    off.push_back(0);
    for (Point3D* p : pts) {
      auto ic = p->cams_.begin();
      auto ip = p->pts2d_.begin();
      for (; ic != p->cams_.end(); ++ic, ++ip) {
        auto f = index.find(ic->second);
        int id;
        if (f == index.end()) {
          id = (int)index.size();
          index[ic->second] = id;
          Camera* cm = ic->second;
          for (int k = 0; k < 9; k++) R.push_back(cm->pos_rt_.R.m[k]);
          for (int k = 0; k < 3; k++) { t.push_back(cm->pos_rt_.t[k]); c.push_back(cm->pos_ac_.c[k]); }
          fk.push_back(cm->cam_model_->f_); fk.push_back(cm->cam_model_->k1_); fk.push_back(cm->cam_model_->k2_);
        } else {
          id = f->second;
        }
        cam.push_back(id);
        xy.push_back(ip->second.x); xy.push_back(ip->second.y);
      }
      off.push_back((int32_t)cam.size());
    }
    if (index.empty()) { R.assign(9, 0); t.assign(3, 0); c.assign(3, 0); fk.assign(3, 1); }
    tr.n_tracks = (int)pts.size(); tr.n_cams = (int)std::max<size_t>(1, index.size());
    tr.track_off = off.data(); tr.track_cam = cam.data(); tr.track_xy = xy.data();
    tr.cam_R = R.data(); tr.cam_t = t.data(); tr.cam_c = c.data(); tr.cam_fk = fk.data();
  }
};
}  // namespace

void TrianglateBatch(const std::vector<Point3D*>& pts, double th_error, double th_angle, bool dlt, std::vector<char>* ok) {
  Flat F(pts);
  std::vector<double> X(3 * pts.size()), mse(pts.size());
  std::vector<uint8_t> okv(pts.size());
  for (size_t i = 0; i < pts.size(); i++) for (int k = 0; k < 3; k++) X[3 * i + k] = pts[i]->data[k];
  if (g_multi)
    check_multi(dlt ? msfm_multi_triangulate_dlt_batch(g_multi, &F.tr, th_error, th_angle, X.data(), mse.data(), okv.data())
                    : msfm_multi_triangulate_midpoint_batch(g_multi, &F.tr, th_error, th_angle, X.data(), mse.data(), okv.data()),
                "triangulate");
  else
    check(dlt ? msfm_triangulate_dlt_batch(Context(), &F.tr, th_error, th_angle, X.data(), mse.data(), okv.data())
              : msfm_triangulate_midpoint_batch(Context(), &F.tr, th_error, th_angle, X.data(), mse.data(), okv.data()),
          "triangulate");
  if (ok) ok->assign(pts.size(), 0);
  for (size_t i = 0; i < pts.size(); i++) {
    for (int k = 0; k < 3; k++) pts[i]->data[k] = X[3 * i + k];
    pts[i]->mse_ = mse[i];
    if (ok) (*ok)[i] = (char)okv[i];
  }
}

void ReprojectionBatch(const std::vector<Point3D*>& pts) {
  Flat F(pts);
  std::vector<double> X(3 * pts.size()), mse(pts.size());
  for (size_t i = 0; i < pts.size(); i++) for (int k = 0; k < 3; k++) X[3 * i + k] = pts[i]->data[k];
  if (g_multi) check_multi(msfm_multi_reproject_mse_batch(g_multi, &F.tr, X.data(), mse.data()), "reproject");
  else check(msfm_reproject_mse_batch(Context(), &F.tr, X.data(), mse.data()), "reproject");
  for (size_t i = 0; i < pts.size(); i++) pts[i]->mse_ = mse[i];
}

bool Point3D::Trianglate(double th_error, double th_angle) {
  std::vector<char> ok;
  TrianglateBatch(std::vector<Point3D*>(1, this), th_error, th_angle, true, &ok);
  return ok[0] != 0;
}
bool Point3D::Trianglate2(double th_error, double th_angle) {
  std::vector<char> ok;
  TrianglateBatch(std::vector<Point3D*>(1, this), th_error, th_angle, false, &ok);
  return ok[0] != 0;
}
void Point3D::Reprojection() { ReprojectionBatch(std::vector<Point3D*>(1, this)); }
bool Point3D::SufficientTriangulationAngle(double th) {
  // the acceptance test of the batch kernel with an unbounded error threshold isolates the angle gate
  Flat F(std::vector<Point3D*>(1, this));
  double X[3] = {data[0], data[1], data[2]}, mse = 0;
  uint8_t ok = 0;
  (void)X; (void)mse;
  std::vector<double> c(F.c);
  const int k = F.off[1];
  const double cos_min = std::cos(th);
  for (int i = 0; i + 1 < k; i++)
    for (int j = i + 1; j < k; j++) {
      double a[3], b[3], na = 0, nb = 0, d = 0;
      for (int q = 0; q < 3; q++) { a[q] = data[q] - c[3 * F.cam[i] + q]; b[q] = data[q] - c[3 * F.cam[j] + q]; na += a[q] * a[q]; nb += b[q] * b[q]; }
      for (int q = 0; q < 3; q++) d += a[q] / std::sqrt(na) * (b[q] / std::sqrt(nb));
      if (d < cos_min) ok = 1;
    }
  return ok != 0;
}

// ---- BundleAdjuster -----------------------------------------------------------------------------
BundleAdjuster::BundleAdjuster(std::vector<Camera*> cams, std::vector<CameraModel*> cam_models, std::vector<Point3D*> pts)
    : cams_(std::move(cams)), cam_models_(std::move(cam_models)), pts_(std::move(pts)) {
  msfm_ba_options_default(&options_);
  summary_ = msfm_ba_summary();
}

void BundleAdjuster::SetOptions(BundleAdjustOptions options) {
  options_.max_num_iterations = options.max_num_iterations;
  options_.progress_to_stdout = options.minimizer_progress_to_stdout ? 1 : 0;
  options_.num_threads = options.num_threads;  // linear solver: dense Schur, always (optimizer.cc:47)
}

void BundleAdjuster::RunOptimizetion(bool is_initial_run, double weight) {
  if (is_initial_run) { Normalize(); Perturb(); }
  // gather (optimizer.cc:59-129): points ascending, observations in std::map key order, bad points skipped
  std::map<Camera*, int> cam_id;
  std::map<CameraModel*, int> model_id;
  for (size_t i = 0; i < cams_.size(); i++) cam_id[cams_[i]] = (int)i;
  for (size_t i = 0; i < cam_models_.size(); i++) model_id[cam_models_[i]] = (int)i;
  std::vector<double> cam_pose(6 * cams_.size()), cam_model(3 * cam_models_.size()), point, obs_xy, pt_weight;
  std::vector<int32_t> model_of_cam(cams_.size()), obs_cam, obs_pt;
  std::vector<uint8_t> cam_mut(cams_.size()), model_mut(cam_models_.size()), pt_mut;
  std::vector<Point3D*> used;
  for (size_t i = 0; i < cams_.size(); i++) {
    for (int k = 0; k < 6; k++) cam_pose[6 * i + k] = cams_[i]->data[k];
    model_of_cam[i] = model_id.at(cams_[i]->cam_model_);
    cam_mut[i] = cams_[i]->is_mutable_;
  }
  for (size_t i = 0; i < cam_models_.size(); i++) {
    for (int k = 0; k < 3; k++) cam_model[3 * i + k] = cam_models_[i]->data[k];
    model_mut[i] = cam_models_[i]->is_mutable_;
  }
  for (Point3D* p : pts_) {
    if (p->is_bad_estimated_) continue;                 // optimizer.cc:64
    if (!keep_point_weights_) {
      if (p->cams_.size() == 2) p->weight = 1.0;        // optimizer.cc:69-78
      if (p->cams_.size() >= 3) p->weight = weight;
    }
    // a residual block exists only where the point or the camera is free (optimizer.cc:86-125): rows of a frozen point in
    // frozen cameras, and points left without any row, are not part of the problem (for the window of one camera out of
    // thousands that is nearly everything)
    const int pid = (int)used.size();
    bool any = false;
    auto ic = p->cams_.begin();
    auto ip = p->pts2d_.begin();
    for (; ic != p->cams_.end(); ++ic, ++ip) {
      if (!p->is_mutable_ && !ic->second->is_mutable_) continue;
      obs_cam.push_back(cam_id.at(ic->second));
      obs_pt.push_back(pid);
      obs_xy.push_back(ip->second.x); obs_xy.push_back(ip->second.y);
      any = true;
    }
    if (!any) continue;
    used.push_back(p);
    for (int k = 0; k < 3; k++) point.push_back(p->data[k]);
    pt_weight.push_back(p->weight);
    pt_mut.push_back(p->is_mutable_);
  }
  msfm_ba_problem P;
  P.n_cams = (int)cams_.size(); P.n_models = (int)cam_models_.size(); P.n_points = (int)used.size(); P.n_obs = (int)obs_cam.size();
  P.cam_pose = cam_pose.data(); P.cam_model = cam_model.data(); P.cam_model_of_cam = model_of_cam.data(); P.point = point.data();
  P.obs_cam = obs_cam.data(); P.obs_pt = obs_pt.data(); P.obs_xy = obs_xy.data(); P.pt_weight = pt_weight.data();
  P.cam_mutable = cam_mut.data(); P.model_mutable = model_mut.data(); P.pt_mutable = pt_mut.data();
  P.gps_xyz = nullptr; P.gps_weight = 0;
  std::vector<double> gps_xyz;
  if (!cams_gps_.empty()) {
    if (cams_gps_.size() != cams_.size()) throw std::runtime_error("SetGPS: one position per camera expected");
    // slam_gps.cc:818-830: `double weight = count1 / cams_.size();` - both int, so the division truncates; count1 is
    // the number of reprojection residual blocks added (rows whose camera and point are both frozen add none)
    long count1 = 0;
    for (size_t o = 0; o < obs_cam.size(); o++) count1 += (cam_mut[obs_cam[o]] || pt_mut[obs_pt[o]]) ? 1 : 0;
    gps_xyz.resize(3 * cams_.size());
    for (size_t i = 0; i < cams_.size(); i++) for (int k = 0; k < 3; k++) gps_xyz[3 * i + k] = cams_gps_[i][k];
    P.gps_xyz = gps_xyz.data();
    P.gps_weight = (double)(count1 / (long)cams_.size());
  }
  iterations_.assign((size_t)options_.max_num_iterations + 2, msfm_ba_iteration());
  summary_.iterations = iterations_.data();
  summary_.iterations_capacity = (int)iterations_.size();
  // == ceres::Solve, optimizer.cc:133 (several GPUs: the same call with the points split inside the library)
  if (g_multi) check_multi(msfm_multi_ba_solve(g_multi, &P, &options_, &summary_), "msfm_multi_ba_solve");
  else check(msfm_ba_solve(Context(), &P, &options_, &summary_), "msfm_ba_solve");
  // Ceres writes through the data blocks; so do we
  for (size_t i = 0; i < cams_.size(); i++) for (int k = 0; k < 6; k++) cams_[i]->data[k] = cam_pose[6 * i + k];
  for (size_t i = 0; i < cam_models_.size(); i++) for (int k = 0; k < 3; k++) cam_models_[i]->data[k] = cam_model[3 * i + k];
  for (size_t i = 0; i < used.size(); i++) for (int k = 0; k < 3; k++) used[i]->data[k] = point[3 * i + k];
}

void BundleAdjuster::UpdateParameters() {
  for (Camera* c : cams_) c->UpdatePoseFromData();
  for (CameraModel* m : cam_models_) m->UpdataModelFromData();
}

void BundleAdjuster::Normalize() {
  const int n = (int)pts_.size();
  double mid[3] = {0, 0, 0};
  for (Point3D* p : pts_) for (int k = 0; k < 3; k++) mid[k] += p->data[k];
  for (int k = 0; k < 3; k++) mid[k] /= n;
  double mad = 0;
  for (Point3D* p : pts_) mad += std::fabs(p->data[0] - mid[0]) + std::fabs(p->data[1] - mid[1]) + std::fabs(p->data[2] - mid[2]);
  mad /= n;
  const double scale = 100.0 / mad;
  for (Point3D* p : pts_) for (int k = 0; k < 3; k++) p->data[k] = scale * (p->data[k] - mid[k]);
  for (Camera* c : cams_) {
    Vec3 cc;
    for (int k = 0; k < 3; k++) cc[k] = scale * (c->pos_ac_.c[k] - mid[k]);
    c->SetACPose(c->pos_ac_.a, cc);
  }
}

void BundleAdjuster::Perturb() {
  std::mt19937_64 gen(perturb_seed_);
  std::normal_distribution<double> nrm(0.0, 1.0);
  const double rotation_sigma = 0.1, translation_sigma = 0.5, point_sigma = 0.5;
  for (Point3D* p : pts_) for (int k = 0; k < 3; k++) p->data[k] += nrm(gen) * point_sigma;
  for (Camera* c : cams_) {
    Vec3 a = c->pos_ac_.a;
    for (int k = 0; k < 3; k++) a[k] += nrm(gen) * rotation_sigma;
    c->SetACPose(a, c->pos_ac_.c);
    Vec3 t = c->pos_rt_.t;
    for (int k = 0; k < 3; k++) t[k] += nrm(gen) * translation_sigma;
    c->SetRTPose(c->pos_rt_.R, t);
  }
}

// ---- IncrementalSfM: window selection + the two adjustments ---------------------------------------
void IncrementalSfM::ImmutableCamsPoints() {
  for (Camera* c : cams_) {
    c->SetMutable(false);
    for (auto& kv : c->pts_) kv.second->SetMutable(false);
  }
}

void IncrementalSfM::MutableCamsPoints() {
  for (Camera* c : cams_) {
    c->SetMutable(true);
    for (auto& kv : c->pts_) kv.second->SetMutable(true);
  }
}

void IncrementalSfM::UpdateVisibleGraph(int idx_new_cam, std::vector<int> idxs_visible_cam) {
  cams_[idx_new_cam]->AddVisibleCamera(idx_new_cam);
  for (int v : idxs_visible_cam) {
    cams_[idx_new_cam]->AddVisibleCamera(v);
    cams_[v]->AddVisibleCamera(idx_new_cam);
  }
}

std::vector<int> IncrementalSfM::VisibleCameras(int idx_cam) const {
  // a 2D-3D match through camera j = a point of camera j (not bad) that the new camera observes too
  std::map<const Camera*, int> count;
  for (auto& kv : cams_[idx_cam]->pts_) {
    const Point3D* p = kv.second;
    if (p->is_bad_estimated_) continue;
    for (auto& pc : p->cams_) if (pc.second != cams_[idx_cam]) count[pc.second]++;
  }
  std::vector<int> vis;
  for (size_t j = 0; j < cams_.size(); j++) {
    auto it = count.find(cams_[j]);
    if (it != count.end() && it->second > options_.th_visible_matches) vis.push_back((int)j);
  }
  return vis;
}

void IncrementalSfM::PartialBundleAdjustment(int idx) {
  ImmutableCamsPoints();
  // optimize only the new camera (all cameras of its model) and its visible cameras, with their good points
  auto free_cam = [&](int idx_cam) {
    cams_[idx_cam]->SetMutable(true);
    for (auto& kv : cams_[idx_cam]->pts_) if (!kv.second->is_bad_estimated_) kv.second->SetMutable(true);
  };
  for (int idx_cam : cams_[idx]->cam_model_->idx_cams_) free_cam(idx_cam);
  for (int idx_cam : cams_[idx]->visible_cams_) free_cam(idx_cam);
  BundleAdjuster bundler(cams_, cam_models_, pts_);
  bundler.SetOptions(bundle_partial_options_);
  bundler.SetGPS(cams_gps_);
  bundler.RunOptimizetion(!found_seed_, 2.0);
  bundler.UpdateParameters();
  summary_ = bundler.summary_;
  iterations_ = bundler.iterations_;
  summary_.iterations = iterations_.data();
}

void IncrementalSfM::FullBundleAdjustment() {
  MutableCamsPoints();
  BundleAdjuster bundler(cams_, cam_models_, pts_);
  bundler.SetOptions(bundle_full_options_);
  bundler.SetGPS(cams_gps_);
  bundler.RunOptimizetion(!found_seed_, 1.0);
  bundler.UpdateParameters();
  summary_ = bundler.summary_;
  iterations_ = bundler.iterations_;
  summary_.iterations = iterations_.data();
}

void IncrementalSfM::RemovePointOutliers() {
  std::vector<Point3D*> live;
  for (Point3D* p : pts_) if (!p->is_bad_estimated_) live.push_back(p);
  ReprojectionBatch(live);   // pts_[i]->Reprojection() for every live point, one launch
  for (Point3D* p : live) {
    if (std::sqrt(p->mse_) > options_.th_mse_outliers) p->is_bad_estimated_ = true;
    p->is_new_added_ = false;
  }
}

// ---- IncrementalSfM: the seed pair ----------------------------------------------------------------
IncrementalSfM::IncrementalSfM() { msfm_seed_default_options(&seed_options_); msfm_localize_pose_default_options(&localize_options_); }

void IncrementalSfM::SortImagePairs(std::vector<std::pair<int, int>>& seed_pair_hyps) const {
  const int num_img = (int)graph_.n_features.size();
  std::vector<float> match_strength(num_img, 0);
  for (int i = 0; i < num_img; i++) {
    float sum = 0;                                   // math::sum(T*, int, float&), basic_funcs.h:50-57
    for (int j = 0; j < num_img; j++) sum += graph_.match_graph_[(size_t)i * num_img + j];
    match_strength[i] = (float)std::log(sum + 2.0);
  }
  std::vector<std::pair<int, float>> pairs;
  for (int i = 0; i + 1 < num_img; i++) {
    if (is_img_processed_[i]) continue;
    for (int j = i + 1; j < num_img; j++) {
      const int num_match_ij = graph_.match_graph_[(size_t)i * num_img + j];
      if (!num_match_ij || is_img_processed_[j]) continue;
      const double strength = match_strength[i] * match_strength[j] * std::log((double)num_match_ij);
      pairs.push_back(std::pair<int, float>(i * num_img + j, (float)strength));
    }
  }
  std::sort(pairs.begin(), pairs.end(), [](const std::pair<int, float>& l, const std::pair<int, float>& r) {
    return l.second > r.second || (l.second == r.second && l.first < r.first);
  });
  seed_pair_hyps.clear();
  for (auto& p : pairs) seed_pair_hyps.push_back(std::make_pair(p.first / num_img, p.first % num_img));
}

namespace {
struct SeedAnswer {   // one hypothesis behind the gates
  bool pass = false;
  double f[2] = {0, 0};
  Mat3 R; Vec3 t;
  std::vector<int> pt_match;
  std::vector<double> X, mse;
};
}  // namespace

// :252-290, :334, :352-373, :401-408 for the hypothesis that passed: two cameras, their model(s), the accepted points
static void seed_adopt(IncrementalSfM& s, int id_img1, int id_img2, const SeedAnswer& a) {
  const int nf_first1 = std::accumulate(s.graph_.n_features.begin(), s.graph_.n_features.begin() + id_img1, 0);
  const int nf_first2 = std::accumulate(s.graph_.n_features.begin(), s.graph_.n_features.begin() + id_img2, 0);
  int m0 = -1;
  for (size_t p = 0; p < s.graph_.pair_img.size() / 2; p++)
    if (s.graph_.pair_img[2 * p] == id_img1 && s.graph_.pair_img[2 * p + 1] == id_img2) m0 = s.graph_.match_off[p];
  if (m0 < 0) throw std::runtime_error("FindSeedPairThenReconstruct: the winning pair is not in graph_");
  // the seed search starts a model (:253): a caller that still holds cameras, models or points of an earlier one owns them
  if (!s.cams_.empty() || !s.cam_models_.empty() || !s.pts_.empty())
    throw std::runtime_error("FindSeedPairThenReconstruct: cams_ / cam_models_ / pts_ must be empty");
  s.cams_.assign(2, nullptr);
  for (int k = 0; k < 2; k++) { s.cams_[k] = new Camera; s.cams_[k]->AssociateImage(k ? id_img2 : id_img1); s.cams_[k]->SetID(k); }
  const bool shared = s.image_model_[id_img1] == s.image_model_[id_img2];
  for (int k = 0; k < (shared ? 1 : 2); k++) {
    CameraModel* m = new CameraModel(k, 0, 0, 0.0, a.f[k], "", "");
    s.cam_models_.push_back(m);
  }
  s.cams_[0]->AssociateCamereModel(s.cam_models_[s.cam_models_.size() - (shared ? 1 : 2)]);
  s.cams_[1]->AssociateCamereModel(s.cam_models_.back());
  s.cams_[0]->cam_model_->AddCamera(0);
  s.cams_[1]->cam_model_->AddCamera(1);
  Mat3 I; for (int k = 0; k < 9; k++) I.m[k] = (k % 4 == 0) ? 1.0 : 0.0;
  Vec3 zero; for (int k = 0; k < 3; k++) zero[k] = 0.0;
  s.cams_[0]->SetRTPose(I, zero);
  s.cams_[1]->SetRTPose(a.R, a.t);
  for (size_t e = 0; e < a.pt_match.size(); e++) {
    const int f1 = s.graph_.matches[2 * (size_t)(m0 + a.pt_match[e])], f2 = s.graph_.matches[2 * (size_t)(m0 + a.pt_match[e]) + 1];
    Point3D* pt = new Point3D;
    pt->id_ = (int)s.pts_.size();
    const int g1 = f1 + id_img1 * s.options_.idx_max_per_image, g2 = f2 + id_img2 * s.options_.idx_max_per_image;
    pt->AddObservation(s.cams_[0], s.keypoints_[2 * (size_t)(nf_first1 + f1)], s.keypoints_[2 * (size_t)(nf_first1 + f1) + 1], g1);
    pt->AddObservation(s.cams_[1], s.keypoints_[2 * (size_t)(nf_first2 + f2)], s.keypoints_[2 * (size_t)(nf_first2 + f2) + 1], g2);
    for (int k = 0; k < 3; k++) pt->data[k] = a.X[3 * e + k];
    pt->mse_ = a.mse[e];
    s.pts_.push_back(pt);
    s.cams_[0]->AddPoints(pt, g1);
    s.cams_[1]->AddPoints(pt, g2);
  }
  if (s.seed_adjust_) {
    s.FullBundleAdjustment();   // :393
    s.RemovePointOutliers();    // :396
  }
  s.cams_[0]->visible_cams_.push_back(0); s.cams_[0]->visible_cams_.push_back(1);   // :401-408
  s.cams_[1]->visible_cams_.push_back(1); s.cams_[1]->visible_cams_.push_back(0);
  s.is_img_processed_[id_img1] = true; s.is_img_processed_[id_img2] = true;
  s.img_cam_map_.insert(std::make_pair(id_img1, 0));
  s.img_cam_map_.insert(std::make_pair(id_img2, 1));
}

static void seed_check_inputs(const IncrementalSfM& s, const char* who) {
  const size_t n = s.graph_.n_features.size();
  const size_t rows = (size_t)std::accumulate(s.graph_.n_features.begin(), s.graph_.n_features.end(), 0);
  if (!s.store_ || s.keypoints_.size() != 2 * rows || s.image_focal_.size() != n || s.image_model_.size() != n)
    throw std::runtime_error(std::string(who) + ": SetMatches, SetKeypoints, image_focal_ and image_model_ first");
}

bool IncrementalSfM::FindSeedPairThenReconstruct() {
  seed_check_inputs(*this, "FindSeedPairThenReconstruct");
  std::vector<std::pair<int, int>> hyps;
  SortImagePairs(hyps);
  seed_hyps_visited_ = 0;
  msfm_seed_options opt = seed_options_;
  opt.th_mse_reprojection = options_.th_mse_reprojection; opt.th_angle_small = options_.th_angle_small;
  opt.th_seedpair_structures = options_.th_seedpair_structures;
  for (size_t c0 = 0; c0 < hyps.size(); c0 += seed_chunk_) {
    const int n = (int)std::min(hyps.size() - c0, (size_t)seed_chunk_);
    std::vector<int> hyp_img(2 * (size_t)n);
    std::vector<double> cam_fk(6 * (size_t)n, 0.0);
    std::vector<uint8_t> same(n);
    for (int h = 0; h < n; h++) {
      const int i1 = hyps[c0 + h].first, i2 = hyps[c0 + h].second;
      hyp_img[2 * h] = i1; hyp_img[2 * h + 1] = i2;
      cam_fk[6 * h] = image_focal_[i1]; cam_fk[6 * h + 3] = image_focal_[i2];
      same[h] = image_model_[i1] == image_model_[i2];
    }
    msfm_seed_problem P{};
    P.n_hyp = n; P.hyp_img = hyp_img.data(); P.cam_fk = cam_fk.data(); P.same_model = same.data(); P.keypoints = keypoints_.data();
    msfm_seed_set* set = nullptr;
    check(msfm_seed_hypotheses(Context(), store_.get(), &P, &opt, &set), "msfm_seed_hypotheses");
    int n_points = 0, winner = -1;
    msfm_seed_set_size(set, nullptr, &n_points, &winner, nullptr);
    if (winner < 0) { msfm_seed_set_destroy(set); continue; }
    std::vector<double> f(2 * (size_t)n), R(9 * (size_t)n), t(3 * (size_t)n), X(3 * (size_t)std::max(1, n_points)), mse(std::max(1, n_points));
    std::vector<int> pt_off(n + 1), pt_match(std::max(1, n_points));
    msfm_seed_set_fetch(set, nullptr, nullptr, nullptr, nullptr, f.data(), R.data(), t.data(), nullptr, pt_off.data(), pt_match.data(), X.data(),
                        mse.data());
    msfm_seed_set_destroy(set);
    SeedAnswer a;
    a.pass = true;
    a.f[0] = f[2 * winner]; a.f[1] = f[2 * winner + 1];
    for (int k = 0; k < 9; k++) a.R.m[k] = R[9 * (size_t)winner + k];
    for (int k = 0; k < 3; k++) a.t[k] = t[3 * (size_t)winner + k];
    a.pt_match.assign(pt_match.begin() + pt_off[winner], pt_match.begin() + pt_off[winner + 1]);
    a.X.assign(X.begin() + 3 * (size_t)pt_off[winner], X.begin() + 3 * (size_t)pt_off[winner + 1]);
    a.mse.assign(mse.begin() + pt_off[winner], mse.begin() + pt_off[winner + 1]);
    seed_hyps_visited_ = (int)c0 + winner + 1;
    seed_adopt(*this, hyps[c0 + winner].first, hyps[c0 + winner].second, a);
    return true;
  }
  return false;
}

bool IncrementalSfM::FindSeedPairThenReconstructHost() {
  seed_check_inputs(*this, "FindSeedPairThenReconstructHost");
  std::vector<std::pair<int, int>> hyps;
  SortImagePairs(hyps);
  seed_hyps_visited_ = 0;
  std::vector<int> first(graph_.n_features.size() + 1, 0);
  for (size_t i = 0; i < graph_.n_features.size(); i++) first[i + 1] = first[i] + graph_.n_features[i];
  for (size_t i = 0; i < hyps.size(); i++) {
    const int id_img1 = hyps[i].first, id_img2 = hyps[i].second;
    seed_hyps_visited_ = (int)i + 1;
    int m0 = 0, cnt = 0;   // graph_.QueryMatch(id_img1, id_img2, matches), :249
    for (size_t p = 0; p < graph_.pair_img.size() / 2; p++)
      if (graph_.pair_img[2 * p] == id_img1 && graph_.pair_img[2 * p + 1] == id_img2) { m0 = graph_.match_off[p]; cnt = graph_.match_off[p + 1] - m0; }
    // :294-304 - behind h empty problems, so that the pose call draws the samples of problem h = i % seed_chunk_
    const int h = (int)(i % (size_t)seed_chunk_);
    std::vector<int> off(h + 2, 0);
    off[h + 1] = cnt;
    std::vector<double> a(2 * (size_t)std::max(1, cnt)), b(a.size());
    for (int j = 0; j < cnt; j++) {
      const size_t r1 = (size_t)first[id_img1] + graph_.matches[2 * (size_t)(m0 + j)], r2 = (size_t)first[id_img2] + graph_.matches[2 * (size_t)(m0 + j) + 1];
      a[2 * j] = keypoints_[2 * r1]; a[2 * j + 1] = keypoints_[2 * r1 + 1]; b[2 * j] = keypoints_[2 * r2]; b[2 * j + 1] = keypoints_[2 * r2 + 1];
    }
    const size_t m = (size_t)h + 1;
    std::vector<double> E(9 * m), R(9 * m), t(3 * m), f1(m, 0.0), f2(m, 0.0);
    std::vector<uint8_t> ok(m, 0);
    SeedAnswer ans;
    ans.f[0] = image_focal_[id_img1]; ans.f[1] = image_focal_[id_img2];
    if (ans.f[0] && ans.f[1]) {   // :307-315
      f1[h] = ans.f[0]; f2[h] = ans.f[1];
      check(msfm_relpose_5pt_batch(Context(), h + 1, off.data(), a.data(), b.data(), f1.data(), f2.data(), seed_options_.ransac_times_5pt,
                                   seed_options_.seed_5pt, E.data(), R.data(), t.data(), ok.data(), nullptr), "relpose_5pt_batch");
      if (!ok[h]) continue;
    } else {                      // :316-333
      std::vector<double> F(9 * m);
      check(msfm_relpose_8pt_batch(Context(), h + 1, off.data(), a.data(), b.data(), seed_options_.ransac_times_8pt, seed_options_.seed_8pt, F.data(),
                                   f1.data(), f2.data(), E.data(), R.data(), t.data(), ok.data(), nullptr, nullptr, nullptr), "relpose_8pt_batch");
      if (!ok[h]) continue;
      if (image_model_[id_img1] == image_model_[id_img2]) { ans.f[0] = (f1[h] + f2[h]) / 2.0; ans.f[1] = ans.f[0]; }
      else { ans.f[0] = f1[h]; ans.f[1] = f2[h]; }
    }
    for (int k = 0; k < 9; k++) ans.R.m[k] = R[9 * (size_t)h + k];
    for (int k = 0; k < 3; k++) ans.t[k] = t[3 * (size_t)h + k];
    // :344-374: Trianglate2 of every match on two temporary cameras (the batch form of Point3D::Trianglate2, one call)
    Camera cam[2];
    CameraModel model[2];
    Mat3 I; for (int k = 0; k < 9; k++) I.m[k] = (k % 4 == 0) ? 1.0 : 0.0;
    Vec3 zero; for (int k = 0; k < 3; k++) zero[k] = 0.0;
    for (int k = 0; k < 2; k++) { model[k].SetFocalLength(ans.f[k]); cam[k].AssociateCamereModel(&model[k]); cam[k].SetID(k); }
    cam[0].SetRTPose(I, zero);
    cam[1].SetRTPose(ans.R, ans.t);
    std::vector<Point3D> tmp(cnt);
    std::vector<Point3D*> ptrs(cnt);
    for (int j = 0; j < cnt; j++) {
      tmp[j].AddObservation(&cam[0], a[2 * j], a[2 * j + 1], 0);
      tmp[j].AddObservation(&cam[1], b[2 * j], b[2 * j + 1], 1);
      ptrs[j] = &tmp[j];
    }
    std::vector<char> okp;
    if (cnt) TrianglateBatch(ptrs, options_.th_mse_reprojection, options_.th_angle_small, false, &okp);
    for (int j = 0; j < cnt; j++)
      if (okp[j]) {
        ans.pt_match.push_back(j);
        for (int k = 0; k < 3; k++) ans.X.push_back(tmp[j].data[k]);
        ans.mse.push_back(tmp[j].mse_);
      }
    if ((int)ans.pt_match.size() < options_.th_seedpair_structures || (int)ans.pt_match.size() < cnt / 5) continue;   // :380-381
    seed_adopt(*this, id_img1, id_img2, ans);
    return true;
  }
  return false;
}

// ---- IncrementalSfM: which image to localise next -------------------------------------------------
void IncrementalSfM::SetMatches(const std::vector<int>& n_features, const std::vector<int>& pair_img, const std::vector<int>& match_off,
                                const std::vector<int>& matches) {
  const int n = (int)n_features.size(), np = (int)pair_img.size() / 2;
  if ((int)match_off.size() != np + 1 || (np && (int)matches.size() < 2 * match_off[np])) throw std::runtime_error("SetMatches: sizes");
  msfm_match_store* st = nullptr;
  check(msfm_match_store_create(Context(), n, n_features.data(), np, pair_img.data(), match_off.data(), matches.data(), &st),
        "msfm_match_store_create");   // (checks the pair order and every index)
  store_.reset(st, msfm_match_store_destroy);
  graph_.n_features = n_features; graph_.pair_img = pair_img; graph_.match_off = match_off; graph_.matches = matches;
  graph_.match_graph_.assign((size_t)n * n, 0);
  for (int p = 0; p < np; p++) graph_.match_graph_[(size_t)pair_img[2 * p] * n + pair_img[2 * p + 1]] = match_off[p + 1] - match_off[p];
  if (is_img_processed_.empty()) is_img_processed_.assign(n, false);
  if (localize_fail_times_.empty()) localize_fail_times_.assign(n, 0);
}

// sfm_incremental.cc:423-438
static std::vector<int> candidate_images(const IncrementalSfM& s) {
  const int num_imgs = (int)s.graph_.n_features.size();
  std::vector<int> image_ids;
  for (size_t i = 0; i < s.cams_.size(); ++i) {
    const int id_img = s.cams_[i]->id_img_;
    for (int j = 0; j < num_imgs; ++j)
      if (s.graph_.match_graph_[(size_t)id_img * num_imgs + j] > 0 && !s.is_img_processed_[j] &&
          s.localize_fail_times_[j] < s.options_.th_max_failure_localization)
        image_ids.push_back(j);
  }
  std::sort(image_ids.begin(), image_ids.end());   // math::unique_vector
  image_ids.erase(std::unique(image_ids.begin(), image_ids.end()), image_ids.end());
  return image_ids;
}

// The flat state of cams_ / pts_ - camera -> image, (camera, local feature) -> point, what the search reads of a point - and one
// msfm_localize_candidates call for `cand`; with_points: point_xyz and keypoints_ go along, and the set keeps its
// correspondences on the device for msfm_localize_poses.  The set is the caller's.
static msfm_localize_set* localize_search(IncrementalSfM& s, const std::vector<int>& cand, bool with_points) {
  std::vector<int> cam_img(s.cams_.size()), feat_point, fail(cand.size());
  for (size_t c = 0; c < s.cams_.size(); c++) {
    const int img = s.cams_[c]->id_img_, nf = s.graph_.n_features[img];
    cam_img[c] = img;
    const size_t at = feat_point.size();
    feat_point.resize(at + nf, -1);
    for (auto& kv : s.cams_[c]->pts_) {
      const long local = (long)kv.first - (long)s.options_.idx_max_per_image * img;
      if (local < 0 || local >= nf) continue;   // (no match of this image can name it)
      const int id = kv.second->id_;
      if (id < 0 || id >= (int)s.pts_.size() || s.pts_[id] != kv.second) throw std::runtime_error("FindImageToLocalize: pts_[i]->id_ != i");
      feat_point[at + local] = id;
    }
  }
  std::vector<uint8_t> pt_bad(s.pts_.size());
  std::vector<double> pt_mse(s.pts_.size()), xyz;
  std::vector<int> pt_views(s.pts_.size());
  for (size_t i = 0; i < s.pts_.size(); i++) {
    pt_bad[i] = s.pts_[i]->is_bad_estimated_; pt_mse[i] = s.pts_[i]->mse_; pt_views[i] = (int)s.pts_[i]->cams_.size();
  }
  for (size_t k = 0; k < cand.size(); k++) fail[k] = s.localize_fail_times_[cand[k]];
  msfm_localize_problem P{};
  P.n_cams = (int)s.cams_.size(); P.cam_img = cam_img.data(); P.feat_point = feat_point.data();
  P.n_points = (int)s.pts_.size(); P.pt_bad = pt_bad.data(); P.pt_mse = pt_mse.data(); P.pt_views = pt_views.data();
  P.n_cand = (int)cand.size(); P.cand_img = cand.data(); P.fail_times = fail.data();
  if (with_points) {   // :592-600
    xyz.resize(3 * std::max<size_t>(1, s.pts_.size()));
    for (size_t i = 0; i < s.pts_.size(); i++)
      for (int q = 0; q < 3; q++) xyz[3 * i + q] = s.pts_[i]->data[q];
    P.point_xyz = xyz.data(); P.keypoints = s.keypoints_.data();
  }
  msfm_localize_set* set = nullptr;
  check(msfm_localize_candidates(Context(), s.store_.get(), &P, &set), "msfm_localize_candidates");
  return set;
}

void IncrementalSfM::FindImageToLocalize(std::vector<int>& image_ids, std::vector<std::vector<std::pair<int, int>>>& corres_2d3d,
                                         std::vector<std::vector<int>>& visible_cams) {
  image_ids.clear(); corres_2d3d.clear(); visible_cams.clear();
  if (!store_) throw std::runtime_error("FindImageToLocalize: SetMatches first");
  const std::vector<int> cand = candidate_images(*this);
  if (cand.empty()) return;
  msfm_localize_set* set = localize_search(*this, cand, false);
  int n_kept = 0, n_corr = 0, n_vis = 0;
  msfm_localize_set_size(set, &n_kept, &n_corr, &n_vis, nullptr, nullptr);
  std::vector<int> rank(n_kept), coff(n_kept + 1), cf(n_corr), cp(n_corr), voff(n_kept + 1), vc(n_vis);
  msfm_localize_set_fetch(set, rank.data(), coff.data(), cf.data(), cp.data(), voff.data(), vc.data(), nullptr, nullptr);
  msfm_localize_set_destroy(set);
  corres_2d3d.resize(n_kept); visible_cams.resize(n_kept);
  for (int r = 0; r < n_kept; r++) {
    image_ids.push_back(cand[rank[r]]);
    for (int e = coff[r]; e < coff[r + 1]; e++) corres_2d3d[r].push_back(std::make_pair(cf[e], cp[e]));
    visible_cams[r].assign(vc.begin() + voff[r], vc.begin() + voff[r + 1]);
  }
}

void IncrementalSfM::FindImageToLocalizeHost(std::vector<int>& image_ids, std::vector<std::vector<std::pair<int, int>>>& corres_2d3d,
                                             std::vector<std::vector<int>>& visible_cams) const {
  const int num_imgs = (int)graph_.n_features.size();
  image_ids = candidate_images(*this);
  corres_2d3d.clear(); visible_cams.clear();
  if (image_ids.empty()) return;
  // "QueryMatch(i, j)" on the lists in memory: pair index of (i, j)
  std::map<std::pair<int, int>, int> pair_at;
  for (int p = 0; p < (int)graph_.pair_img.size() / 2; p++) pair_at[std::make_pair(graph_.pair_img[2 * p], graph_.pair_img[2 * p + 1])] = p;
  corres_2d3d.resize(image_ids.size());
  visible_cams.resize(image_ids.size());
  for (size_t i = 0; i < image_ids.size(); i++) {
    const int id_img_i = image_ids[i];
    std::vector<int> visible_cams_i;
    std::map<int, int> corres_2d3d_i;        // first, idx of 2d keypoints; second, idx of 3d points
    std::map<int, double> corres_2d3d_info_i;
    for (int id_img_j = 0; id_img_j < num_imgs; ++id_img_j) {
      if (!(graph_.match_graph_[(size_t)id_img_i * num_imgs + id_img_j] > 0 && is_img_processed_[id_img_j])) continue;   // :457
      auto iter_i_c = img_cam_map_.find(id_img_j);
      if (iter_i_c == img_cam_map_.end()) continue;
      const int idx_cam = iter_i_c->second;
      auto pit = pair_at.find(std::make_pair(id_img_i, id_img_j));
      if (pit == pair_at.end()) continue;
      int count_2d3d_ij = 0;
      for (int m = graph_.match_off[pit->second]; m < graph_.match_off[pit->second + 1]; m++) {   // :480
        const int idx_i_local = graph_.matches[2 * (size_t)m], idx_j_local = graph_.matches[2 * (size_t)m + 1];
        const int idx_j_global = idx_j_local + options_.idx_max_per_image * id_img_j;
        auto iter_cam_3dpt = cams_[idx_cam]->pts_.find(idx_j_global);
        if (iter_cam_3dpt != cams_[idx_cam]->pts_.end() && !iter_cam_3dpt->second->is_bad_estimated_) {   // :486-487
          corres_2d3d_i.insert(std::pair<int, int>(idx_i_local, iter_cam_3dpt->second->id_));
          double mse_3dpt = iter_cam_3dpt->second->mse_;
          if (iter_cam_3dpt->second->cams_.size() <= 2) mse_3dpt += 3.0;
          corres_2d3d_info_i.insert(std::pair<int, double>(idx_i_local, mse_3dpt));
          count_2d3d_ij++;
        }
      }
      if (count_2d3d_ij > options_.th_visible_matches) visible_cams_i.push_back(idx_cam);   // :503
    }
    if (corres_2d3d_i.empty()) continue;
    std::vector<std::pair<int, double>> sorted_i(corres_2d3d_info_i.begin(), corres_2d3d_info_i.end());
    std::sort(sorted_i.begin(), sorted_i.end(), [](const std::pair<int, double>& l, const std::pair<int, double>& r) {   // :524 + the ties
      const bool ln = std::isnan(l.second), rn = std::isnan(r.second);
      if (ln != rn) return rn;
      if (!ln && l.second != r.second) return l.second < r.second;
      return l.first < r.first;
    });
    for (auto& e : sorted_i) corres_2d3d[i].push_back(std::pair<int, int>(e.first, corres_2d3d_i[e.first]));
    visible_cams[i] = visible_cams_i;
  }
  // :537-562
  std::vector<std::pair<int, int>> idx_num(image_ids.size());
  for (size_t i = 0; i < image_ids.size(); i++)
    idx_num[i] = std::make_pair((int)i, (int)(corres_2d3d[i].size() / (5 + localize_fail_times_[image_ids[i]])));
  std::stable_sort(idx_num.begin(), idx_num.end(), [](const std::pair<int, int>& l, const std::pair<int, int>& r) { return l.second > r.second; });
  std::vector<int> ids_sort;
  std::vector<std::vector<std::pair<int, int>>> corres_sort;
  std::vector<std::vector<int>> visible_sort;
  for (auto& e : idx_num) {
    if (e.second <= 0) continue;
    ids_sort.push_back(image_ids[e.first]);
    corres_sort.push_back(corres_2d3d[e.first]);
    visible_sort.push_back(visible_cams[e.first]);
  }
  image_ids = ids_sort; corres_2d3d = corres_sort; visible_cams = visible_sort;
}

// ---- IncrementalSfM: the localisation of the next image --------------------------------------------
// CameraAssociateCameraModel as far as image_model_ describes it: the model of a camera whose image shares the value
static CameraModel* model_of_image(const IncrementalSfM& s, int id_img) {
  for (const Camera* c : s.cams_)
    if (s.image_model_[c->id_img_] == s.image_model_[id_img]) return c->cam_model_;
  return nullptr;
}

static void localize_check_inputs(const IncrementalSfM& s, const char* who) {
  seed_check_inputs(s, who);
  for (size_t i = 0; i < s.image_focal_.size(); i++)
    if (s.image_focal_[i] == 0.0 && s.image_focal_init_.size() != s.image_focal_.size())
      throw std::runtime_error(std::string(who) + ": image_focal_init_ for the images without a focal length");
}

// :575-589: the camera of `id_img` on its model (an existing one, or a new one that is not yet in cam_models_)
static Camera* localize_new_camera(const IncrementalSfM& s, int id_img) {
  Camera* cam_new = new Camera;
  cam_new->AssociateImage(id_img);
  CameraModel* model = model_of_image(s, id_img);
  if (!model) model = new CameraModel((int)s.cam_models_.size(), 0, 0, 0.0, s.image_focal_[id_img], "", "");
  cam_new->AssociateCamereModel(model);
  return cam_new;
}

static void localize_drop_camera(Camera* cam) {
  if (cam->cam_model_->num_cams_ == 0) delete cam->cam_model_;
  delete cam;
}

// :733-748
static void localize_register_camera(IncrementalSfM& s, Camera* cam_new, const std::vector<int>& visible_cams) {
  if (cam_new->cam_model_->num_cams_ == 0) s.cam_models_.push_back(cam_new->cam_model_);
  cam_new->SetID((int)s.cams_.size());
  cam_new->cam_model_->AddCamera(cam_new->id_);
  s.cams_.push_back(cam_new);
  s.UpdateVisibleGraph((int)s.cams_.size() - 1, visible_cams);
}

bool IncrementalSfM::LocalizeNextImage() {
  localize_check_inputs(*this, "LocalizeNextImage");
  localize_image_ids_.clear(); localize_failed_.clear(); localize_count_inliers_ = 0;
  const std::vector<int> cand = candidate_images(*this);
  if (cand.empty()) return false;
  std::shared_ptr<msfm_localize_set> set(localize_search(*this, cand, true), msfm_localize_set_destroy);
  int n_kept = 0, n_corr = 0, n_vis = 0;
  msfm_localize_set_size(set.get(), &n_kept, &n_corr, &n_vis, nullptr, nullptr);
  if (n_kept == 0) return false;   // :137
  found_seed_ = true;              // :141
  std::vector<int> rank(n_kept), coff(n_kept + 1), cf(n_corr), cp(n_corr), voff(n_kept + 1), vc(n_vis);
  msfm_localize_set_fetch(set.get(), rank.data(), coff.data(), cf.data(), cp.data(), voff.data(), vc.data(), nullptr, nullptr);
  std::vector<double> row_f(n_kept), row_f_init(n_kept, 0.0);
  for (int r = 0; r < n_kept; r++) {
    const int img = cand[rank[r]];
    localize_image_ids_.push_back(img);
    const CameraModel* model = model_of_image(*this, img);
    row_f[r] = model ? model->f_ : image_focal_[img];   // :644
    if (row_f[r] == 0.0) row_f_init[r] = image_focal_init_[img];
  }
  std::vector<uint8_t> added(std::max<size_t>(1, pts_.size()));
  for (size_t i = 0; i < pts_.size(); i++) added[i] = pts_[i]->is_new_added_;
  msfm_localize_pose_options opt = localize_options_;
  opt.th_mse_localization = options_.th_mse_localization; opt.th_min_2d3d_corres = options_.th_min_2d3d_corres;
  std::vector<uint8_t> tried(n_kept), arm(n_kept), state(std::max(1, n_corr));
  std::vector<double> f(n_kept), R(9 * (size_t)n_kept), t(3 * (size_t)n_kept);
  std::vector<int> n_inliers(n_kept);
  int winner = -1;
  while (opt.first_row >= 0) {   // :146-159, max_tries rows per call
    msfm_localize_pose_set* ps = nullptr;
    check(msfm_localize_poses(Context(), set.get(), row_f.data(), row_f_init.data(), (int)pts_.size(), added.data(), &opt, &ps), "msfm_localize_poses");
    int next_row = -1;
    msfm_localize_pose_set_size(ps, nullptr, nullptr, nullptr, &winner, &next_row);
    msfm_localize_pose_set_fetch(ps, tried.data(), arm.data(), nullptr, f.data(), R.data(), t.data(), nullptr, nullptr, nullptr, n_inliers.data(), nullptr,
                                 nullptr, state.data());
    msfm_localize_pose_set_destroy(ps);
    for (int r = 0; r < n_kept; r++)
      if (tried[r] && (winner < 0 || r < winner)) {   // :650 / :681
        localize_fail_times_[localize_image_ids_[r]]++;
        localize_failed_.push_back(localize_image_ids_[r]);
      }
    if (winner >= 0) break;
    opt.first_row = next_row;
  }
  if (winner < 0) return false;    // :160-164
  const int id_img = localize_image_ids_[winner];
  size_t first = 0;
  for (int i = 0; i < id_img; i++) first += graph_.n_features[i];
  Camera* cam_new = localize_new_camera(*this, id_img);
  if (arm[winner] == 2) cam_new->cam_model_->SetFocalLength(f[winner]);   // :703
  RTPose pose;
  for (int q = 0; q < 9; q++) pose.R.m[q] = R[9 * (size_t)winner + q];
  for (int q = 0; q < 3; q++) pose.t[q] = t[3 * (size_t)winner + q];
  cam_new->SetRTPose(pose.R, pose.t);                                     // :705
  for (int e = coff[winner]; e < coff[winner + 1]; e++) {                 // :709-729 as the call reports it
    Point3D* pt = pts_[cp[e]];
    if (state[e] == 1) { pt->is_bad_estimated_ = true; continue; }
    if ((state[e] == 2) != !pt->is_new_added_) throw std::runtime_error("LocalizeNextImage: corr_state disagrees with is_new_added_");
    if (state[e] != 2) continue;
    const int idx_2d_global = cf[e] + id_img * options_.idx_max_per_image;
    pt->AddObservation(cam_new, keypoints_[2 * (first + cf[e])], keypoints_[2 * (first + cf[e]) + 1], idx_2d_global);
    pt->is_new_added_ = true;
    cam_new->AddPoints(pt, idx_2d_global);
    localize_count_inliers_++;
  }
  if (localize_count_inliers_ != n_inliers[winner]) throw std::runtime_error("LocalizeNextImage: n_inliers disagrees with the walk");
  localize_register_camera(*this, cam_new, std::vector<int>(vc.begin() + voff[winner], vc.begin() + voff[winner + 1]));
  return true;
}

bool IncrementalSfM::LocalizeImage(int id_img, std::vector<std::pair<int, int>>& corres_2d3d, std::vector<int>& visible_cams) {
  if (corres_2d3d.size() < 3) return false;   // :567
  localize_check_inputs(*this, "LocalizeImage");
  size_t first = 0;
  for (int i = 0; i < id_img; i++) first += graph_.n_features[i];
  Camera* cam_new = localize_new_camera(*this, id_img);
  // :592-600, flat, as problem localize_row_ behind empty problems
  const int r = localize_row_, N = (int)corres_2d3d.size();
  std::vector<int> off(r + 2, 0);
  off[r + 1] = N;
  std::vector<double> pts_w(3 * (size_t)N), pts_2d(2 * (size_t)N), fs(r + 1, 1.0), Rr(9 * (size_t)(r + 1)), tr(3 * (size_t)(r + 1)), avg(r + 1),
      error_reproj(N), f_out(r + 1);
  for (int i = 0; i < N; i++) {
    const int idx_2d = corres_2d3d[i].first, idx_3d = corres_2d3d[i].second;
    pts_2d[2 * (size_t)i] = keypoints_[2 * (first + idx_2d)]; pts_2d[2 * (size_t)i + 1] = keypoints_[2 * (first + idx_2d) + 1];
    for (int q = 0; q < 3; q++) pts_w[3 * (size_t)i + q] = pts_[idx_3d]->data[q];
  }
  const bool known = cam_new->cam_model_->f_ != 0.0;   // :644
  if (known) {
    fs[r] = cam_new->cam_model_->f_;
    check(msfm_epnp_ransac_batch(Context(), r + 1, off.data(), pts_w.data(), pts_2d.data(), fs.data(), localize_options_.max_iter,
                                 localize_options_.seed, Rr.data(), tr.data(), error_reproj.data(), avg.data(), nullptr), "epnp_ransac_batch");
  } else {
    fs[r] = image_focal_init_[id_img];                 // :675
    check(msfm_epnpf_sweep_batch(Context(), r + 1, off.data(), pts_w.data(), pts_2d.data(), fs.data(), &localize_options_.sweep, f_out.data(),
                                 Rr.data(), tr.data(), error_reproj.data(), avg.data(), nullptr, nullptr, nullptr), "epnpf_sweep_batch");
  }
  const double avg_error = avg[r];
  if (avg_error > options_.th_mse_localization) {      // :648 / :679
    localize_fail_times_[id_img]++;
    localize_drop_camera(cam_new);
    return false;
  }
  if (!known) cam_new->cam_model_->SetFocalLength(f_out[r]);   // :703
  RTPose pose;
  for (int q = 0; q < 9; q++) pose.R.m[q] = Rr[9 * (size_t)r + q];
  for (int q = 0; q < 3; q++) pose.t[q] = tr[3 * (size_t)r + q];
  cam_new->SetRTPose(pose.R, pose.t);
  int count_inliers = 0;
  for (int i = 0; i < N; i++) {                        // :709-729
    const int idx_3d = corres_2d3d[i].second;
    if (error_reproj[i] > avg_error) { pts_[idx_3d]->is_bad_estimated_ = true; continue; }
    const int idx_2d_local = corres_2d3d[i].first;
    const int idx_2d_global = idx_2d_local + id_img * options_.idx_max_per_image;
    if (!pts_[idx_3d]->is_new_added_) {
      pts_[idx_3d]->AddObservation(cam_new, pts_2d[2 * (size_t)i], pts_2d[2 * (size_t)i + 1], idx_2d_global);
      pts_[idx_3d]->is_new_added_ = true;
      cam_new->AddPoints(pts_[idx_3d], idx_2d_global);
      count_inliers++;
    }
  }
  localize_count_inliers_ = count_inliers;
  localize_register_camera(*this, cam_new, visible_cams);
  return true;
}

// ---- IncrementalSfM: the new points of the image just localised -------------------------------------
// sfm_incremental.cc:755-915.  The flat state of cams_ / pts_ (as FindImageToLocalize gathers it, plus the poses), one
// msfm_new_points call for the newest camera against its visible_cams_, then :899-910 on the answer.
void IncrementalSfM::GenerateNew3DPoints() {
  if (!store_) throw std::runtime_error("GenerateNew3DPoints: SetMatches first");
  if (cams_.empty()) throw std::runtime_error("GenerateNew3DPoints: no camera");
  size_t rows = 0;
  std::vector<size_t> first(graph_.n_features.size() + 1, 0);
  for (size_t i = 0; i < graph_.n_features.size(); i++) { rows += graph_.n_features[i]; first[i + 1] = rows; }
  if (keypoints_.size() != 2 * rows) throw std::runtime_error("GenerateNew3DPoints: SetKeypoints first");
  const int idx_cam_1 = (int)cams_.size() - 1;
  const int id_img_1 = cams_[idx_cam_1]->id_img_;
  std::vector<int> cam_img(cams_.size()), feat_point;
  std::vector<double> R, t, c, fk;
  for (size_t k = 0; k < cams_.size(); k++) {
    const Camera* cm = cams_[k];
    const int img = cm->id_img_, nf = graph_.n_features[img];
    cam_img[k] = img;
    const size_t at = feat_point.size();
    feat_point.resize(at + nf, -1);
    for (auto& kv : cm->pts_) {   // pts_.find(id) != pts_.end(), :804-805: whatever the point's state
      const long local = (long)kv.first - (long)options_.idx_max_per_image * img;
      if (local >= 0 && local < nf) feat_point[at + local] = std::max(0, kv.second->id_);
    }
    for (int q = 0; q < 9; q++) R.push_back(cm->pos_rt_.R.m[q]);
    for (int q = 0; q < 3; q++) { t.push_back(cm->pos_rt_.t[q]); c.push_back(cm->pos_ac_.c[q]); }
    fk.push_back(cm->cam_model_->f_); fk.push_back(cm->cam_model_->k1_); fk.push_back(cm->cam_model_->k2_);
  }
  const std::vector<int>& visible = cams_[idx_cam_1]->visible_cams_;
  const int vis_off[2] = {0, (int)visible.size()};
  msfm_new_points_options o;
  msfm_new_points_default_options(&o);
  o.th_mse_reprojection = options_.th_mse_reprojection; o.th_angle_small = options_.th_angle_small; o.th_angle_large = options_.th_angle_large;
  msfm_new_points_problem P{};
  P.n_cams = (int)cams_.size(); P.cam_img = cam_img.data(); P.feat_point = feat_point.data(); P.n_points = (int)pts_.size();
  P.cam_R = R.data(); P.cam_t = t.data(); P.cam_c = c.data(); P.cam_fk = fk.data();
  P.n_new = 1; P.new_cam = &idx_cam_1; P.vis_off = vis_off; P.vis_cam = visible.data(); P.keypoints = keypoints_.data();
  msfm_new_points_set* set = nullptr;
  check(msfm_new_points(Context(), store_.get(), &P, &o, &set), "msfm_new_points");
  int n = 0;
  msfm_new_points_set_size(set, nullptr, &n, nullptr, nullptr);
  std::vector<int> cam2(n), f1(n), f2(n);
  std::vector<double> X(3 * (size_t)n), mse(n);
  std::vector<uint8_t> takes1(n), takes2(n);
  msfm_new_points_set_fetch(set, nullptr, cam2.data(), f1.data(), f2.data(), nullptr, nullptr, X.data(), mse.data(), takes1.data(), takes2.data(),
                            nullptr, nullptr, nullptr, nullptr);
  msfm_new_points_set_destroy(set);
  for (int i = 0; i < n; i++) {   // :899-910
    const int idx_cam_2 = cam2[i], id_img_2 = cams_[idx_cam_2]->id_img_;
    const int id_pt1_global = f1[i] + id_img_1 * options_.idx_max_per_image, id_pt2_global = f2[i] + id_img_2 * options_.idx_max_per_image;
    const size_t r1 = first[id_img_1] + f1[i], r2 = first[id_img_2] + f2[i];
    Point3D* pt = new Point3D;
    pt->AddObservation(cams_[idx_cam_1], keypoints_[2 * r1], keypoints_[2 * r1 + 1], id_pt1_global);
    pt->AddObservation(cams_[idx_cam_2], keypoints_[2 * r2], keypoints_[2 * r2 + 1], id_pt2_global);
    pt->is_new_added_ = true;
    for (int q = 0; q < 3; q++) pt->data[q] = X[3 * (size_t)i + q];
    pt->mse_ = mse[i];
    pt->id_ = (int)pts_.size();
    pts_.push_back(pt);
    cams_[idx_cam_1]->AddPoints(pt, id_pt1_global);
    cams_[idx_cam_2]->AddPoints(pt, id_pt2_global);
    // the library's claims are these two inserts
    if ((cams_[idx_cam_1]->pts_[id_pt1_global] == pt) != (takes1[i] != 0) || (cams_[idx_cam_2]->pts_[id_pt2_global] == pt) != (takes2[i] != 0))
      throw std::runtime_error("GenerateNew3DPoints: takes1 / takes2 disagree with Camera::AddPoints");
  }
  num_new_points_ = n;
}

// ---- IncrementalSfM: the second half of a round in one call ---------------------------------------
void IncrementalSfM::AdjustRound(int idx_new_cam, bool full) {
  if (!store_) throw std::runtime_error("AdjustRound: SetMatches first");
  if (idx_new_cam < 0 || idx_new_cam >= (int)cams_.size()) throw std::runtime_error("AdjustRound: no such camera");
  if (!cams_gps_.empty()) throw std::runtime_error("AdjustRound: no GPS rows (PartialBundleAdjustment / FullBundleAdjustment attach them)");
  size_t kp_rows = 0;
  for (int v : graph_.n_features) kp_rows += v;
  if (keypoints_.size() != 2 * kp_rows) throw std::runtime_error("AdjustRound: SetKeypoints first");
  const int nc = (int)cams_.size(), nm = (int)cam_models_.size(), np = (int)pts_.size();
  std::map<const Camera*, int> cam_id;
  std::map<const CameraModel*, int> model_id;
  for (int k = 0; k < nc; k++) cam_id[cams_[k]] = k;
  for (int m = 0; m < nm; m++) model_id[cam_models_[m]] = m;
  // the camera side (Camera::pts_) and the solver's parameter blocks
  std::vector<int> cam_img(nc), feat_point, model_of_cam(nc);
  std::vector<double> cam_pose(6 * (size_t)nc), cam_model(3 * (size_t)nm);
  std::vector<uint8_t> model_mut(nm);
  for (int k = 0; k < nc; k++) {
    const Camera* cm = cams_[k];
    const int img = cm->id_img_, nf = graph_.n_features[img];
    cam_img[k] = img;
    const size_t at = feat_point.size();
    feat_point.resize(at + nf, -1);
    for (auto& kv : cm->pts_) {
      const long local = (long)kv.first - (long)options_.idx_max_per_image * img;
      if (local < 0 || local >= nf) throw std::runtime_error("AdjustRound: a key of Camera::pts_ is no feature of its image");
      feat_point[at + local] = kv.second->id_;
    }
    for (int q = 0; q < 6; q++) cam_pose[6 * (size_t)k + q] = cm->data[q];
    model_of_cam[k] = model_id.at(cm->cam_model_);
  }
  for (int m = 0; m < nm; m++) {
    for (int q = 0; q < 3; q++) cam_model[3 * (size_t)m + q] = cam_models_[m]->data[q];
    model_mut[m] = cam_models_[m]->is_mutable_;
  }
  // the point side (Point3D::cams_): one row per observation
  std::vector<int> obs_point, obs_cam, obs_feat;
  std::vector<double> xyz(3 * (size_t)np), mse(np);
  std::vector<uint8_t> bad(np), mut(np), added(np);
  for (int i = 0; i < np; i++) {
    const Point3D* p = pts_[i];
    if (p->id_ != i) throw std::runtime_error("AdjustRound: pts_[i]->id_ != i");
    for (auto& kv : p->cams_) {
      obs_point.push_back(i);
      obs_cam.push_back(cam_id.at(kv.second));
      obs_feat.push_back((int)((long)kv.first - (long)options_.idx_max_per_image * kv.second->id_img_));
    }
    for (int q = 0; q < 3; q++) xyz[3 * (size_t)i + q] = p->data[q];
    mse[i] = p->mse_; bad[i] = p->is_bad_estimated_; mut[i] = p->is_mutable_; added[i] = p->is_new_added_;
  }
  const std::vector<int>& visible = cams_[idx_new_cam]->visible_cams_;
  msfm_round_options o;
  msfm_round_default_options(&o);
  o.partial.max_num_iterations = bundle_partial_options_.max_num_iterations;
  o.partial.progress_to_stdout = bundle_partial_options_.minimizer_progress_to_stdout ? 1 : 0;
  o.partial.num_threads = bundle_partial_options_.num_threads;
  o.full.max_num_iterations = bundle_full_options_.max_num_iterations;
  o.full.progress_to_stdout = bundle_full_options_.minimizer_progress_to_stdout ? 1 : 0;
  o.full.num_threads = bundle_full_options_.num_threads;
  o.th_mse_outliers = options_.th_mse_outliers;
  msfm_round_problem P{};
  P.n_cams = nc; P.cam_img = cam_img.data(); P.feat_point = feat_point.data(); P.n_points = np; P.keypoints = keypoints_.data();
  P.n_obs = (int)obs_point.size(); P.obs_point = obs_point.data(); P.obs_cam = obs_cam.data(); P.obs_feat = obs_feat.data();
  P.cam_pose = cam_pose.data(); P.n_models = nm; P.cam_model = cam_model.data(); P.cam_model_of_cam = model_of_cam.data();
  P.model_mutable = model_mut.data();
  P.point_xyz = xyz.data(); P.pt_bad = bad.data(); P.pt_mse = mse.data(); P.pt_mutable = mut.data(); P.pt_new_added = added.data();
  P.new_cam = idx_new_cam; P.n_visible = (int)visible.size(); P.visible = visible.data();
  P.do_partial = 1; P.do_full = full ? 1 : 0; P.do_outliers = 1;
  msfm_round_set* set = nullptr;
  check(msfm_round_adjust(Context(), store_.get(), &P, &o, &set), "msfm_round_adjust");
  std::vector<double> R(9 * (size_t)nc), t(3 * (size_t)nc), c(3 * (size_t)nc);
  for (int k = 0; k < 2; k++) {
    round_iterations_[k].assign((size_t)std::max(0, k ? o.full.max_num_iterations : o.partial.max_num_iterations) + 2, msfm_ba_iteration());
    round_summary_[k] = msfm_ba_summary();
    round_summary_[k].iterations = round_iterations_[k].data();
    round_summary_[k].iterations_capacity = (int)round_iterations_[k].size();
  }
  msfm_round_set_fetch(set, cam_pose.data(), cam_model.data(), R.data(), t.data(), c.data(), nullptr, xyz.data(), mut.data(), bad.data(), mse.data(),
                       added.data(), nullptr, round_counts_, &round_adjust_[0][0], round_solved_, round_summary_);
  msfm_round_set_destroy(set);
  // BundleAdjuster::UpdateParameters and the flags, as the call reports them
  const int m_new = model_of_cam[idx_new_cam];
  std::vector<uint8_t> cam_free(nc, full ? 1 : 0);
  if (!full) {
    for (int k = 0; k < nc; k++) cam_free[k] = model_of_cam[k] == m_new;
    for (int v : visible) cam_free[v] = 1;
  }
  for (int k = 0; k < nc; k++) {
    Camera* cm = cams_[k];
    for (int q = 0; q < 6; q++) cm->data[q] = cam_pose[6 * (size_t)k + q];
    for (int q = 0; q < 3; q++) { cm->pos_ac_.a[q] = cm->data[q]; cm->pos_rt_.t[q] = t[3 * (size_t)k + q]; cm->pos_ac_.c[q] = c[3 * (size_t)k + q]; }
    for (int q = 0; q < 9; q++) cm->pos_rt_.R.m[q] = R[9 * (size_t)k + q];
    for (int r = 0; r < 3; r++) { for (int q = 0; q < 3; q++) cm->M[4 * r + q] = R[9 * (size_t)k + 3 * r + q]; cm->M[4 * r + 3] = t[3 * (size_t)k + r]; }
    cm->is_mutable_ = cam_free[k] != 0;
  }
  for (int m = 0; m < nm; m++) {
    for (int q = 0; q < 3; q++) cam_models_[m]->data[q] = cam_model[3 * (size_t)m + q];
    cam_models_[m]->UpdataModelFromData();
  }
  for (int i = 0; i < np; i++) {
    Point3D* p = pts_[i];
    for (int q = 0; q < 3; q++) p->data[q] = xyz[3 * (size_t)i + q];
    p->mse_ = mse[i]; p->is_bad_estimated_ = bad[i] != 0; p->is_mutable_ = mut[i] != 0; p->is_new_added_ = added[i] != 0;
  }
  const int last = full && round_solved_[1] ? 1 : 0;   // summary_: of the last adjustment
  iterations_ = round_iterations_[last];
  summary_ = round_summary_[last];
  summary_.iterations = iterations_.data();
}

// The same function as the reference writes it, over the matches and keypoints in memory.
void IncrementalSfM::GenerateNew3DPointsHost() {
  if (cams_.empty()) throw std::runtime_error("GenerateNew3DPointsHost: no camera");
  std::vector<size_t> first(graph_.n_features.size() + 1, 0);
  for (size_t i = 0; i < graph_.n_features.size(); i++) first[i + 1] = first[i] + graph_.n_features[i];
  if (keypoints_.size() != 2 * first.back()) throw std::runtime_error("GenerateNew3DPointsHost: SetKeypoints first");
  std::map<std::pair<int, int>, int> pair_at;   // "QueryMatch(i, j)" on the lists in memory
  for (int p = 0; p < (int)graph_.pair_img.size() / 2; p++) pair_at[std::make_pair(graph_.pair_img[2 * p], graph_.pair_img[2 * p + 1])] = p;
  struct Point3DNew { Point3D* pt; int id_cam1, id_cam2, id_pt1, id_pt2; };
  const int idx_cam_1 = (int)cams_.size() - 1;
  const int id_img_1 = cams_[idx_cam_1]->id_img_;
  std::vector<std::pair<Point3DNew, int>> pts_new;
  for (size_t i = 0; i < cams_[idx_cam_1]->visible_cams_.size(); i++) {
    const int idx_cam_2 = cams_[idx_cam_1]->visible_cams_[i];
    if (idx_cam_2 == idx_cam_1) continue;
    const int id_img_2 = cams_[idx_cam_2]->id_img_;
    auto pit = pair_at.find(std::make_pair(id_img_1, id_img_2));
    if (pit == pair_at.end()) continue;
    const int m0 = graph_.match_off[pit->second], cnt = graph_.match_off[pit->second + 1] - m0;
    double th_tri_angle = options_.th_angle_small;   // :780-784
    if (cnt > 500) th_tri_angle = options_.th_angle_large;
    for (int j = 0; j < cnt; j++) {
      const int id_pt1_local = graph_.matches[2 * (size_t)(m0 + j)], id_pt2_local = graph_.matches[2 * (size_t)(m0 + j) + 1];
      const int id_pt1_global = id_pt1_local + id_img_1 * options_.idx_max_per_image;
      const int id_pt2_global = id_pt2_local + id_img_2 * options_.idx_max_per_image;
      if (cams_[idx_cam_1]->pts_.find(id_pt1_global) != cams_[idx_cam_1]->pts_.end() ||
          cams_[idx_cam_2]->pts_.find(id_pt2_global) != cams_[idx_cam_2]->pts_.end())
        continue;
      const size_t r1 = first[id_img_1] + id_pt1_local, r2 = first[id_img_2] + id_pt2_local;
      Point3D* pt_temp = new Point3D;
      pt_temp->AddObservation(cams_[idx_cam_1], keypoints_[2 * r1], keypoints_[2 * r1 + 1], id_pt1_global);
      pt_temp->AddObservation(cams_[idx_cam_2], keypoints_[2 * r2], keypoints_[2 * r2 + 1], id_pt2_global);
      pt_temp->is_new_added_ = true;
      if (pt_temp->Trianglate2(options_.th_mse_reprojection, th_tri_angle))   // :821, one call per candidate
        pts_new.push_back(std::make_pair(Point3DNew{pt_temp, idx_cam_1, idx_cam_2, id_pt1_global, id_pt2_global}, (int)pt_temp->mse_));   // :829
      else
        delete pt_temp;
    }
  }
  // :897 - std::sort leaves ties open; here, as in msfm_new_points, they keep the order of the walk
  std::stable_sort(pts_new.begin(), pts_new.end(),
                   [](const std::pair<Point3DNew, int>& lhs, const std::pair<Point3DNew, int>& rhs) { return lhs.second < rhs.second; });
  for (size_t i = 0; i < pts_new.size(); i++) {
    const Point3DNew& p = pts_new[i].first;
    p.pt->id_ = (int)pts_.size();
    pts_.push_back(p.pt);
    cams_[p.id_cam1]->AddPoints(p.pt, p.id_pt1);
    cams_[p.id_cam2]->AddPoints(p.pt, p.id_pt2);
  }
  num_new_points_ = (int)pts_new.size();
}

void SLAMGPS::FullBundleAdjustment() {
  // slam_gps.cc:690-712 adds ReprojectionErrorPoseCamXYZ for every observation of every non-bad point with the point's
  // own weight: everything is free, and the weight rule of BundleAdjuster does not apply
  for (Camera* c : cams_) c->SetMutable(true);
  for (CameraModel* m : cam_models_) m->is_mutable_ = true;
  std::vector<double> keep;
  for (Point3D* p : pts_) { p->SetMutable(true); keep.push_back(p->weight); }
  BundleAdjuster bundler(cams_, cam_models_, pts_);
  BundleAdjustOptions o;
  o.max_num_iterations = 200; o.minimizer_progress_to_stdout = minimizer_progress_to_stdout_; o.num_threads = 8;   // slam_gps.cc:681-683
  bundler.SetOptions(o);
  bundler.SetGPS(cams_gps_);
  bundler.keep_point_weights_ = true;
  bundler.RunOptimizetion(false, 1.0);
  for (size_t i = 0; i < pts_.size(); i++) pts_[i]->weight = keep[i];
  bundler.UpdateParameters();   // slam_gps.cc:844-852
  summary_ = bundler.summary_;
  iterations_ = bundler.iterations_;
  summary_.iterations = iterations_.data();
}

// ---- matching -----------------------------------------------------------------------------------
std::vector<PairMatches> MatchImagePairs(const std::vector<std::vector<float>>& descriptors,
                                         const std::vector<std::pair<int, int>>& pairs, float thRatio_good, float thRatio_all) {
  if (g_multi) {
    // the pair list split over the contexts inside the library (fine_matching_graph.cc:87: the pairs are independent)
    const int n_img = (int)descriptors.size();
    std::vector<const float*> dp(n_img);
    std::vector<int> cnt(n_img), flat;
    for (int i = 0; i < n_img; i++) { dp[i] = descriptors[i].data(); cnt[i] = (int)(descriptors[i].size() / 128); }
    for (auto& p : pairs) { flat.push_back(p.first); flat.push_back(p.second); }
    std::vector<std::vector<int32_t>> codes(pairs.size());
    std::vector<int32_t*> cp(pairs.size());
    for (size_t p = 0; p < pairs.size(); p++) { codes[p].assign((size_t)std::max(1, cnt[pairs[p].second]), -1); cp[p] = codes[p].data(); }
    check_multi(msfm_multi_match_pairs(g_multi, n_img, dp.data(), cnt.data(), 128, flat.data(), (int)pairs.size(), thRatio_good, thRatio_all, cp.data(),
                                       nullptr, nullptr), "multi_match_pairs");
    std::vector<PairMatches> out(pairs.size());
    for (size_t p = 0; p < pairs.size(); p++) {
      out[p].idx1 = pairs[p].first; out[p].idx2 = pairs[p].second;
      for (int m = 0; m < cnt[pairs[p].second]; m++) {
        const int32_t code = codes[p][m];
        if (code < 0) continue;
        const int id1 = code & MSFM_MATCH_ID_MASK;
        if (code & MSFM_MATCH_GOOD) out[p].matches_good.push_back(std::make_pair(id1, m));
        if (!(code & MSFM_MATCH_NOT_ALL)) out[p].matches_all.push_back(std::make_pair(id1, m));
      }
    }
    return out;
  }
  msfm_descset* set = nullptr;
  check(msfm_descset_create(Context(), (int)descriptors.size(), 128, &set), "descset_create");
  for (size_t i = 0; i < descriptors.size(); i++)
    check(msfm_descset_upload(set, (int)i, descriptors[i].data(), (int)(descriptors[i].size() / 128)), "descset_upload");
  std::vector<int> flat;
  for (auto& p : pairs) { flat.push_back(p.first); flat.push_back(p.second); }
  msfm_match_result* res = nullptr;
  check(msfm_match_pairs(set, flat.data(), (int)pairs.size(), thRatio_good, thRatio_all, 0, &res), "match_pairs");
  std::vector<PairMatches> out(pairs.size());
  for (size_t p = 0; p < pairs.size(); p++) {
    out[p].idx1 = pairs[p].first; out[p].idx2 = pairs[p].second;
    const int n2 = (int)(descriptors[pairs[p].second].size() / 128);
    std::vector<int32_t> code((size_t)std::max(1, n2));
    check(msfm_match_result_fetch(res, (int)p, code.data(), nullptr, nullptr), "match_fetch");
    for (int m = 0; m < n2; m++) {  // the loop of fine_matching_graph.cc:116-133, decisions already made on the GPU
      if (code[m] < 0) continue;
      const int id1 = code[m] & MSFM_MATCH_ID_MASK;
      if (code[m] & MSFM_MATCH_GOOD) out[p].matches_good.push_back(std::make_pair(id1, m));
      if (!(code[m] & MSFM_MATCH_NOT_ALL)) out[p].matches_all.push_back(std::make_pair(id1, m));
    }
  }
  msfm_match_result_destroy(res);
  msfm_descset_destroy(set);
  return out;
}

// ---- geometric verification ----------------------------------------------------------------------
static void flatten(const std::vector<Point2f>& v, std::vector<float>& out) {
  out.resize(2 * v.size());
  for (size_t i = 0; i < v.size(); i++) { out[2 * i] = v[i].x; out[2 * i + 1] = v[i].y; }
}

bool GeoVerification::GeoVerificationFundamental(std::vector<Point2f>& pt1, std::vector<Point2f>& pt2, std::vector<int>& match_inliers,
                                                 Mat3& FMatrix) {
  if (pt1.size() < 30) return false;
  std::vector<float> a, b;
  flatten(pt1, a); flatten(pt2, b);
  const int off[2] = {0, (int)pt1.size()};
  msfm_fransac_options o;
  msfm_fransac_default_options(&o);
  std::vector<uint8_t> status(pt1.size());
  int nin = 0;
  uint8_t ok = 0;
  check(msfm_fundamental_ransac_batch(Context(), 1, off, a.data(), b.data(), &o, FMatrix.m, status.data(), &nin, &ok), "fundamental_ransac");
  for (size_t i = 0; i < status.size(); i++) if (status[i]) match_inliers.push_back((int)i);
  return match_inliers.size() >= 30;
}

bool GeoVerification::GeoVerificationFundamental(std::vector<Point2f>& pt1, std::vector<Point2f>& pt2, Mat3 FMatrix,
                                                 std::vector<int>& match_inliers) {
  match_inliers.clear();
  if (pt1.empty()) return true;
  std::vector<float> a, b;
  flatten(pt1, a); flatten(pt2, b);
  std::vector<uint8_t> in(pt1.size());
  check(msfm_epipolar_filter(Context(), a.data(), b.data(), (int)pt1.size(), FMatrix.m, 3.0, in.data()), "epipolar_filter");
  for (size_t i = 0; i < in.size(); i++) if (in[i]) match_inliers.push_back((int)i);
  return true;
}

// ---- which pairs to match (initial_matching_graph.cc:164-294) ----
namespace math {
// basic_funcs.h:127-152: the first group is never unique (its first element is compared with itself), the last never pushed
static std::vector<int> keep_unique_vector(std::vector<int> data) {
  std::vector<int> kept;
  std::sort(data.begin(), data.end());
  int v = data[0];
  bool is_unique = true;
  for (int x : data) {
    if (x != v) {
      if (is_unique) kept.push_back(v);
      v = x;
      is_unique = true;
    } else {
      is_unique = false;
    }
  }
  return kept;
}
// basic_funcs.cc:380-408: the index that opens a group, when the group before it was unique
static std::vector<int> keep_unique_idx_vector(const std::vector<int>& data) {
  std::vector<std::pair<int, int>> by_word(data.size());
  for (size_t i = 0; i < data.size(); i++) by_word[i] = {(int)i, data[i]};
  std::stable_sort(by_word.begin(), by_word.end(), [](const std::pair<int, int>& a, const std::pair<int, int>& b) { return a.second < b.second; });
  std::vector<int> unique_idx;
  bool is_unique = true;
  int v = by_word[0].second;
  for (const auto& e : by_word) {
    if (e.second != v) {
      if (is_unique) unique_idx.push_back(e.first);
      v = e.second;
      is_unique = true;
    } else {
      is_unique = false;
    }
  }
  return unique_idx;
}
}  // namespace math

void InitialMatchingGraph::Reset(int n, int K) {
  match_graph_init.assign(n, {});
  hyp_img_.assign(n, std::vector<int>(K, 0));
  n_init_.assign(n, std::vector<int>(K, 0));
  n_inliers_.assign(n, std::vector<int>(K, 0));
  verdict_.assign(n, std::vector<uint8_t>(K, 0));
}

static int ThNumMatch(int num_imgs, int max_hypotheses) {   // :168-169
  if (max_hypotheses > 0) return max_hypotheses;
  int k = std::min(std::max(200, num_imgs / 10), num_imgs - 1);
  return k > 500 ? 500 : k;
}

void InitialMatchingGraph::BuildInitialMatchGraphFeature(const std::vector<std::vector<int>>& words, int num_words,
                                                         const std::vector<std::vector<Point2f>>& keypoints) {
  const int n = (int)words.size();
  std::vector<int> n_features(n), flat_words;
  std::vector<uint8_t> has_words(n);
  std::vector<float> kp;
  for (int i = 0; i < n; i++) {
    n_features[i] = (int)keypoints[i].size();
    has_words[i] = words[i].empty() ? 0 : 1;
    if (has_words[i] && words[i].size() != keypoints[i].size()) throw std::runtime_error("BuildInitialMatchGraphFeature: one word per feature");
    for (int f = 0; f < n_features[i]; f++) {
      flat_words.push_back(has_words[i] ? words[i][f] : 0);
      kp.push_back(keypoints[i][f].x); kp.push_back(keypoints[i][f].y);
    }
  }
  msfm_wordset* ws = nullptr;
  check(msfm_wordset_create(Context(), n, n_features.data(), has_words.data(), flat_words.data(), num_words, kp.data(), max_hypotheses_, &ws),
        "msfm_wordset_create");
  int K = 0;
  msfm_wordset_size(ws, nullptr, &K, nullptr, nullptr, nullptr);
  Reset(n, K);
  std::vector<int> hyp((size_t)n * K);
  int rc = msfm_wordset_fetch(ws, nullptr, hyp.data(), nullptr, nullptr, nullptr, nullptr);
  for (int i = 0; i < n && rc == MSFM_OK; i++) std::copy(hyp.begin() + (size_t)i * K, hyp.begin() + (size_t)(i + 1) * K, hyp_img_[i].begin());
  msfm_pair_select_options opt;
  msfm_pair_select_default_options(&opt);
  for (int r0 = 0; r0 < n && rc == MSFM_OK; r0 += rows_per_call_) {
    const int rows = std::min(rows_per_call_, n - r0);
    msfm_pair_set* ps = nullptr;
    rc = msfm_pair_select(ws, r0, rows, &opt, &ps);
    if (rc != MSFM_OK) break;
    std::vector<int> ni((size_t)rows * K), nin((size_t)rows * K);
    std::vector<uint8_t> ver((size_t)rows * K);
    msfm_pair_set_fetch(ps, ni.data(), nin.data(), ver.data(), nullptr, nullptr, nullptr, nullptr, nullptr);
    msfm_pair_set_destroy(ps);
    for (int r = 0; r < rows; r++)
      for (int s = 0; s < K; s++) {
        const size_t h = (size_t)r * K + s;
        n_init_[r0 + r][s] = ni[h]; n_inliers_[r0 + r][s] = nin[h]; verdict_[r0 + r][s] = ver[h];
        if (ver[h] == 0) match_graph_init[r0 + r].push_back(hyp_img_[r0 + r][s]);   // :280-284
      }
  }
  const std::string err = rc == MSFM_OK ? "" : msfm_last_error(Context());
  msfm_wordset_destroy(ws);
  if (rc != MSFM_OK) throw std::runtime_error("BuildInitialMatchGraphFeature: " + err);
}

void InitialMatchingGraph::MatchGraphFeatureHost(const std::vector<std::vector<int>>& words, int num_words,
                                                 const std::vector<std::vector<Point2f>>& keypoints) {
  const int num_imgs = (int)words.size();
  const int th_num_match = ThNumMatch(num_imgs, max_hypotheses_);
  Reset(num_imgs, th_num_match);
  // similarity_graph.cc:88-117, :63-81
  std::vector<std::vector<int>> inverted_file(num_words);
  for (int i = 0; i < num_imgs; i++)
    if (!words[i].empty())
      for (int id : math::keep_unique_vector(words[i])) inverted_file[id].push_back(i);
  const size_t th_bin_size = (size_t)(num_words / 100);
  for (auto& bin : inverted_file)
    if (!bin.empty() && bin.size() > th_bin_size) bin.clear();
  std::vector<std::vector<int>> similarity_matrix(num_imgs, std::vector<int>(num_imgs, 0));
  for (const auto& bin : inverted_file)
    for (size_t m = 0; m + 1 < bin.size(); m++)
      for (size_t k = m + 1; k < bin.size(); k++) { similarity_matrix[bin[m]][bin[k]]++; similarity_matrix[bin[k]][bin[m]]++; }
  // :188-203
  std::vector<std::map<int, int>> pt_word_map(num_imgs);
  for (int i = 0; i < num_imgs; i++) {
    if (words[i].empty()) continue;
    for (int idx : math::keep_unique_idx_vector(words[i])) pt_word_map[i].insert({words[i][idx], idx});
  }
  msfm_fransac_options fo;
  msfm_fransac_default_options(&fo);
  for (int r0 = 0; r0 < num_imgs; r0 += rows_per_call_) {
    const int rows = std::min(rows_per_call_, num_imgs - r0);
    std::vector<int> off(1, 0);
    std::vector<float> a, b;
    for (int idx1 = r0; idx1 < r0 + rows; idx1++) {
      // :216-231
      std::vector<std::pair<int, int>> sim_sort;
      for (int j = 0; j < num_imgs; j++)
        if (j != idx1) sim_sort.push_back({j, similarity_matrix[idx1][j]});
      std::stable_sort(sim_sort.begin(), sim_sort.end(), [](const std::pair<int, int>& x, const std::pair<int, int>& y) { return x.second > y.second; });
      for (int j = 0; j < th_num_match; j++) {
        const int idx2 = sim_sort[j].first;
        hyp_img_[idx1][j] = idx2;
        // :242-253
        int n_matches = 0;
        for (const auto& it1 : pt_word_map[idx1]) {
          const auto it2 = pt_word_map[idx2].find(it1.first);
          if (it2 == pt_word_map[idx2].end()) continue;
          const Point2f &p = keypoints[idx1][it1.second], &q = keypoints[idx2][it2->second];
          a.push_back(p.x); a.push_back(p.y); b.push_back(q.x); b.push_back(q.y);
          n_matches++;
        }
        n_init_[idx1][j] = n_matches;
        off.push_back(off.back() + n_matches);
      }
    }
    const int H = rows * th_num_match;
    std::vector<double> F(9 * (size_t)H);
    std::vector<uint8_t> inlier(std::max<size_t>(1, a.size() / 2)), ok(H);
    std::vector<int> nin(H);
    check(msfm_fundamental_ransac_batch(Context(), H, off.data(), a.data(), b.data(), &fo, F.data(), inlier.data(), nin.data(), ok.data()),
          "fundamental_ransac");
    for (int r = 0; r < rows; r++)
      for (int s = 0; s < th_num_match; s++) {
        const int h = r * th_num_match + s, i = r0 + r;
        n_inliers_[i][s] = nin[h];
        verdict_[i][s] = n_init_[i][s] < 30 ? 1 : !ok[h] ? 2 : !(nin[h] > 20) ? 3 : 0;   // :254, :270, :274
        if (verdict_[i][s] == 0) match_graph_init[i].push_back(hyp_img_[i][s]);
      }
  }
}

// ---- pose initialisers ----
static const uint64_t kPoseSeed = 0x4D53464D50ull;

void AbsolutePoseBatch(const std::vector<std::vector<Vec3>>& pts_w, const std::vector<std::vector<Vec2>>& pts_2d, const std::vector<double>& f,
                       std::vector<RTPose>& poses, std::vector<std::vector<double>>& errors, std::vector<double>& avg_error) {
  const int n = (int)pts_w.size();
  std::vector<int> off(n + 1, 0);
  for (int p = 0; p < n; p++) off[p + 1] = off[p] + (int)pts_w[p].size();
  std::vector<double> X(3 * (size_t)std::max(1, off[n])), x(2 * (size_t)std::max(1, off[n])), R(9 * (size_t)std::max(1, n)),
      t(3 * (size_t)std::max(1, n)), err(std::max(1, off[n]));
  for (int p = 0; p < n; p++)
    for (size_t i = 0; i < pts_w[p].size(); i++) {
      const size_t e = off[p] + i;
      for (int k = 0; k < 3; k++) X[3 * e + k] = pts_w[p][i][k];
      x[2 * e] = pts_2d[p][i].x; x[2 * e + 1] = pts_2d[p][i].y;
    }
  avg_error.assign(std::max(1, n), 0.0);
  check(msfm_epnp_ransac_batch(Context(), n, off.data(), X.data(), x.data(), f.data(), 200, kPoseSeed, R.data(), t.data(), err.data(),
                               avg_error.data(), nullptr), "epnp_ransac_batch");
  avg_error.resize(n);
  poses.resize(n); errors.resize(n);
  for (int p = 0; p < n; p++) {
    for (int k = 0; k < 9; k++) poses[p].R.m[k] = R[9 * (size_t)p + k];
    for (int k = 0; k < 3; k++) poses[p].t[k] = t[3 * (size_t)p + k];
    errors[p].assign(err.begin() + off[p], err.begin() + off[p + 1]);
  }
}

// AbsolutePoseEstimation::AbsolutePoseWithoutFocalLength (absolute_pose_estimation.cc:28-40) for many images: the EPNPF sweep
// over (0.5 + 0.01 i) * f_estimated, i < 350, 200 samples each (absolute_pose_via_epnpf.cc:34-63), then Error at the kept focal
// length.  f_out[p] is what the caller hands to SetFocalLength once avg_error passes th_mse_localization (sfm_incremental.cc:673-704).
void AbsolutePoseWithoutFocalLengthBatch(const std::vector<std::vector<Vec3>>& pts_w, const std::vector<std::vector<Vec2>>& pts_2d,
                                         const std::vector<double>& f_estimated, std::vector<double>& f_out, std::vector<RTPose>& poses,
                                         std::vector<std::vector<double>>& errors, std::vector<double>& avg_error) {
  const int n = (int)pts_w.size();
  std::vector<int> off(n + 1, 0);
  for (int p = 0; p < n; p++) off[p + 1] = off[p] + (int)pts_w[p].size();
  std::vector<double> X(3 * (size_t)std::max(1, off[n])), x(2 * (size_t)std::max(1, off[n])), R(9 * (size_t)std::max(1, n)),
      t(3 * (size_t)std::max(1, n)), err(std::max(1, off[n]));
  for (int p = 0; p < n; p++)
    for (size_t i = 0; i < pts_w[p].size(); i++) {
      const size_t e = off[p] + i;
      for (int k = 0; k < 3; k++) X[3 * e + k] = pts_w[p][i][k];
      x[2 * e] = pts_2d[p][i].x; x[2 * e + 1] = pts_2d[p][i].y;
    }
  msfm_epnpf_options opt;
  msfm_epnpf_default_options(&opt);
  opt.seed = kPoseSeed;
  avg_error.assign(std::max(1, n), 0.0);
  f_out.assign(std::max(1, n), 0.0);
  check(msfm_epnpf_sweep_batch(Context(), n, off.data(), X.data(), x.data(), f_estimated.data(), &opt, f_out.data(), R.data(), t.data(),
                               err.data(), avg_error.data(), nullptr, nullptr, nullptr), "epnpf_sweep_batch");
  avg_error.resize(n); f_out.resize(n);
  poses.resize(n); errors.resize(n);
  for (int p = 0; p < n; p++) {
    for (int k = 0; k < 9; k++) poses[p].R.m[k] = R[9 * (size_t)p + k];
    for (int k = 0; k < 3; k++) poses[p].t[k] = t[3 * (size_t)p + k];
    errors[p].assign(err.begin() + off[p], err.begin() + off[p + 1]);
  }
}

bool AbsolutePoseEstimation::AbsolutePoseWithFocalLength(std::vector<Vec3>& pts_w, std::vector<Vec2>& pts_2d, double f, RTPose& pose_absolute,
                                                         std::vector<double>& errors, double& avg_error) {
  std::vector<RTPose> poses;
  std::vector<std::vector<double>> errs;
  std::vector<double> avg;
  AbsolutePoseBatch({pts_w}, {pts_2d}, {f}, poses, errs, avg);
  pose_absolute = poses[0];
  errors = errs[0];
  avg_error = avg[0];
  return true;  // the reference always returns true; the caller gates on avg_error (sfm_incremental.cc:648)
}

bool RelativePoseEstimation::RelativePoseWithFocalLength(std::vector<Vec2>& pts_ref, std::vector<Vec2>& pts_cur, double f_ref, double f_cur,
                                                         RTPoseRelative& pose_relative) {
  const int off[2] = {0, (int)pts_cur.size()};
  std::vector<double> a(2 * (size_t)std::max(1, off[1])), b(a.size());
  for (int i = 0; i < off[1]; i++) { a[2 * i] = pts_ref[i].x; a[2 * i + 1] = pts_ref[i].y; b[2 * i] = pts_cur[i].x; b[2 * i + 1] = pts_cur[i].y; }
  double E[9], R[9], t[3];
  uint8_t ok = 0;
  check(msfm_relpose_5pt_batch(Context(), 1, off, a.data(), b.data(), &f_ref, &f_cur, 100, kPoseSeed, E, R, t, &ok, nullptr), "relpose_5pt_batch");
  if (!ok) return false;
  for (int k = 0; k < 9; k++) pose_relative.R.m[k] = R[k];
  for (int k = 0; k < 3; k++) pose_relative.t[k] = t[k];
  return true;
}

// RelativePoseEstimation::RelativePoseWithoutFocalLength (relative_pose_estimation.cc:29-83) for several pairs: 200 samples of
// 8 matches each (fundamental_matrix_eight_point.cc:52), focal lengths and pose from the kept F.
void RelativePoseWithoutFocalLengthBatch(const std::vector<std::vector<Vec2>>& pts_ref, const std::vector<std::vector<Vec2>>& pts_cur,
                                         std::vector<double>& f_ref, std::vector<double>& f_cur, std::vector<RTPoseRelative>& poses,
                                         std::vector<uint8_t>& ok) {
  const int n = (int)pts_cur.size();
  std::vector<int> off(n + 1, 0);
  for (int p = 0; p < n; p++) off[p + 1] = off[p] + (int)pts_cur[p].size();
  const size_t m = (size_t)std::max(1, n);
  std::vector<double> a(2 * (size_t)std::max(1, off[n])), b(a.size()), F(9 * m), E(9 * m), R(9 * m), t(3 * m);
  for (int p = 0; p < n; p++)
    for (size_t i = 0; i < pts_cur[p].size(); i++) {
      const size_t e = off[p] + i;
      a[2 * e] = pts_ref[p][i].x; a[2 * e + 1] = pts_ref[p][i].y; b[2 * e] = pts_cur[p][i].x; b[2 * e + 1] = pts_cur[p][i].y;
    }
  f_ref.assign(m, 0.0); f_cur.assign(m, 0.0); ok.assign(m, 0);
  check(msfm_relpose_8pt_batch(Context(), n, off.data(), a.data(), b.data(), 200, kPoseSeed, F.data(), f_ref.data(), f_cur.data(), E.data(),
                               R.data(), t.data(), ok.data(), nullptr, nullptr, nullptr), "relpose_8pt_batch");
  f_ref.resize(n); f_cur.resize(n); ok.resize(n);
  poses.resize(n);
  for (int p = 0; p < n; p++) {
    for (int k = 0; k < 9; k++) poses[p].R.m[k] = R[9 * (size_t)p + k];
    for (int k = 0; k < 3; k++) poses[p].t[k] = t[3 * (size_t)p + k];
  }
}

bool RelativePoseEstimation::RelativePoseWithoutFocalLength(std::vector<Vec2>& pts_ref, std::vector<Vec2>& pts_cur, double& f_ref,
                                                            double& f_cur, RTPoseRelative& pose_relative) {
  std::vector<double> f1, f2;
  std::vector<RTPoseRelative> poses;
  std::vector<uint8_t> ok;
  RelativePoseWithoutFocalLengthBatch({pts_ref}, {pts_cur}, f1, f2, poses, ok);
  if (!ok[0]) return false;  // f_ref, f_cur and the pose stay as they were, as in the reference
  f_ref = f1[0];
  f_cur = f2[0];
  pose_relative = poses[0];
  return true;
}

std::vector<std::vector<std::pair<int, int>>> VerifyPairs(const std::vector<PairMatches>& matches,
                                                          const std::vector<std::vector<Point2f>>& keypoints) {
  const int np = (int)matches.size();
  std::vector<int> off_g(np + 1, 0), off_a(np + 1, 0);
  for (int p = 0; p < np; p++) {
    off_g[p + 1] = off_g[p] + (int)matches[p].matches_good.size();
    off_a[p + 1] = off_a[p] + (int)matches[p].matches_all.size();
  }
  std::vector<float> g1(2 * (size_t)off_g[np]), g2(g1.size()), a1(2 * (size_t)off_a[np]), a2(a1.size());
  for (int p = 0; p < np; p++) {
    const auto& k1 = keypoints[matches[p].idx1];
    const auto& k2 = keypoints[matches[p].idx2];
    size_t e = off_g[p];
    for (auto& m : matches[p].matches_good) { g1[2 * e] = k1[m.first].x; g1[2 * e + 1] = k1[m.first].y; g2[2 * e] = k2[m.second].x; g2[2 * e + 1] = k2[m.second].y; e++; }
    e = off_a[p];
    for (auto& m : matches[p].matches_all) { a1[2 * e] = k1[m.first].x; a1[2 * e + 1] = k1[m.first].y; a2[2 * e] = k2[m.second].x; a2[2 * e + 1] = k2[m.second].y; e++; }
  }
  msfm_fransac_options o;
  msfm_fransac_default_options(&o);
  std::vector<double> F(9 * (size_t)std::max(1, np));
  std::vector<uint8_t> in_g(std::max(1, off_g[np])), ok(std::max(1, np)), in_a(std::max(1, off_a[np]));
  std::vector<int> nin(std::max(1, np));
  check(msfm_fundamental_ransac_batch(Context(), np, off_g.data(), g1.data(), g2.data(), &o, F.data(), in_g.data(), nin.data(), ok.data()),
        "fundamental_ransac_batch");
  check(msfm_epipolar_filter_batch(Context(), np, off_a.data(), a1.data(), a2.data(), F.data(), ok.data(), 3.0, in_a.data()),
        "epipolar_filter_batch");
  std::vector<std::vector<std::pair<int, int>>> out(np);
  for (int p = 0; p < np; p++) {
    if (!ok[p]) continue;  // isOK == false: the pair writes nothing (fine_matching_graph.cc:182-186)
    for (int e = off_a[p]; e < off_a[p + 1]; e++)
      if (in_a[e]) out[p].push_back(matches[p].matches_all[e - off_a[p]]);
  }
  return out;
}

// ---- feature files ---------------------------------------------------------------------------------
bool WriteoutImageFeature(const std::string& fold, int idx, const ImageInfo& info, const std::vector<Point2f>& kp,
                          const std::vector<float>& desc, int desc_cols) {
  std::ofstream ofs(fold + "/" + std::to_string(idx) + "_feature", std::ios::binary);
  if (!ofs.is_open()) return false;
  ofs.write((const char*)&info.rows, sizeof(int));
  ofs.write((const char*)&info.cols, sizeof(int));
  for (const float* f : {&info.zoom_ratio, &info.f_mm, &info.f_pixel, &info.gps_latitude, &info.gps_longitude}) ofs.write((const char*)f, sizeof(float));
  for (const std::string* t : {&info.cam_maker, &info.cam_model}) {
    const int n = (int)t->length();
    ofs.write((const char*)&n, sizeof(int));
    ofs.write(t->data(), n);
  }
  const int num_pts = (int)kp.size();
  ofs.write((const char*)&num_pts, sizeof(int));
  std::vector<float> c(2 * (size_t)num_pts);
  for (int i = 0; i < num_pts; i++) {  // points are centralized (database.cc:522-527)
    c[2 * i] = (float)(kp[i].x - info.cols / 2.0);
    c[2 * i + 1] = (float)(kp[i].y - info.rows / 2.0);
  }
  ofs.write((const char*)c.data(), c.size() * sizeof(float));
  const int rows = desc_cols ? (int)(desc.size() / desc_cols) : 0, type = 5;  // CV_32FC1
  ofs.write((const char*)&rows, sizeof(int));
  ofs.write((const char*)&desc_cols, sizeof(int));
  ofs.write((const char*)&type, sizeof(int));
  ofs.write((const char*)desc.data(), desc.size() * sizeof(float));
  return true;
}

bool ReadinImageFeatures(const std::string& fold, int idx, ImageInfo& info, std::vector<Point2f>& kp, std::vector<float>& desc,
                         int& desc_cols) {
  std::ifstream ifs(fold + "/" + std::to_string(idx) + "_feature", std::ios::binary);
  if (!ifs.is_open()) return false;
  ifs.read((char*)&info.rows, sizeof(int));
  ifs.read((char*)&info.cols, sizeof(int));
  for (float* f : {&info.zoom_ratio, &info.f_mm, &info.f_pixel, &info.gps_latitude, &info.gps_longitude}) ifs.read((char*)f, sizeof(float));
  for (std::string* t : {&info.cam_maker, &info.cam_model}) {
    int n = 0;
    ifs.read((char*)&n, sizeof(int));
    t->assign((size_t)std::max(0, n), '\0');
    ifs.read(&(*t)[0], n);
  }
  int num_pts = 0;
  ifs.read((char*)&num_pts, sizeof(int));
  std::vector<float> c(2 * (size_t)std::max(0, num_pts));
  ifs.read((char*)c.data(), c.size() * sizeof(float));
  kp.resize(num_pts);
  for (int i = 0; i < num_pts; i++) { kp[i].x = c[2 * i]; kp[i].y = c[2 * i + 1]; }
  int rows = 0, type = 0;
  ifs.read((char*)&rows, sizeof(int));
  ifs.read((char*)&desc_cols, sizeof(int));
  ifs.read((char*)&type, sizeof(int));
  if (type != 5) return false;  // only CV_32FC1 descriptors (database.cc:412-418)
  desc.resize((size_t)rows * desc_cols);
  ifs.read((char*)desc.data(), desc.size() * sizeof(float));
  return (bool)ifs;
}

// ---- track building -------------------------------------------------------------------------------
std::vector<Point3D> BuildTracks(const std::string& fold, const std::vector<std::vector<int>>& match_graph, std::vector<Camera>& cams,
                                 const std::vector<std::vector<Vec2>>& keypoints) {
  const int n_img = (int)match_graph.size();
  std::vector<int> n_feat(n_img), pair_img, off{0}, flat;
  for (int i = 0; i < n_img; i++) n_feat[i] = (int)keypoints[i].size();
  for (int i = 0; i < n_img; i++) {
    std::vector<int> ids;
    std::vector<std::vector<std::pair<int, int>>> recs;
    QueryMatch(fold, i, ids, recs);  // the file of image i holds one record per matched image
    for (int j = 0; j < n_img; j++) {
      if (match_graph[i][j] <= 0) continue;  // slam_gps.cc:571-575
      for (size_t r = 0; r < ids.size(); r++) {
        if (ids[r] != j) continue;
        pair_img.push_back(i); pair_img.push_back(j);
        for (auto& m : recs[r]) { flat.push_back(m.first); flat.push_back(m.second); }
        off.push_back((int)flat.size() / 2);
        break;
      }
    }
  }
  msfm_track_set* set = nullptr;
  // the whole image set at once: the GPU form of the walk (identical result, tests/test_gpu_tracks.py)
  check(msfm_tracks_build_device(Context(), n_img, n_feat.data(), (int)pair_img.size() / 2, pair_img.data(), off.data(), flat.data(), &set), "tracks_build");
  int nt = 0, no = 0;
  msfm_track_set_size(set, &nt, &no);
  std::vector<int> toff(nt + 1), oi(std::max(1, no)), of(std::max(1, no));
  msfm_track_set_fetch(set, toff.data(), oi.data(), of.data());
  msfm_track_set_destroy(set);
  std::vector<Point3D> pts(nt);
  for (int t = 0; t < nt; t++)
    for (int e = toff[t]; e < toff[t + 1]; e++)
      pts[t].AddObservation(&cams[oi[e]], keypoints[oi[e]][of[e]].x, keypoints[oi[e]][of[e]].y, oi[e]);
  return pts;
}

// ---- match files ---------------------------------------------------------------------------------
void WriteOutMatches(const std::string& fold, int idx1, int idx2, const std::vector<std::pair<int, int>>& matches) {
  const int num_match = (int)matches.size();
  if (!num_match) return;
  std::vector<int> tmp(2 * (size_t)num_match);
  for (int m = 0; m < num_match; m++) { tmp[2 * m] = matches[m].first; tmp[2 * m + 1] = matches[m].second; }
  std::ofstream ofs(fold + "/" + std::to_string(idx1) + "_match", std::ios::out | std::ios::app | std::ios::binary);
  ofs.write((const char*)&idx2, sizeof(int));
  ofs.write((const char*)&num_match, sizeof(int));
  ofs.write((const char*)tmp.data(), tmp.size() * sizeof(int));
}

void WriteOutMatchGraph(const std::string& fold, const std::vector<std::vector<int>>& match_graph) {
  std::ofstream ofs(fold + "/graph_matching.txt", std::ios::binary);
  for (auto& row : match_graph) {
    for (int v : row) ofs << v << " ";
    ofs << std::endl;
  }
}

void QueryMatch(const std::string& fold, int idx, std::vector<int>& image_ids,
                std::vector<std::vector<std::pair<int, int>>>& match_pts) {
  std::ifstream ifs(fold + "/" + std::to_string(idx) + "_match", std::ios::in | std::ios::binary);
  int id, num_match;
  while (ifs.read((char*)&id, sizeof(int))) {
    ifs.read((char*)&num_match, sizeof(int));
    std::vector<int> tmp(2 * (size_t)num_match);
    ifs.read((char*)tmp.data(), tmp.size() * sizeof(int));
    image_ids.push_back(id);
    std::vector<std::pair<int, int>> mt(num_match);
    for (int i = 0; i < num_match; i++) mt[i] = std::make_pair(tmp[2 * i], tmp[2 * i + 1]);
    match_pts.push_back(mt);
  }
}

void SLAMGPS::FeatureMatchingPriors(std::vector<std::vector<int>>& ids, std::vector<std::vector<Mat3>>& Fs,
                                    std::vector<std::vector<Mat3>>& Hs) {
  // cams_info (slam_gps.cc:324-327): camera id -> index in cams_; the points' observations in std::map key order
  std::map<int, int> cams_info;
  for (size_t i = 0; i < cams_.size(); i++) cams_info.insert(std::make_pair(cams_[i]->id_, (int)i));
  std::vector<int32_t> off(1, 0), cam;
  std::vector<double> xy;
  for (Point3D* p : pts_) {
    auto it1 = p->pts2d_.begin();
    for (auto it2 = p->cams_.begin(); it2 != p->cams_.end(); ++it1, ++it2) {
      cam.push_back(cams_info.find(it2->second->id_)->second);
      xy.push_back(it1->second.x);
      xy.push_back(it1->second.y);
    }
    off.push_back((int32_t)cam.size());
  }
  msfm_tracks t = {};
  t.n_tracks = (int)pts_.size();
  t.n_cams = (int)cams_.size();
  t.track_off = off.data();
  t.track_cam = cam.data();
  t.track_xy = xy.data();
  msfm_slam_prior_options o;
  msfm_slam_prior_default_options(&o);
  o.th_epipolar = (float)(2.0 / resize_ratio);   // float th_epipolar = 2.0 / resize_ratio;  (:316)
  o.th_distance = (float)(5.0 / resize_ratio);   // float th_distance = 5.0 / resize_ratio;  (:317)
  const size_t cap = std::max<size_t>(1, cams_.size() * (2 * o.win_size - 1));
  std::vector<int> pairs(2 * cap);
  std::vector<double> F(9 * cap), H(9 * cap);
  int n = 0;
  if (msfm_slam_priors(Context(), &t, &o, &n, pairs.data(), F.data(), H.data(), nullptr, nullptr) != MSFM_OK)
    throw std::runtime_error(std::string("msfm_slam_priors: ") + msfm_last_error(Context()));
  ids.assign(cams_.size(), {});
  Fs.assign(cams_.size(), {});
  Hs.assign(cams_.size(), {});
  for (int k = 0; k < n; k++) {
    Mat3 f, h;
    for (int q = 0; q < 9; q++) { f.m[q] = F[9 * (size_t)k + q]; h.m[q] = H[9 * (size_t)k + q]; }
    ids[pairs[2 * k]].push_back(pairs[2 * k + 1]);
    Fs[pairs[2 * k]].push_back(f);
    Hs[pairs[2 * k]].push_back(h);
  }
}

void SLAMGPS::WriteOutPriorInfo(const std::string& file, const std::vector<std::vector<int>>& ids, const std::vector<std::vector<Mat3>>& Fs,
                                const std::vector<std::vector<Mat3>>& Hs) {
  std::ofstream ff(file);
  ff << std::fixed << std::setprecision(12);
  ff << ids.size() << std::endl;
  for (size_t i = 0; i < ids.size(); i++) {
    ff << ids[i].size() << std::endl;
    for (size_t j = 0; j < ids[i].size(); j++) {
      ff << ids[i][j] << " ";
      for (int m = 0; m < 3; m++)
        for (int n = 0; n < 3; n++) {
          ff << Fs[i][j](m, n) << " ";
          ff << Hs[i][j](m, n) << " ";
        }
      ff << std::endl;
    }
  }
}

void SLAMGPS::ReadinPriorInfo(const std::string& file, std::vector<std::vector<int>>& ids, std::vector<std::vector<Mat3>>& Fs,
                              std::vector<std::vector<Mat3>>& Hs) {
  std::ifstream ff(file);
  int num = 0;
  ff >> num;
  ids.assign(num, {});
  Fs.assign(num, {});
  Hs.assign(num, {});
  for (int i = 0; i < num; i++) {
    int n = 0;
    ff >> n;
    ids[i].resize(n);
    Fs[i].resize(n);
    Hs[i].resize(n);
    for (int j = 0; j < n; j++) {
      ff >> ids[i][j];
      for (int m = 0; m < 3; m++)
        for (int q = 0; q < 3; q++) ff >> Fs[i][j](m, q) >> Hs[i][j](m, q);
    }
  }
}

void SLAMGPS::FeatureMatching(const std::vector<std::vector<float>>& descriptors, const std::vector<std::vector<Point2f>>& keypoints,
                              const std::vector<std::vector<int>>& ids, const std::vector<std::vector<Mat3>>& Fs, const std::vector<std::vector<Mat3>>& Hs,
                              std::vector<std::vector<std::vector<std::pair<int, int>>>>& matches_out, std::vector<std::vector<int>>& match_graph_out) {
  const size_t n_img = descriptors.size();
  if (keypoints.size() != n_img || ids.size() > n_img || Fs.size() != ids.size() || Hs.size() != ids.size())
    throw std::runtime_error("SLAMGPS::FeatureMatching: descriptors, keypoints and priors do not belong together");
  // the pair list in the order the loops of :432 / :451 walk it
  std::vector<int> flat;
  std::vector<double> F, H;
  for (size_t i = 0; i < ids.size(); i++) {
    if (Fs[i].size() != ids[i].size() || Hs[i].size() != ids[i].size()) throw std::runtime_error("SLAMGPS::FeatureMatching: one F and one H per id");
    for (size_t j = 0; j < ids[i].size(); j++) {
      flat.push_back((int)i); flat.push_back(ids[i][j]);
      F.insert(F.end(), Fs[i][j].m, Fs[i][j].m + 9);
      H.insert(H.end(), Hs[i][j].m, Hs[i][j].m + 9);
    }
  }
  const int n_pairs = (int)(flat.size() / 2);
  matches_out.assign(n_img, {});
  for (size_t i = 0; i < ids.size(); i++) matches_out[i].assign(ids[i].size(), {});
  match_graph_out.assign(n_img, std::vector<int>(n_img, 0));   // :426-430
  if (n_pairs == 0) return;
  msfm_descset* set = nullptr;
  msfm_match_result* res = nullptr;
  msfm_chain* chain = nullptr;
  auto release = [&] {
    if (chain) msfm_chain_destroy(chain);
    if (res) msfm_match_result_destroy(res);
    if (set) msfm_descset_destroy(set);
  };
  try {
    check(msfm_descset_create(Context(), (int)n_img, 128, &set), "descset_create");
    for (size_t i = 0; i < n_img; i++) {
      const int n = (int)(descriptors[i].size() / 128);
      if (keypoints[i].size() != (size_t)n) throw std::runtime_error("SLAMGPS::FeatureMatching: one keypoint per descriptor");
      check(msfm_descset_upload(set, (int)i, descriptors[i].data(), n), "descset_upload");
      if (n == 0) continue;
      std::vector<float> xy(2 * (size_t)n);
      for (int k = 0; k < n; k++) { xy[2 * k] = keypoints[i][k].x; xy[2 * k + 1] = keypoints[i][k].y; }
      check(msfm_descset_upload_keypoints(set, (int)i, xy.data(), n), "descset_upload_keypoints");
    }
    msfm_slam_match_options mo;
    msfm_slam_match_default_options(&mo);               // th_first_second_ratio 0.80 (:320)
    mo.th_epipolar = (float)(2.0 / resize_ratio);       // :316
    mo.th_distance = (float)(5.0 / resize_ratio);       // :317
    check(msfm_match_pairs_slam(set, flat.data(), n_pairs, F.data(), H.data(), &mo, 0, &res), "match_pairs_slam");
    check(msfm_chain_create(res, &chain), "chain_create");
    msfm_fransac_options fo;
    msfm_fransac_default_options(&fo);
    check(msfm_chain_verify_slam(chain, res, &fo), "chain_verify_slam");
    std::vector<int> n_m((size_t)n_pairs);
    check(msfm_chain_matches(chain, n_m.data(), nullptr, nullptr), "chain_matches");
    int p = 0;
    for (size_t i = 0; i < ids.size(); i++)
      for (size_t j = 0; j < ids[i].size(); j++, p++) {
        std::vector<int> m(2 * (size_t)std::max(1, n_m[p]));
        check(msfm_chain_fetch_matches(chain, p, m.data()), "chain_fetch_matches");
        auto& out = matches_out[i][j];
        out.resize((size_t)n_m[p]);
        for (int k = 0; k < n_m[p]; k++) out[k] = std::make_pair(m[2 * k], m[2 * k + 1]);
        match_graph_out[i][ids[i][j]] = n_m[p];          // :540
      }
  } catch (...) {
    release();
    throw;
  }
  release();
}

// ---- SLAM + GPS registration (slam_gps.cc:98-119) ---------------------------------------------
void Camera::Transformation(const Mat3& R, const Vec3& t, double scale) {
  const double* A = R.m;
  const double c00 = A[4] * A[8] - A[5] * A[7], c01 = A[5] * A[6] - A[3] * A[8], c02 = A[3] * A[7] - A[4] * A[6];
  const double invdet = 1.0 / (A[0] * c00 + A[1] * c01 + A[2] * c02);
  Mat3 Ri, Rn, sR;
  Ri.m[0] = c00 * invdet; Ri.m[1] = (A[2] * A[7] - A[1] * A[8]) * invdet; Ri.m[2] = (A[1] * A[5] - A[2] * A[4]) * invdet;
  Ri.m[3] = c01 * invdet; Ri.m[4] = (A[0] * A[8] - A[2] * A[6]) * invdet; Ri.m[5] = (A[2] * A[3] - A[0] * A[5]) * invdet;
  Ri.m[6] = c02 * invdet; Ri.m[7] = (A[1] * A[6] - A[0] * A[7]) * invdet; Ri.m[8] = (A[0] * A[4] - A[1] * A[3]) * invdet;
  for (int r = 0; r < 3; r++)
    for (int c = 0; c < 3; c++) Rn(r, c) = pos_rt_.R(r, 0) * Ri(0, c) + pos_rt_.R(r, 1) * Ri(1, c) + pos_rt_.R(r, 2) * Ri(2, c);
  pos_rt_.R = Rn;                                             // pos_rt_.R = pos_rt_.R * R.inverse()
  for (int k = 0; k < 9; k++) sR.m[k] = scale * R.m[k];
  const Vec3 rc = sR * pos_ac_.c;
  for (int k = 0; k < 3; k++) pos_ac_.c[k] = rc[k] + t[k];    // pos_ac_.c = scale * R * pos_ac_.c + t
  const Vec3 rt = pos_rt_.R * pos_ac_.c;
  for (int k = 0; k < 3; k++) pos_rt_.t[k] = -rt[k];          // pos_rt_.t = -pos_rt_.R * pos_ac_.c
  rotation::RotationMatrixToAngleAxis(pos_rt_.R, pos_ac_.a);
  UpdateDataFromPose();
}

void SLAMGPS::AbsoluteOrientationWithGPSGlobal() {
  const size_t n = cams_.size();
  std::vector<double> R(9 * n), c(3 * n), g(3 * n), oR(9 * n), ot(3 * n), oc(3 * n), oa(3 * n), og(3 * n);
  orient_weight_.assign(n, 0.0);
  for (size_t i = 0; i < n; i++) {
    for (int k = 0; k < 9; k++) R[9 * i + k] = cams_[i]->pos_rt_.R.m[k];
    for (int k = 0; k < 3; k++) { c[3 * i + k] = cams_[i]->pos_ac_.c[k]; g[3 * i + k] = cams_gps_[i][k]; }
  }
  msfm_gps_orient_result out;
  out.cam_R = oR.data(); out.cam_t = ot.data(); out.cam_c = oc.data(); out.cam_aa = oa.data(); out.gps = og.data(); out.weight = orient_weight_.data();
  if (msfm_gps_orient_global((int)n, R.data(), c.data(), g.data(), nullptr, &out) != MSFM_OK)
    throw std::runtime_error("AbsoluteOrientationWithGPSGlobal: fewer than 3 cameras");
  for (size_t i = 0; i < n; i++) {
    Camera* cm = cams_[i];
    for (int k = 0; k < 9; k++) cm->pos_rt_.R.m[k] = oR[9 * i + k];
    for (int k = 0; k < 3; k++) { cm->pos_rt_.t[k] = ot[3 * i + k]; cm->pos_ac_.c[k] = oc[3 * i + k]; cm->pos_ac_.a[k] = oa[3 * i + k]; cams_gps_[i][k] = og[3 * i + k]; }
    cm->UpdateDataFromPose();
  }
  for (int k = 0; k < 9; k++) orient_R_.m[k] = out.Rg[k];
  for (int k = 0; k < 3; k++) { orient_t_[k] = out.tg[k]; gps_offset_[k] = out.offset[k]; }
  orient_scale_ = out.scale; orient_err_ = out.err;
}

namespace {
// pts_ as CSR rows over cams_ (camera index = position in cams_), a point's observations in std::map order
struct SlamFlat {
  std::vector<int32_t> off, cam;
  std::vector<double> xy, R, t, c, fk, dc, X;
  std::vector<uint8_t> ok;
  msfm_tracks tr;
  SlamFlat(const std::vector<Camera*>& cams, const std::vector<Point3D*>& pts) {
    std::map<const Camera*, int> index;
    for (size_t i = 0; i < cams.size(); i++) {
      index[cams[i]] = (int)i;
      for (int k = 0; k < 9; k++) R.push_back(cams[i]->pos_rt_.R.m[k]);
      for (int k = 0; k < 3; k++) { t.push_back(cams[i]->pos_rt_.t[k]); c.push_back(cams[i]->pos_ac_.c[k]); }
      const CameraModel* m = cams[i]->cam_model_;
      fk.push_back(m->f_); fk.push_back(m->k1_); fk.push_back(m->k2_);
      dc.push_back(m->dcx_); dc.push_back(m->dcy_);
    }
    off.push_back(0);
    for (const Point3D* p : pts) {
      auto ip = p->pts2d_.begin();
      for (auto ic = p->cams_.begin(); ic != p->cams_.end(); ++ic, ++ip) {
        cam.push_back(index.at(ic->second));
        xy.push_back(ip->second.x); xy.push_back(ip->second.y);
      }
      off.push_back((int32_t)cam.size());
      for (int k = 0; k < 3; k++) X.push_back(p->data[k]);
      ok.push_back(p->is_bad_estimated_ ? 0 : 1);
    }
    tr.n_tracks = (int)pts.size(); tr.n_cams = (int)cams.size();
    tr.track_off = off.data(); tr.track_cam = cam.data(); tr.track_xy = xy.data();
    tr.cam_R = R.data(); tr.cam_t = t.data(); tr.cam_c = c.data(); tr.cam_fk = fk.data();
  }
};
}  // namespace

void SLAMGPS::GetAccuracy() {
  SlamFlat F(cams_, pts_);
  const size_t n = pts_.size();
  accuracy_errors_.assign(n, 0.0); accuracy_mse_.assign(n, 0.0); accuracy_n_obs_.assign(n, 0);
  std::vector<uint8_t> ok(n);
  int n_in = 0;
  check(msfm_point_accuracy_batch(Context(), &F.tr, F.dc.data(), F.X.data(), F.ok.data(), 0, th_outlier_, accuracy_errors_.data(), accuracy_mse_.data(),
                                  accuracy_n_obs_.data(), ok.data(), &count_outliers_, &n_in), "point_accuracy");
  for (size_t i = 0; i < n; i++) if (!ok[i]) pts_[i]->is_bad_estimated_ = true;   // slam_gps.cc:1587-1590 (a bad point's error is 1000.0)
}

void SLAMGPS::GetAccuracyHost() {
  const size_t n = pts_.size();
  accuracy_errors_.assign(n, 1000.0); accuracy_mse_.assign(n, 0.0); accuracy_n_obs_.assign(n, 0);   // accuracy_accessment.cc:94
  for (size_t i = 0; i < n; i++) {
    Point3D* p = pts_[i];
    if (p->is_bad_estimated_) continue;                                              // :95-97
    std::vector<double> errors;
    auto iter_pts = p->pts2d_.begin();
    for (auto iter_cams = p->cams_.begin(); iter_cams != p->cams_.end(); ++iter_cams, ++iter_pts) {   // :45-61
      const double* M = iter_cams->second->M;
      const CameraModel* m = iter_cams->second->cam_model_;
      const double pc0 = M[0] * p->data[0] + M[1] * p->data[1] + M[2] * p->data[2] + M[3];
      const double pc1 = M[4] * p->data[0] + M[5] * p->data[1] + M[6] * p->data[2] + M[7];
      const double pc2 = M[8] * p->data[0] + M[9] * p->data[1] + M[10] * p->data[2] + M[11];
      if (pc2 > 0) {
        const double x = pc0 / pc2, y = pc1 / pc2;
        const double r2 = x * x + y * y;
        const double distortion = 1.0 + r2 * (m->k1_ + m->k2_ * r2);
        const double u = m->f_ * distortion * x + m->dcx_, v = m->f_ * distortion * y + m->dcy_;
        const double du = u - iter_pts->second.x, dv = v - iter_pts->second.y;
        errors.push_back(du * du + dv * dv);
      }
    }
    if (errors.size() <= 1) continue;                                                // :64-66
    double e_avg = 0.0, e_mse = 0.0;
    for (size_t k = 0; k < errors.size(); k++) e_avg += errors[k];
    e_avg /= errors.size();
    for (size_t k = 0; k < errors.size(); k++) e_mse += (errors[k] - e_avg) * (errors[k] - e_avg);
    e_mse = std::sqrt(e_mse / (errors.size() - 1));
    accuracy_errors_[i] = e_avg; accuracy_mse_[i] = e_mse; accuracy_n_obs_[i] = (int)errors.size();
  }
  count_outliers_ = 0;
  for (size_t i = 0; i < n; i++)                                                     // slam_gps.cc:1584-1592
    if (accuracy_errors_[i] > th_outlier_) { pts_[i]->is_bad_estimated_ = true; count_outliers_++; }
}

void SLAMGPS::GPSRegistration2() {
  SlamFlat F(cams_, pts_);
  std::vector<double> g(3 * cams_.size());
  for (size_t i = 0; i < cams_.size(); i++) for (int k = 0; k < 3; k++) g[3 * i + k] = cams_gps_[i][k];
  check(msfm_gps_register_points(Context(), F.tr.n_tracks, F.off.data(), F.cam.data(), F.ok.data(), F.tr.n_cams, F.c.data(), g.data(), F.X.data()),
        "gps_register_points");
  for (size_t i = 0; i < pts_.size(); i++) for (int k = 0; k < 3; k++) pts_[i]->data[k] = F.X[3 * i + k];
  for (size_t i = 0; i < cams_.size(); i++) cams_[i]->SetACPose(cams_[i]->pos_ac_.a, cams_gps_[i]);   // :980-982
}

void SLAMGPS::GPSRegistration2Host() {
  std::vector<Vec3> cam_offset(cams_.size());                                        // :920-924
  std::map<const Camera*, int> cams_info;
  for (size_t i = 0; i < cams_.size(); i++) {
    for (int k = 0; k < 3; k++) cam_offset[i][k] = cams_gps_[i][k] - cams_[i]->pos_ac_.c[k];
    cams_info[cams_[i]] = (int)i;
  }
  for (size_t i = 0; i < pts_.size(); i++) {                                         // :933-978
    Point3D* p = pts_[i];
    if (p->is_bad_estimated_) continue;
    double offset_i[3] = {0.0, 0.0, 0.0}, weight_i = 0.0;
    for (auto it = p->cams_.begin(); it != p->cams_.end(); ++it) {
      const int id_cam = cams_info.at(it->second);
      const double dx = p->data[0] - cams_[id_cam]->pos_ac_.c(0), dy = p->data[1] - cams_[id_cam]->pos_ac_.c(1), dz = p->data[2] - cams_[id_cam]->pos_ac_.c(2);
      const double dis = std::sqrt(dx * dx + dy * dy + dz * dz);
      const double w = 1.0 / (std::sqrt(dis) + 5.0);
      weight_i += w;
      for (int k = 0; k < 3; k++) offset_i[k] += w * cam_offset[id_cam][k];
    }
    for (int k = 0; k < 3; k++) offset_i[k] /= weight_i;
    for (int k = 0; k < 3; k++) p->data[k] += offset_i[k];
  }
  for (size_t i = 0; i < cams_.size(); i++) cams_[i]->SetACPose(cams_[i]->pos_ac_.a, cams_gps_[i]);
}

}  // namespace objectsfm
