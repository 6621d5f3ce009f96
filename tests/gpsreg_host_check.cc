// The host mirror's registration steps (host/objectsfm.h: SLAMGPS::AbsoluteOrientationWithGPSGlobal, GetAccuracy,
// GPSRegistration2) against its own literal walks, on a model written by tests/test_gpu_gpsreg_host.py:
//   gpsreg_host_check <model> <out>
// model: int32 n_cams, n_tracks, n_rows; double cam_R [n][9], cam_c [n][3], model [n][5] (f, k1, k2, dcx, dcy), gps [n][3], path_gps
//        [n][3]; int32 off [n_tracks + 1], cam [n_rows]; double xy [n_rows][2], X [n_tracks][3]; uint8 ok [n_tracks].
// Two objects are built from it.  The first holds the cameras and path_gps and is oriented: the library call must equal
// Camera::Transformation applied twice by hand (slam_gps.cc:1639-1660).  The second holds the cameras, gps and the points:
// GetAccuracy and GPSRegistration2 must equal GetAccuracyHost and GPSRegistration2Host on a copy.  Exit status 1 on any difference;
// the results of the library forms go to <out> for the comparison with the Python host:
//   double orient cam_R [n][9], cam_t, cam_c, cam_aa, gps [n][3], weight [n], Rg [9], tg [3], scale, err, offset [3];
//   double errors [n_tracks], mse [n_tracks]; int32 n_obs [n_tracks]; uint8 bad [n_tracks]; int32 count_outliers;
//   double X [n_tracks][3] after the shift; double cam data [n][6] after SetACPose.
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>

#include "objectsfm.h"

using namespace objectsfm;

namespace {
struct Model {
  std::vector<std::unique_ptr<CameraModel>> models;
  std::vector<std::unique_ptr<Camera>> cams;
  std::vector<std::unique_ptr<Point3D>> pts;
  SLAMGPS s;
};

template <class T>
std::vector<T> get(FILE* f, size_t n) {
  std::vector<T> v(n);
  if (n && fread(v.data(), sizeof(T), n, f) != n) { fprintf(stderr, "short model file\n"); exit(2); }
  return v;
}
template <class T>
void put(FILE* f, const T* p, size_t n) { if (n) fwrite(p, sizeof(T), n, f); }

void build(Model& m, int n, const double* R, const double* c, const double* md, const double* gps, int nt, const int* off, const int* cam,
           const double* xy, const double* X, const uint8_t* ok) {
  for (int i = 0; i < n; i++) {
    m.models.emplace_back(new CameraModel());
    CameraModel* cm = m.models.back().get();
    cm->f_ = md[5 * i]; cm->k1_ = md[5 * i + 1]; cm->k2_ = md[5 * i + 2]; cm->dcx_ = md[5 * i + 3]; cm->dcy_ = md[5 * i + 4];
    cm->UpdateDataFromModel();
    m.cams.emplace_back(new Camera());
    Camera* ca = m.cams.back().get();
    ca->SetID(i); ca->AssociateCamereModel(cm);
    for (int k = 0; k < 9; k++) ca->pos_rt_.R.m[k] = R[9 * i + k];
    for (int k = 0; k < 3; k++) ca->pos_ac_.c[k] = c[3 * i + k];
    const Vec3 t = ca->pos_rt_.R * ca->pos_ac_.c;
    for (int k = 0; k < 3; k++) ca->pos_rt_.t[k] = -t[k];
    rotation::RotationMatrixToAngleAxis(ca->pos_rt_.R, ca->pos_ac_.a);
    ca->UpdateDataFromPose();
    m.s.cams_.push_back(ca); m.s.cam_models_.push_back(cm);
    Vec3 g; for (int k = 0; k < 3; k++) g[k] = gps[3 * i + k];
    m.s.cams_gps_.push_back(g);
  }
  for (int p = 0; p < nt; p++) {
    m.pts.emplace_back(new Point3D());
    Point3D* pt = m.pts.back().get();
    pt->id_ = p;
    for (int k = 0; k < 3; k++) pt->data[k] = X[3 * p + k];
    pt->is_bad_estimated_ = ok[p] == 0;
    for (int i = off[p]; i < off[p + 1]; i++) pt->AddObservation(m.cams[cam[i]].get(), xy[2 * i], xy[2 * i + 1], cam[i]);   // (cameras ascending: std::map order = row order)
    m.s.pts_.push_back(pt);
  }
}

int differ(const char* what, const double* a, const double* b, size_t n) {
  if (memcmp(a, b, n * sizeof(double)) == 0) return 0;
  fprintf(stderr, "%s differs\n", what);
  return 1;
}
}  // namespace

int main(int argc, char** argv) {
  if (argc < 3) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  const std::vector<int> hdr = get<int>(f, 3);
  const int n = hdr[0], nt = hdr[1], nr = hdr[2];
  const auto R = get<double>(f, 9 * (size_t)n), c = get<double>(f, 3 * (size_t)n), md = get<double>(f, 5 * (size_t)n), gps = get<double>(f, 3 * (size_t)n),
             pgps = get<double>(f, 3 * (size_t)n);
  const auto off = get<int>(f, (size_t)nt + 1), cam = get<int>(f, (size_t)nr);
  const auto xy = get<double>(f, 2 * (size_t)nr), X = get<double>(f, 3 * (size_t)nt);
  const auto ok = get<uint8_t>(f, (size_t)nt);
  fclose(f);
  int bad = 0;
  FILE* o = fopen(argv[2], "wb");
  if (!o) return 2;

  // ---- AbsoluteOrientationWithGPSGlobal against Camera::Transformation by hand ----
  Model a, b;
  build(a, n, R.data(), c.data(), md.data(), pgps.data(), 0, off.data(), cam.data(), xy.data(), X.data(), ok.data());
  build(b, n, R.data(), c.data(), md.data(), pgps.data(), 0, off.data(), cam.data(), xy.data(), X.data(), ok.data());
  a.s.AbsoluteOrientationWithGPSGlobal();
  for (int i = 0; i < n; i++) b.s.cams_[i]->Transformation(a.s.orient_R_, a.s.orient_t_, a.s.orient_scale_);   // slam_gps.cc:1639-1641
  Vec3 offset;
  for (int i = 0; i < n; i++) for (int k = 0; k < 3; k++) offset[k] += b.s.cams_[i]->pos_ac_.c[k];               // :1651-1655
  for (int k = 0; k < 3; k++) offset[k] /= n;
  Vec3 neg; for (int k = 0; k < 3; k++) neg[k] = -offset[k];
  for (int i = 0; i < n; i++) b.s.cams_[i]->Transformation(Mat3(), neg, 1.0);                                     // :1657-1660
  bad += differ("gps_offset_", offset.v, a.s.gps_offset_.v, 3);
  for (int i = 0; i < n; i++) {
    bad += differ("oriented camera data", a.s.cams_[i]->data, b.s.cams_[i]->data, 6);
    bad += differ("oriented camera M", a.s.cams_[i]->M, b.s.cams_[i]->M, 12);
    bad += differ("oriented camera c", a.s.cams_[i]->pos_ac_.c.v, b.s.cams_[i]->pos_ac_.c.v, 3);
  }
  for (int i = 0; i < n; i++) put(o, a.s.cams_[i]->pos_rt_.R.m, 9);
  for (int i = 0; i < n; i++) put(o, a.s.cams_[i]->pos_rt_.t.v, 3);
  for (int i = 0; i < n; i++) put(o, a.s.cams_[i]->pos_ac_.c.v, 3);
  for (int i = 0; i < n; i++) put(o, a.s.cams_[i]->pos_ac_.a.v, 3);
  for (int i = 0; i < n; i++) put(o, a.s.cams_gps_[i].v, 3);
  put(o, a.s.orient_weight_.data(), n);
  put(o, a.s.orient_R_.m, 9); put(o, a.s.orient_t_.v, 3); put(o, &a.s.orient_scale_, 1); put(o, &a.s.orient_err_, 1); put(o, a.s.gps_offset_.v, 3);

  // ---- GetAccuracy / GPSRegistration2 against the literal walks ----
  Model g, h;
  build(g, n, R.data(), c.data(), md.data(), gps.data(), nt, off.data(), cam.data(), xy.data(), X.data(), ok.data());
  build(h, n, R.data(), c.data(), md.data(), gps.data(), nt, off.data(), cam.data(), xy.data(), X.data(), ok.data());
  g.s.GetAccuracy();
  h.s.GetAccuracyHost();
  bad += differ("accuracy_errors_", g.s.accuracy_errors_.data(), h.s.accuracy_errors_.data(), nt);
  bad += differ("accuracy_mse_", g.s.accuracy_mse_.data(), h.s.accuracy_mse_.data(), nt);
  if (g.s.accuracy_n_obs_ != h.s.accuracy_n_obs_ || g.s.count_outliers_ != h.s.count_outliers_) { fprintf(stderr, "accuracy counts differ\n"); bad++; }
  std::vector<uint8_t> flags(nt);
  for (int p = 0; p < nt; p++) {
    flags[p] = g.s.pts_[p]->is_bad_estimated_;
    if (g.s.pts_[p]->is_bad_estimated_ != h.s.pts_[p]->is_bad_estimated_) { fprintf(stderr, "is_bad_estimated_ of point %d differs\n", p); bad++; }
  }
  put(o, g.s.accuracy_errors_.data(), nt); put(o, g.s.accuracy_mse_.data(), nt); put(o, g.s.accuracy_n_obs_.data(), nt); put(o, flags.data(), nt);
  put(o, &g.s.count_outliers_, 1);
  g.s.GPSRegistration2();
  h.s.GPSRegistration2Host();
  for (int p = 0; p < nt; p++) bad += differ("registered point", g.s.pts_[p]->data, h.s.pts_[p]->data, 3);
  for (int i = 0; i < n; i++) bad += differ("camera on its GPS position", g.s.cams_[i]->data, h.s.cams_[i]->data, 6);
  for (int p = 0; p < nt; p++) put(o, g.s.pts_[p]->data, 3);
  for (int i = 0; i < n; i++) put(o, g.s.cams_[i]->data, 6);
  fclose(o);
  if (bad) { fprintf(stderr, "%d difference(s)\n", bad); return 1; }
  printf("gpsreg_host_check ok: %d cameras, %d points, %d outliers\n", n, nt, g.s.count_outliers_);
  return 0;
}
