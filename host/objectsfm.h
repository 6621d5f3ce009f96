// C++ host side above the C ABI: the reference's camera / point / bundle-adjuster classes
// (same names, members and method spellings, typos included) re-implemented without Eigen, Ceres,
// OpenCV or FLANN, so that a maintainer can see exactly where libmsfm plugs in:
//   CameraModel         SfM/src/basic_structs.h:48-124
//   Camera              SfM/src/camera.h:34-85, camera.cc:43-137
//   Point3D             SfM/src/structure.h:29-72, structure.cc:163-355
//   BundleAdjuster      SfM/src/optimizer.h, optimizer.cc:31-232
//   FineMatchingGraph   SfM/src/graph/fine_matching_graph.cc:40-194 (kNN + ratio tests part)
// Everything numeric on the hot path goes through include/msfm.h; there is no CPU fallback.
#pragma once
#include <array>
#include <cmath>
#include <map>
#include <memory>
#include <random>
#include <string>
#include <utility>
#include <vector>

#include "../include/msfm.h"

namespace objectsfm {

struct Vec2 { double x = 0, y = 0; double operator()(int i) const { return i ? y : x; } };
struct Vec3 {
  double v[3] = {0, 0, 0};
  double& operator()(int i) { return v[i]; }
  double operator()(int i) const { return v[i]; }
  double& operator[](int i) { return v[i]; }
  double operator[](int i) const { return v[i]; }
};
struct Mat3 {
  double m[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};  // row-major
  double& operator()(int r, int c) { return m[3 * r + c]; }
  double operator()(int r, int c) const { return m[3 * r + c]; }
};
inline Vec3 operator*(const Mat3& A, const Vec3& x) {
  Vec3 y;
  for (int r = 0; r < 3; r++) y[r] = A(r, 0) * x[0] + A(r, 1) * x[1] + A(r, 2) * x[2];
  return y;
}
inline Mat3 transpose(const Mat3& A) { Mat3 T; for (int r = 0; r < 3; r++) for (int c = 0; c < 3; c++) T(r, c) = A(c, r); return T; }

namespace rotation {  // SfM/src/utils/basic_funcs.cc:25-158
void AngleAxisToRotationMatrix(const Vec3& angle_axis, Mat3& R);
void RotationMatrixToAngleAxis(const Mat3& R, Vec3& axis);
}  // namespace rotation

struct RTPose { Mat3 R; Vec3 t; };  // basic_structs.h:126-145
struct ACPose { Vec3 a, c; };

struct BundleAdjustOptions {  // basic_structs.h:229-235
  int max_num_iterations = 200;
  bool minimizer_progress_to_stdout = true;
  int num_threads = 1;
};

struct CameraModel {  // basic_structs.h:48-124
  CameraModel() {}
  CameraModel(int id, int h, int w, double f_mm, double f, std::string cam_maker, std::string cam_model);
  void SetFocalLength(double f) { f_ = f; UpdateDataFromModel(); }
  void UpdateDataFromModel() { data[0] = f_; data[1] = k1_; data[2] = k2_; data[3] = dcx_; data[4] = dcy_; }
  void UpdataModelFromData() { f_ = data[0]; k1_ = data[1]; k2_ = data[2]; dcx_ = data[3]; dcy_ = data[4]; px_ += dcx_; py_ += dcy_; }
  void AddCamera(int idx) { idx_cams_.push_back(idx); num_cams_++; }
  void SetImmutable() { is_mutable_ = false; }
  int id_ = 0;
  std::string cam_maker_, cam_model_;
  int w_ = 0, h_ = 0;
  double f_mm_ = 0, f_ = 0, f_hyp_ = 0, px_ = 0, py_ = 0;
  double k1_ = 0, k2_ = 0, dcx_ = 0, dcy_ = 0;
  double data[5] = {0, 0, 0, 0, 0};  // {f, k1, k2, dcx, dcy}; BA optimises the first three (optimizer.cc:90-92)
  int num_cams_ = 0;
  std::vector<int> idx_cams_;
  bool is_mutable_ = true;
};

class Point3D;
class Camera {  // camera.h:34-85
 public:
  void AssociateImage(int id_img) { id_img_ = id_img; }
  void AssociateCamereModel(CameraModel* cam_model) { cam_model_ = cam_model; }
  void SetRTPose(const Mat3& R, const Vec3& t);   // camera.cc:43-54
  void SetACPose(const Vec3& a, const Vec3& c);   // camera.cc:69-80
  void Transformation(const Mat3& R, const Vec3& t, double scale);   // camera.cc:79-87 (R.inverse() by cofactors)
  void UpdateDataFromPose();                      // camera.cc:89-111
  void UpdatePoseFromData();                      // camera.cc:113-137
  void SetMutable(bool is_mutable) { is_mutable_ = is_mutable; }
  void AddPoints(Point3D* pt, int idx) { pts_.insert(std::make_pair(idx, pt)); }     // camera.cc:152-155
  void AddVisibleCamera(int id_visible_cam) { visible_cams_.push_back(id_visible_cam); }  // camera.cc:157-160
  void SetID(int id) { id_ = id; }
  int id_ = 0;
  int id_img_ = 0;
  std::map<int, Point3D*> pts_;      // global feature id -> 3-D point (camera.h:81)
  std::vector<int> visible_cams_;    // camera.h:82
  CameraModel* cam_model_ = nullptr;
  RTPose pos_rt_;
  ACPose pos_ac_;
  double data[6] = {0, 0, 0, 0, 0, 0};  // angle-axis, t
  double M[12] = {0};                   // [R|t] row-major 3x4
  bool is_mutable_ = true;
};

class Point3D {  // structure.h:29-72
 public:
  void AddObservation(Camera* cam, double x, double y, int idx);  // structure.cc:128-137
  bool Trianglate(double th_error, double th_angle);   // DLT, structure.cc:163-209
  bool Trianglate2(double th_error, double th_angle);  // ray midpoint, structure.cc:211-265
  void Reprojection();                                 // structure.cc:267-300
  bool SufficientTriangulationAngle(double th_angle_triangulation);  // structure.cc:325-355 (through the batch kernel)
  void SetMutable(bool is_mutable) { is_mutable_ = is_mutable; }
  int id_ = 0;
  double data[3] = {0, 0, 0};
  std::map<int, Camera*> cams_;
  std::map<int, Vec2> pts2d_;
  double weight = 1.0, mse_ = 0.0;
  bool is_mutable_ = true, is_bad_estimated_ = false, is_new_added_ = true;
};

// One GPU context per process; created on first use, destroyed at exit.
msfm_ctx* Context();
// `n_gpus` contexts in this one process (msfm_ctx_create_multi); share_device_0: all of them on device 0 (a one-GPU box).
// Call before the first GPU call.  Matching, triangulation / reprojection and the bundle adjustment then split inside the library.
void UseGpus(int n_gpus, bool share_device_0 = false);

// Batched forms the pipeline should prefer (RemovePointOutliers, sfm_incremental.cc:1831-1863; GenerateNew3DPoints has its
// own call, IncrementalSfM::GenerateNew3DPoints below): one kernel launch for all points.
void TrianglateBatch(const std::vector<Point3D*>& pts, double th_error, double th_angle, bool dlt, std::vector<char>* ok);
void ReprojectionBatch(const std::vector<Point3D*>& pts);

class BundleAdjuster {  // optimizer.h / optimizer.cc:31-232
 public:
  BundleAdjuster(std::vector<Camera*> cams, std::vector<CameraModel*> cam_models, std::vector<Point3D*> pts);
  void SetOptions(BundleAdjustOptions options);                 // optimizer.cc:42-48
  void RunOptimizetion(bool is_initial_run, double weight);     // optimizer.cc:50-135 -> msfm_ba_solve
  void UpdateParameters();                                      // optimizer.cc:142-153
  void Normalize();                                             // optimizer.cc:155-195
  void Perturb();                                               // optimizer.cc:197-232 (seeded std::mt19937_64, not std::rand)
  // The absolute GPS rows SLAMGPS::FullBundleAdjustment adds after the reprojection rows (slam_gps.cc:714-832,
  // use_absolute_gps): one GPSErrorPoseAbsolute per camera on pose[3:6], Huber(1), weight = count1 / cams_.size()
  // (integer division, :824) with count1 = reprojection residual blocks added.  Empty = none.
  void SetGPS(const std::vector<Vec3>& cams_gps) { cams_gps_ = cams_gps; }
  msfm_ba_summary summary_;
  std::vector<msfm_ba_iteration> iterations_;
  unsigned long long perturb_seed_ = 0x4D53464DULL;
  bool keep_point_weights_ = false;   // SLAMGPS passes pts_[i]->weight as it is (slam_gps.cc:703)

 private:
  std::vector<Camera*> cams_;
  std::vector<CameraModel*> cam_models_;
  std::vector<Point3D*> pts_;
  std::vector<Vec3> cams_gps_;
  msfm_ba_options options_;
};

// The bundle-adjustment side of the incremental loop (SfM/src/sfm_incremental.h/.cc): which cameras and points a
// partial adjustment frees, the full adjustment, the outlier sweep - and, on the resident match store, the seed search, the
// search for the next image, its localisation and its new points.  File handling stays with its own stage (matching above).
struct IncrementalSfMOptions {       // basic_structs.h:147-227, the fields this part reads
  double th_mse_outliers = 3.0;      // test_sfm.cc:46 (UAV), 1.0 for WEB (:57)
  int th_visible_matches = 5;        // `count_2d3d_ij > 5`, sfm_incremental.cc:503
  bool use_same_camera = false;      // basic_structs.h:167
  int idx_max_per_image = 1000000;   // basic_structs.h:171: global feature id = local + idx_max_per_image * image
  int th_max_failure_localization = 5;   // basic_structs.h:176
  double th_mse_reprojection = 3.0;      // basic_structs.h:187
  double th_angle_small = 3.0 / 180.0 * 3.1415;   // basic_structs.h:190
  int th_seedpair_structures = 20;       // basic_structs.h:174
  double th_angle_large = 5.0 / 180.0 * 3.1415;   // basic_structs.h:191
  int th_min_2d3d_corres = 20;           // basic_structs.h:177
  double th_mse_localization = 5.0;      // basic_structs.h:186
};
// What FindImageToLocalize reads of Graph (SfM/src/graph/graph.h): match_graph_ and the verified match lists - here in memory
// in the flat layout of msfm_match_store_create instead of behind Graph::QueryMatch's `<i>_match` files (graph.cc:92-137).
struct MatchGraph {
  std::vector<int> match_graph_;                 // [num_imgs * num_imgs] matches of the ordered pair (i, j)
  std::vector<int> n_features;                   // [num_imgs]
  std::vector<int> pair_img, match_off, matches; // pairs strictly ascending in (idx1, idx2)
};
class IncrementalSfM {
 public:
  void ImmutableCamsPoints();                                            // sfm_incremental.cc:1865-1878
  void MutableCamsPoints();                                              // sfm_incremental.cc:1880-1893
  void UpdateVisibleGraph(int idx_new_cam, std::vector<int> idxs_visible_cam);  // sfm_incremental.cc:1895-1903
  // the counting loop of FindImageToLocalize (sfm_incremental.cc:455-506) for a camera whose points are attached:
  // cameras through which it has more than th_visible_matches 2D-3D matches (non-bad points), ascending
  std::vector<int> VisibleCameras(int idx_cam) const;
  void PartialBundleAdjustment(int idx);                                 // sfm_incremental.cc:917-1014
  void FullBundleAdjustment();                                           // sfm_incremental.cc:1016-1026
  void RemovePointOutliers();                                            // sfm_incremental.cc:1831-1863 (one batched reprojection)
  // The verified matches of the image set (pair_img [P][2] strictly ascending, match_off [P+1], matches [M][2]): fills graph_
  // and uploads them once into a msfm_match_store; sizes is_img_processed_ / localize_fail_times_ when they are empty.
  void SetMatches(const std::vector<int>& n_features, const std::vector<int>& pair_img, const std::vector<int>& match_off,
                  const std::vector<int>& matches);
  // sfm_incremental.cc:417-563: the candidate images (:423-438) on the host, then one msfm_localize_candidates call on the
  // flat state gathered from cams_ / pts_ (pts_[i]->id_ == i, as LocalizeImage :599 indexes them).  Ties the reference's
  // std::sort leaves open go to the lower feature / the lower image id.
  void FindImageToLocalize(std::vector<int>& image_ids, std::vector<std::vector<std::pair<int, int>>>& corres_2d3d,
                           std::vector<std::vector<int>>& visible_cams);
  // The same function as the reference writes it - std::map walks on one thread - over the matches in memory (same ties):
  // what scripts/localize_bench.py times the library call against, and a second opinion for tests/localize_host_check.cc.
  void FindImageToLocalizeHost(std::vector<int>& image_ids, std::vector<std::vector<std::pair<int, int>>>& corres_2d3d,
                               std::vector<std::vector<int>>& visible_cams) const;
  // Run :126-164 (sfm_incremental.cc): FindImageToLocalize, then the tries of :146-159 around LocalizeImage (:565-753) through
  // two library calls - msfm_localize_candidates with the points, whose correspondences stay on the device, and
  // msfm_localize_poses on that set, in chunks of localize_options_.max_tries rows until a row passes or the rows run out.  The
  // tried rows ahead of the winner get their localize_fail_times_ incremented (:650 / :681); the winner becomes a Camera - on
  // the CameraModel of a camera whose image has the same image_model_ (at that model's current f_), else on a new one that
  // starts at image_focal_ (0.0: the sweep around image_focal_init_, :675, and SetFocalLength, :703) - with SetRTPose, the
  // observations and bad flags of :708-729 as the call reports them, and UpdateVisibleGraph (:748).  As in the reference
  // is_img_processed_ / img_cam_map_ are the caller's (Run :175-176).  Returns whether an image was localised.
  // Needs SetMatches, SetKeypoints, image_focal_, image_model_ and, for images without a focal length, image_focal_init_.
  bool LocalizeNextImage();
  // The reference's function for one image, through the public pose calls on host arrays.  The image is handed to them as
  // problem localize_row_ (its row in FindImageToLocalize's order, set by the caller) behind empty problems, so it draws the
  // samples the batched call draws: the same camera bit for bit.  A second opinion for tests/localizepose_host_check.cc and
  // what scripts/localizepose_bench.py times the batched call against.
  bool LocalizeImage(int id_img, std::vector<std::pair<int, int>>& corres_2d3d, std::vector<int>& visible_cams);
  int localize_row_ = 0;
  msfm_localize_pose_options localize_options_;   // msfm_localize_pose_default_options; the two thresholds come from options_ at each call
  std::vector<double> image_focal_init_;     // per image: 1.2 * max(w, h) (:675), read where the model has no focal length
  std::vector<int> localize_image_ids_;      // of the last LocalizeNextImage: the ranked candidates,
  std::vector<int> localize_failed_;         // the images whose fail counter it incremented,
  int localize_count_inliers_ = 0;           // count_inliers (:727) of the winner
  // sfm_incremental.cc:1790-1829: the image pairs in the order the seed search tries them.  Row sums in binary32, the C
  // library's log; ties, which the reference's std::sort leaves open, go to the lower i * num_img + j.
  void SortImagePairs(std::vector<std::pair<int, int>>& seed_pair_hyps) const;
  // sfm_incremental.cc:224-415.  The ranked pairs go to msfm_seed_hypotheses on the resident store in chunks of seed_chunk_
  // until a chunk has a winner (hypothesis h of a chunk draws the samples of problem h); the winner's two cameras, their
  // models and its points become cams_ / cam_models_ / pts_, then FullBundleAdjustment, RemovePointOutliers and the
  // bookkeeping of :401-408.  Needs SetMatches, SetKeypoints and the per-image image_focal_ / image_model_.
  bool FindSeedPairThenReconstruct();
  // The same function as the reference writes it: one hypothesis at a time through RelativePoseWith[out]FocalLength's library
  // calls and Trianglate2 per match, on host arrays.  Hypothesis i of the walk is handed to the pose call as problem
  // i % seed_chunk_ behind empty problems, so it draws the samples the batched call draws: same poses bit for bit, points
  // to the 1e-9 by which msfm_triangulate_midpoint_batch differs.  What scripts/seed_bench.py times the batched call against.
  bool FindSeedPairThenReconstructHost();
  // sfm_incremental.cc:755-915 for the newest camera (cams_.size() - 1) and its visible_cams_: the flat state gathered from
  // cams_ / pts_, one msfm_new_points call on the resident store, then the points appended in the call's order - two
  // observations, is_new_added_, id, Camera::AddPoints (:899-910).  Needs SetMatches and SetKeypoints.  std::sort's ties (:897)
  // keep the order of the walk.  The call is always handed keypoints_, so the keypoint rows of the involved images are
  // uploaded every time, also when the store came from a chain and holds them (the appended observations need keypoints_ anyway).
  void GenerateNew3DPoints();
  // The same function as the reference writes it: one Point3D::Trianglate2 per candidate (a library call each), the same tie
  // rule.  Same points, order and inserts, coordinates to the 1e-9 by which msfm_triangulate_midpoint_batch differs.  What
  // scripts/newpoints_bench.py times the batched call against, and a second opinion for tests/newpoints_host_check.cc.
  void GenerateNew3DPointsHost();
  int num_new_points_ = 0;                   // points the last of the two appended
  // Run :172-186 (sfm_incremental.cc) for camera idx_new_cam in ONE msfm_round_adjust call: PartialBundleAdjustment(idx_new_cam),
  // with `full` FullBundleAdjustment behind it, then RemovePointOutliers.  Both sides of the flat state are gathered from the
  // std::maps - the camera side from Camera::pts_ as GenerateNew3DPoints gathers it, the point side (one row per observation)
  // from Point3D::cams_ - and everything is written back: Camera::data / pos_rt_ / pos_ac_ / M and is_mutable_, CameraModel::data
  // and f_, k1_, k2_, Point3D::data, is_mutable_, is_bad_estimated_, mse_, is_new_added_.  Needs SetMatches and SetKeypoints
  // (the observations' coordinates are the keypoints, as :592-600 / :810-821 store them) and pts_[i]->id_ == i; no GPS rows.
  // The three methods above remain the one-stage-at-a-time form.
  void AdjustRound(int idx_new_cam, bool full);
  int round_counts_[3] = {0, 0, 0};          // of the last AdjustRound: count_outliers, count_new_add, count_outliers_new_add (:1833-1862)
  int round_adjust_[2][2] = {{0, 0}, {0, 0}};   // "adjust cams" / "adjust pts" (:962-963) of the partial and of the full solve
  int round_solved_[2] = {0, 0};
  msfm_ba_summary round_summary_[2] = {};    // (iterations point into round_iterations_)
  std::vector<msfm_ba_iteration> round_iterations_[2];
  void SetKeypoints(const std::vector<float>& keypoints) { keypoints_ = keypoints; }   // [sum of n_features][2], images in order
  std::vector<float> keypoints_;
  std::vector<double> image_focal_;          // per image: f of its camera model in pixels, 0.0 = unknown (CameraModel::f_)
  std::vector<int> image_model_;             // per image: images with equal values share a CameraModel (CameraAssociateCameraModel)
  int seed_chunk_ = 64;
  bool seed_adjust_ = true;                  // false: stop behind the gates, before FullBundleAdjustment (tests, timing)
  int seed_hyps_visited_ = 0;                // hypotheses the reference's loop visits up to and including the winner
  msfm_seed_options seed_options_;           // filled by the constructor from msfm_seed_default_options and options_
  IncrementalSfM();
  MatchGraph graph_;
  std::vector<bool> is_img_processed_;
  std::vector<int> localize_fail_times_;
  std::map<int, int> img_cam_map_;           // image id -> index in cams_
  std::shared_ptr<msfm_match_store> store_;  // the resident copy of graph_'s matches
  std::vector<Camera*> cams_;
  std::vector<CameraModel*> cam_models_;
  std::vector<Point3D*> pts_;
  // BASELINE config 5 ("incremental-window BA with GCP constraints"): when set, both adjustments attach the
  // absolute GPS rows of SLAMGPS::FullBundleAdjustment (slam_gps.cc:818-830) to the cameras they free
  std::vector<Vec3> cams_gps_;
  IncrementalSfMOptions options_;
  BundleAdjustOptions bundle_full_options_, bundle_partial_options_;
  bool found_seed_ = true;
  msfm_ba_summary summary_;                  // of the last adjustment
  std::vector<msfm_ba_iteration> iterations_;
};

struct Point2f;
// SLAMGPS::FullBundleAdjustment (SfM/src/slam_gps.cc:675-863): every non-bad point's observations as
// ReprojectionErrorPoseCamXYZ rows with the point's weight, the absolute GPS rows, max 200 iterations, 8 threads.
class SLAMGPS {
 public:
  void FullBundleAdjustment();
  // SLAMGPS::FeatureMatching step 1 (slam_gps.cc:323-423) through msfm_slam_priors: camera i's kept window partners ids[i]
  // (ascending) with the prior F / H of each (row-major [9]), from pts_ (observations in std::map key order) over cams_.
  // Window and thresholds of :314-319: win 5, 20 shared points, th_epipolar = 2.0 / resize_ratio, th_distance =
  // 5.0 / resize_ratio (binary32, as the reference's `float` locals), th_ratio_f 0.5, th_h_f_ratio 0.90.
  void FeatureMatchingPriors(std::vector<std::vector<int>>& ids, std::vector<std::vector<Mat3>>& Fs, std::vector<std::vector<Mat3>>& Hs);
  // feature/prior.txt (slam_gps.cc:1821-1885): the camera count, per camera n and n lines `id F00 H00 F01 H01 ... F22 H22`
  static void WriteOutPriorInfo(const std::string& file, const std::vector<std::vector<int>>& ids, const std::vector<std::vector<Mat3>>& Fs,
                                const std::vector<std::vector<Mat3>>& Hs);
  static void ReadinPriorInfo(const std::string& file, std::vector<std::vector<int>>& ids, std::vector<std::vector<Mat3>>& Fs,
                              std::vector<std::vector<Mat3>>& Hs);
  // SLAMGPS::FeatureMatching step 2 (slam_gps.cc:425-555) for the ids / Fs / Hs of FeatureMatchingPriors: descriptors [image][n*128]
  // and keypoints (centred pixels) uploaded once, then msfm_match_pairs_slam (the three checks, :469-503), msfm_chain_create and
  // msfm_chain_verify_slam (GeoVerificationFundamental on all survivors, :513; the pair keeps `inliers` whatever the verdict,
  // :514-518).  matches_out[i][j] = the kept (feature in i, feature in ids[i][j]) of pair (i, ids[i][j]), fetched with
  // msfm_chain_fetch_matches; match_graph_out[i][ids[i][j]] = their number (:540).  Thresholds as in FeatureMatchingPriors,
  // th_first_second_ratio 0.80 (:320).
  void FeatureMatching(const std::vector<std::vector<float>>& descriptors, const std::vector<std::vector<Point2f>>& keypoints,
                       const std::vector<std::vector<int>>& ids, const std::vector<std::vector<Mat3>>& Fs, const std::vector<std::vector<Mat3>>& Hs,
                       std::vector<std::vector<std::vector<std::pair<int, int>>>>& matches_out, std::vector<std::vector<int>>& match_graph_out);
  std::vector<Camera*> cams_;
  std::vector<CameraModel*> cam_models_;
  std::vector<Point3D*> pts_;
  std::vector<Vec3> cams_gps_;               // cv::Point3d cams_gps_ (slam_gps.h)
  // The registration steps of Run (slam_gps.cc:98-119), each one library call on arrays gathered from cams_ / pts_ (a point's
  // observations in std::map order, camera index = position in cams_) and written back:
  //   AbsoluteOrientationWithGPSGlobal (:1596-1674) msfm_gps_orient_global: cams_ get R, t, c, a and data / M; cams_gps_ is
  //                                    shifted; gps_offset_, orient_scale_, orient_err_, orient_weight_ are kept
  //   GetAccuracy (:1573-1594)         msfm_point_accuracy_batch with ok_in = !is_bad_estimated_ (min_views 0: Triangulation
  //                                    has flagged the short tracks, :643): accuracy_errors_ is `errors`, points above
  //                                    th_outlier_ become is_bad_estimated_
  //   GPSRegistration2 (:917-983)      msfm_gps_register_points on the non-bad points, then every camera onto its GPS
  //                                    position with SetACPose
  // The ...Host forms are the literal walks over the object graph, one point at a time.
  void AbsoluteOrientationWithGPSGlobal();
  void GetAccuracy();
  void GetAccuracyHost();
  void GPSRegistration2();
  void GPSRegistration2Host();
  Vec3 gps_offset_;
  double th_outlier_ = 3.0;                  // slam_gps.cc:1587
  double orient_scale_ = 0.0, orient_err_ = 0.0;
  Mat3 orient_R_;
  Vec3 orient_t_;
  std::vector<double> orient_weight_;
  std::vector<double> accuracy_errors_, accuracy_mse_;   // per point: e_avg (1000.0 where there is none), e_mse
  std::vector<int> accuracy_n_obs_;
  int count_outliers_ = 0;
  // slam_gps.h:135, set to 0.5 by SLAMGPS::SLAMGPS (slam_gps.cc:55): the SLAM observations are stored at full resolution,
  // (px - cx) / resize_ratio (:199), and step 1's pixel thresholds scale with it (:316-317)
  double resize_ratio = 0.5;
  bool minimizer_progress_to_stdout_ = true; // slam_gps.cc:682
  msfm_ba_summary summary_;
  std::vector<msfm_ba_iteration> iterations_;
};

// The kNN + ratio-test part of FineMatchingGraph::BuildMatchGraph (fine_matching_graph.cc:87-133),
// one batched call for a whole pair list.  matches_good/all[p] = (ptid1 in idx1, ptid2 in idx2).
struct PairMatches { int idx1, idx2; std::vector<std::pair<int, int>> matches_good, matches_all; };
std::vector<PairMatches> MatchImagePairs(const std::vector<std::vector<float>>& descriptors /*[image][n*128]*/,
                                         const std::vector<std::pair<int, int>>& pairs, float thRatio_good = 0.6f,
                                         float thRatio_all = 0.85f);

// Geometric verification (SfM/src/utils/geo_verification.h/.cc:30-79).  cv::Point2f / cv::Mat become Point2f / Mat3.
struct Point2f { float x = 0, y = 0; };
class GeoVerification {
 public:
  // cv::findFundamentalMat(FM_RANSAC, 3.0) + the 30-point / 30-inlier gates            (geo_verification.cc:30-58)
  static bool GeoVerificationFundamental(std::vector<Point2f>& pt1, std::vector<Point2f>& pt2, std::vector<int>& match_inliers,
                                         Mat3& FMatrix);
  // closed-form filter of a second match set with a given F                            (geo_verification.cc:60-79)
  static bool GeoVerificationFundamental(std::vector<Point2f>& pt1, std::vector<Point2f>& pt2, Mat3 FMatrix,
                                         std::vector<int>& match_inliers);
};
// The verification half of FineMatchingGraph::BuildMatchGraph (fine_matching_graph.cc:138-187) for every pair in two
// batched calls: RANSAC on the "good" matches, then the F filter on the "all" matches of the pairs that passed.
// keypoints[image][feature] are the centred pixel coordinates of database.cc:522-527.
// Returns per pair the surviving matches_all entries (empty when the pair failed: nothing is written for it).
std::vector<std::vector<std::pair<int, int>>> VerifyPairs(const std::vector<PairMatches>& matches,
                                                          const std::vector<std::vector<Point2f>>& keypoints);

// Which image pairs are matched at all, matching_type "feature" (SfM/src/graph/initial_matching_graph.h/.cc:164-294 with the
// inverted-file similarity of similarity_graph.cc:47-117).  words[i] = Database::words_id_[i] (empty: `<i>_words` is empty),
// num_words = Database::max_words_id_, keypoints[image][feature] = the centred pixels of database.cc:522-527.
// BuildInitialMatchGraphFeature is one msfm_wordset_create plus msfm_pair_select per rows_per_call_ images;
// MatchGraphFeatureHost walks the reference's loops (std::map per image, one hypothesis after the other) and hands the joined
// points of the same rows_per_call_ images to one msfm_fundamental_ransac_batch, so that every hypothesis keeps its sampler
// index: both fill the same members with the same values (tests/pairselect_host_check.cc).  Ties the reference leaves to
// std::sort are fixed as msfm.h says: the lowest feature of a repeated word, the lower image id at equal similarity.
class InitialMatchingGraph {
 public:
  int rows_per_call_ = 64;   // decides which samples a pair sees: keep it when results are to be reproduced
  int max_hypotheses_ = 0;   // 0: th_num_match of :168-169
  std::vector<std::vector<int>> match_graph_init;              // :47: per image the images to match it against
  std::vector<std::vector<int>> hyp_img_, n_init_, n_inliers_;  // per image and slot: set_idx2, matches_init.size(), inliers
  std::vector<std::vector<uint8_t>> verdict_;                  // per image and slot: 0 kept, 1 / 2 / 3 = the gate that refused
  void BuildInitialMatchGraphFeature(const std::vector<std::vector<int>>& words, int num_words,
                                     const std::vector<std::vector<Point2f>>& keypoints);
  void MatchGraphFeatureHost(const std::vector<std::vector<int>>& words, int num_words,
                             const std::vector<std::vector<Point2f>>& keypoints);
 private:
  void Reset(int n, int K);
};

// Pose initialisers (SfM/src/orientation/{absolute,relative}_pose_estimation.h).  Eigen::Vector3d / Vector2d / Matrix3d
// become Vec3 / Vec2 / Mat3; RTPoseRelative has the fields of RTPose (basic_structs.h:126-138).
typedef RTPose RTPoseRelative;
class AbsolutePoseEstimation {
 public:
  // EPnP RANSAC (200 samples of 4 correspondences) + per-point reprojection errors   (absolute_pose_estimation.cc:42-58)
  static bool AbsolutePoseWithFocalLength(std::vector<Vec3>& pts_w, std::vector<Vec2>& pts_2d, double f, RTPose& pose_absolute,
                                          std::vector<double>& errors, double& avg_error);
};
class RelativePoseEstimation {
 public:
  // five-point RANSAC on points / f, then the pose from the best essential matrix     (relative_pose_estimation.cc:91-120)
  static bool RelativePoseWithFocalLength(std::vector<Vec2>& pts_ref, std::vector<Vec2>& pts_cur, double f_ref, double f_cur,
                                          RTPoseRelative& pose_relative);
  // normalised eight-point F RANSAC on centred pixels, both focal lengths from F, then the pose from E = K2 F K1
  //                                                                                    (relative_pose_estimation.cc:29-83)
  static bool RelativePoseWithoutFocalLength(std::vector<Vec2>& pts_ref, std::vector<Vec2>& pts_cur, double& f_ref, double& f_cur,
                                             RTPoseRelative& pose_relative);
};
// RelativePoseWithoutFocalLength for several candidate seed pairs at once: the reference walks its sorted pair list one by
// one until a pair reconstructs (sfm_incremental.cc:224-415), the host can hand over the top K instead.  ok[p] is the
// per-pair return value; f_ref, f_cur and poses of a failed pair are zero.  Pair p draws the samples of pair index p: a
// single-pair call equals entry 0 of a batch.
void RelativePoseWithoutFocalLengthBatch(const std::vector<std::vector<Vec2>>& pts_ref, const std::vector<std::vector<Vec2>>& pts_cur,
                                         std::vector<double>& f_ref, std::vector<double>& f_cur, std::vector<RTPoseRelative>& poses,
                                         std::vector<uint8_t>& ok);
// Many images / pairs in one call each (the batched form the GPU wants; same results as the per-item calls above).
void AbsolutePoseBatch(const std::vector<std::vector<Vec3>>& pts_w, const std::vector<std::vector<Vec2>>& pts_2d, const std::vector<double>& f,
                       std::vector<RTPose>& poses, std::vector<std::vector<double>>& errors, std::vector<double>& avg_error);
// AbsolutePoseWithoutFocalLength for many images (absolute_pose_estimation.cc:28-40): the EPNPF focal sweep around f_estimated
// (the reference: 1.2 * max(w, h), sfm_incremental.cc:675); f_out = the focal length it keeps, for SetFocalLength (:704).
void AbsolutePoseWithoutFocalLengthBatch(const std::vector<std::vector<Vec3>>& pts_w, const std::vector<std::vector<Vec2>>& pts_2d,
                                         const std::vector<double>& f_estimated, std::vector<double>& f_out, std::vector<RTPose>& poses,
                                         std::vector<std::vector<double>>& errors, std::vector<double>& avg_error);

// The per-image feature file of the extraction stage (Database::WriteoutImageFeature / ReadinImageFeatures,
// SfM/src/database.cc:490-541, :352-423): header, centred keypoints, raw descriptors.  cv::Mat -> flat float rows.
struct ImageInfo {  // basic_structs.h ImageInfo
  int rows = 0, cols = 0;
  float zoom_ratio = 1.f, f_mm = 0.f, f_pixel = 0.f, gps_latitude = 0.f, gps_longitude = 0.f;
  std::string cam_maker, cam_model;
};
bool WriteoutImageFeature(const std::string& output_fold, int idx, const ImageInfo& info, const std::vector<Point2f>& keypoints_px,
                          const std::vector<float>& descriptors /*[n][cols]*/, int desc_cols = 128);
bool ReadinImageFeatures(const std::string& output_fold, int idx, ImageInfo& info, std::vector<Point2f>& keypoints_centred,
                         std::vector<float>& descriptors, int& desc_cols);

// Track building, the data association of SLAMGPS::Triangulation (slam_gps.cc:565-635): walk the match graph in the
// reference's order (idx1 ascending, idx2 ascending over match_graph[idx1][idx2] > 0, matches read back with
// QueryMatch) and grow points greedily - msfm_tracks_build_device keeps the std::map::insert semantics.  Returns the new
// points with their observations attached (AddObservation(cam, x, y, image id), as :600-603 keys them).
std::vector<Point3D> BuildTracks(const std::string& output_fold, const std::vector<std::vector<int>>& match_graph,
                                 std::vector<Camera>& cams, const std::vector<std::vector<Vec2>>& keypoints);

// The reference's stage boundary is a set of files: per image `<idx1>_match` (binary records
// int idx2, int n, int[2n]) and `graph_matching.txt`.  Same bytes as FineMatchingGraph::WriteOutMatches /
// WriteOutMatchGraph (fine_matching_graph.cc:247-292) and Graph::QueryMatch (graph.cc:92-137).
void WriteOutMatches(const std::string& output_fold, int idx1, int idx2, const std::vector<std::pair<int, int>>& matches);
void WriteOutMatchGraph(const std::string& output_fold, const std::vector<std::vector<int>>& match_graph);
void QueryMatch(const std::string& output_fold, int idx, std::vector<int>& image_ids,
                std::vector<std::vector<std::pair<int, int>>>& match_pts);

}  // namespace objectsfm
