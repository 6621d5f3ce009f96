// Sequential restatement of the loop body of IncrementalSfM::FindSeedPairThenReconstruct (SfM/src/sfm_incremental.cc:235-390)
// for tests/seed_ref.py: one hypothesis after the other - QueryMatch, the keypoint gather, the camera set-up, a two-view
// Point3D::Trianglate2 per match (tests/point3d_ref.h), the two gates, the winner.  The relative poses are INPUT (tests/seed_data.py gets them from oracle.relpose_5pt and tests/relposef_ref.cpp on the points sr_gather returns).
// Built with g++ -O2 -ffp-contract=off: + - * / sqrt only, so the library's seed.hip must agree bit for bit.
#include <cmath>
#include <cstdint>
#include <vector>

#include "point3d_ref.h"   // Cam, Obs, trianglate2

namespace {

// Graph::QueryMatch(i1, i2): the stored matches of that pair, or none
void query_match(int n_pairs, const int* pair_img, const int* match_off, int i1, int i2, int* first, int* count) {
  *first = 0; *count = 0;
  for (int p = 0; p < n_pairs; p++)
    if (pair_img[2 * p] == i1 && pair_img[2 * p + 1] == i2) { *first = match_off[p]; *count = match_off[p + 1] - match_off[p]; return; }
}

}  // namespace

// The matches of every hypothesis as the pose estimators get them (:294-304): n_matches [n_hyp], pts1 / pts2 [sum][2] in
// hypothesis order (capacity: the caller sizes them from a first call with pts1 == nullptr).
extern "C" int sr_gather(int n_pairs, const int* pair_img, const int* match_off, const int* matches, const int* feat_off, const float* keypoints,
                         int n_hyp, const int* hyp_img, int* n_matches, double* pts1, double* pts2) {
  long e = 0;
  for (int h = 0; h < n_hyp; h++) {
    const int i1 = hyp_img[2 * h], i2 = hyp_img[2 * h + 1];
    int m0, cnt;
    query_match(n_pairs, pair_img, match_off, i1, i2, &m0, &cnt);
    n_matches[h] = cnt;
    if (pts1)
      for (int j = 0; j < cnt; j++, e++) {
        const long a = feat_off[i1] + matches[2 * (long)(m0 + j)], b = feat_off[i2] + matches[2 * (long)(m0 + j) + 1];
        pts1[2 * e] = (double)keypoints[2 * a]; pts1[2 * e + 1] = (double)keypoints[2 * a + 1];
        pts2[2 * e] = (double)keypoints[2 * b]; pts2[2 * e + 1] = (double)keypoints[2 * b + 1];
      }
  }
  return 0;
}

// pose_ok_in / R_in [n][9] / t_in [n][3]: what the arm's estimator returned for the hypothesis; f_in [n][2]: the two focal
// lengths RelativePoseWithoutFocalLength returned (eight-point arm only).  Point outputs have capacity sum of n_matches.
extern "C" int sr_reconstruct(int n_pairs, const int* pair_img, const int* match_off, const int* matches, const int* feat_off,
                              const float* keypoints, int n_hyp, const int* hyp_img, const double* cam_fk, const uint8_t* same_model,
                              const uint8_t* pose_ok_in, const double* R_in, const double* t_in, const double* f_in, double th_mse_reprojection,
                              double th_angle_small, int th_seedpair_structures, uint8_t* arm, uint8_t* pose_ok, uint8_t* pass, int* n_matches,
                              double* f, double* R, double* t, double* c, int* pt_off, int* pt_match, double* X, double* mse, int* winner) {
  const double cos_min = std::cos(th_angle_small);
  *winner = -1;
  pt_off[0] = 0;
  for (int h = 0; h < n_hyp; h++) {
    const int i1 = hyp_img[2 * h], i2 = hyp_img[2 * h + 1];
    int m0, cnt;
    query_match(n_pairs, pair_img, match_off, i1, i2, &m0, &cnt);   // :249
    n_matches[h] = cnt;
    Cam cam0, cam1;
    for (int k = 0; k < 9; k++) cam0.R[k] = (k % 4 == 0) ? 1.0 : 0.0;   // :290
    for (int k = 0; k < 3; k++) { cam0.t[k] = 0.0; cam0.c[k] = 0.0; }
    for (int k = 0; k < 3; k++) { cam0.fk[k] = cam_fk[6 * h + k]; cam1.fk[k] = cam_fk[6 * h + 3 + k]; }
    const bool five = cam0.fk[0] != 0.0 && cam1.fk[0] != 0.0;          // :307
    arm[h] = five ? 5 : 8;
    pose_ok[h] = pose_ok_in[h]; pass[h] = 0;
    f[2 * h] = cam0.fk[0]; f[2 * h + 1] = cam1.fk[0];
    for (int k = 0; k < 9; k++) R[9 * h + k] = 0.0;
    for (int k = 0; k < 3; k++) { t[3 * h + k] = 0.0; c[3 * h + k] = 0.0; }
    pt_off[h + 1] = pt_off[h];
    if (!pose_ok_in[h]) continue;                                      // :313, :321
    if (!five) {                                                       // :324-332
      const double f1 = f_in[2 * h], f2 = f_in[2 * h + 1];
      if (same_model[h]) { cam0.fk[0] = (f1 + f2) / 2.0; cam1.fk[0] = cam0.fk[0]; }
      else { cam0.fk[0] = f1; cam1.fk[0] = f2; }
    }
    for (int k = 0; k < 9; k++) cam1.R[k] = R_in[9 * h + k];           // :334, Camera::SetRTPose
    for (int k = 0; k < 3; k++) cam1.t[k] = t_in[3 * h + k];
    for (int k = 0; k < 3; k++) cam1.c[k] = -(cam1.R[k] * cam1.t[0] + cam1.R[3 + k] * cam1.t[1] + cam1.R[6 + k] * cam1.t[2]);
    f[2 * h] = cam0.fk[0]; f[2 * h + 1] = cam1.fk[0];
    for (int k = 0; k < 9; k++) R[9 * h + k] = cam1.R[k];
    for (int k = 0; k < 3; k++) { t[3 * h + k] = cam1.t[k]; c[3 * h + k] = cam1.c[k]; }
    int e = pt_off[h];
    for (int j = 0; j < cnt; j++) {                                    // :344-374
      const long a = feat_off[i1] + matches[2 * (long)(m0 + j)], b = feat_off[i2] + matches[2 * (long)(m0 + j) + 1];
      std::vector<Obs> obs;
      obs.push_back(Obs{&cam0, (double)keypoints[2 * a], (double)keypoints[2 * a + 1]});
      obs.push_back(Obs{&cam1, (double)keypoints[2 * b], (double)keypoints[2 * b + 1]});
      double Xp[3], m, cs;
      if (trianglate2(obs, th_mse_reprojection, cos_min, Xp, &m, &cs) == 2) {
        pt_match[e] = j;
        X[3 * e] = Xp[0]; X[3 * e + 1] = Xp[1]; X[3 * e + 2] = Xp[2];
        mse[e] = m;
        e++;
      }
    }
    const int n_points = e - pt_off[h];
    pt_off[h + 1] = e;
    pass[h] = !(n_points < th_seedpair_structures || n_points < cnt / 5);   // :380-381
    if (pass[h] && *winner < 0) *winner = h;
  }
  return 0;
}
