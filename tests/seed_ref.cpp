// Sequential restatement of the loop body of IncrementalSfM::FindSeedPairThenReconstruct (SfM/src/sfm_incremental.cc:235-390)
// for tests/seed_ref.py: one hypothesis after the other - QueryMatch, the keypoint gather, the camera set-up, a two-view
// Point3D::Trianglate2 per match (structure.cc:211-265, :267-300, :325-355), the two gates, the winner.  The relative poses
// are INPUT (tests/seed_data.py gets them from oracle.relpose_5pt and tests/relposef_ref.cpp on the points sr_gather returns).
// Built with g++ -O2 -ffp-contract=off: + - * / sqrt only, so the library's seed.hip must agree bit for bit.
#include <cmath>
#include <cstdint>
#include <vector>

namespace {

struct Cam { double R[9], t[3], c[3], fk[3]; };
struct Obs { const Cam* cam; double x, y; };

// Graph::QueryMatch(i1, i2): the stored matches of that pair, or none
void query_match(int n_pairs, const int* pair_img, const int* match_off, int i1, int i2, int* first, int* count) {
  *first = 0; *count = 0;
  for (int p = 0; p < n_pairs; p++)
    if (pair_img[2 * p] == i1 && pair_img[2 * p + 1] == i2) { *first = match_off[p]; *count = match_off[p + 1] - match_off[p]; return; }
}

// Point3D::Reprojection, structure.cc:267-300
double reprojection(const std::vector<Obs>& obs, const double* X) {
  double mse = 0.0;
  int count = 0;
  for (const Obs& o : obs) {
    const double* R = o.cam->R;
    const double* tt = o.cam->t;
    const double* fk = o.cam->fk;
    const double pc0 = R[0] * X[0] + R[1] * X[1] + R[2] * X[2] + tt[0];
    const double pc1 = R[3] * X[0] + R[4] * X[1] + R[5] * X[2] + tt[1];
    const double pc2 = R[6] * X[0] + R[7] * X[1] + R[8] * X[2] + tt[2];
    if (pc2 < 0) return 100000.0;
    const double x = pc0 / pc2, y = pc1 / pc2;
    const double r2 = x * x + y * y;
    const double distortion = 1.0 + r2 * (fk[1] + fk[2] * r2);
    const double u = fk[0] * distortion * x, v = fk[0] * distortion * y;
    const double du = u - o.x, dv = v - o.y;
    mse += du * du + dv * dv;
    count++;
  }
  return mse / count;
}

// Point3D::SufficientTriangulationAngle, structure.cc:325-355
bool sufficient_angle(const std::vector<Obs>& obs, const double* X, double cos_min) {
  for (size_t i = 0; i + 1 < obs.size(); i++) {
    const double* ci = obs[i].cam->c;
    double a[3] = {X[0] - ci[0], X[1] - ci[1], X[2] - ci[2]};
    const double na = std::sqrt(a[0] * a[0] + a[1] * a[1] + a[2] * a[2]);
    a[0] /= na; a[1] /= na; a[2] /= na;
    for (size_t j = i + 1; j < obs.size(); j++) {
      const double* cj = obs[j].cam->c;
      double d[3] = {X[0] - cj[0], X[1] - cj[1], X[2] - cj[2]};
      const double nd = std::sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
      d[0] /= nd; d[1] /= nd; d[2] /= nd;
      if (a[0] * d[0] + a[1] * d[1] + a[2] * d[2] < cos_min) return true;
    }
  }
  return false;
}

// Point3D::Trianglate2, structure.cc:211-265: sum of (I - d d^T) over the rays in homogeneous 4 x 4 form, Eigen::LLT
bool trianglate2(const std::vector<Obs>& obs, double th_error, double cos_min, double* X, double* mse) {
  double A[16], bv[4] = {0, 0, 0, 0};
  for (int k = 0; k < 16; k++) A[k] = 0.0;
  for (const Obs& ob : obs) {
    const double* R = ob.cam->R;
    const double* o = ob.cam->c;
    const double f = ob.cam->fk[0];
    double dw[3] = {R[0] * ob.x + R[3] * ob.y + R[6] * f, R[1] * ob.x + R[4] * ob.y + R[7] * f, R[2] * ob.x + R[5] * ob.y + R[8] * f};
    const double n = std::sqrt(dw[0] * dw[0] + dw[1] * dw[1] + dw[2] * dw[2]);
    dw[0] /= n; dw[1] /= n; dw[2] /= n;
    const double dh[4] = {dw[0], dw[1], dw[2], 0.0};
    const double oh[4] = {o[0], o[1], o[2], 1.0};
    for (int r = 0; r < 4; r++) {
      double acc = 0.0;
      for (int q = 0; q < 4; q++) {
        const double at = (r == q ? 1.0 : 0.0) - dh[r] * dh[q];
        A[r * 4 + q] += at;
        acc += at * oh[q];
      }
      bv[r] += acc;
    }
  }
  double L[16];
  for (int k = 0; k < 16; k++) L[k] = 0.0;
  bool pd = true;
  for (int j = 0; j < 4; j++) {
    double d = A[j * 4 + j];
    for (int k = 0; k < j; k++) d -= L[j * 4 + k] * L[j * 4 + k];
    if (!(d > 0.0)) pd = false;
    L[j * 4 + j] = std::sqrt(d);
    for (int i = j + 1; i < 4; i++) {
      double s = A[i * 4 + j];
      for (int k = 0; k < j; k++) s -= L[i * 4 + k] * L[j * 4 + k];
      L[i * 4 + j] = s / L[j * 4 + j];
    }
  }
  if (!pd) return false;
  double y[4], x[4];
  for (int i = 0; i < 4; i++) {
    double s = bv[i];
    for (int k = 0; k < i; k++) s -= L[i * 4 + k] * y[k];
    y[i] = s / L[i * 4 + i];
  }
  for (int i = 3; i >= 0; i--) {
    double s = y[i];
    for (int k = i + 1; k < 4; k++) s -= L[k * 4 + i] * x[k];
    x[i] = s / L[i * 4 + i];
  }
  X[0] = x[0] / x[3]; X[1] = x[1] / x[3]; X[2] = x[2] / x[3];
  *mse = reprojection(obs, X);
  return !(std::sqrt(*mse) > th_error || !sufficient_angle(obs, X, cos_min));
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
      double Xp[3], m;
      if (trianglate2(obs, th_mse_reprojection, cos_min, Xp, &m)) {
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
