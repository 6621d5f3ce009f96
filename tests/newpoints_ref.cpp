// Sequential restatement of IncrementalSfM::GenerateNew3DPoints (SfM/src/sfm_incremental.cc:755-915) for
// tests/newpoints_ref.py: per new camera the walk over its visible cameras (:766-894), QueryMatch, the angle threshold of the
// pair (:780-784), the candidate test (:804-808), a two-view Point3D::Trianglate2 per candidate
// (tests/point3d_ref.h), the sort by the mse truncated to int (:829, :897; stable here) and Camera::AddPoints' std::map::insert (:908-909).  Built with g++ -O2 -ffp-contract=off: + - * / sqrt only, so the library's newpoints.hip must agree bit for bit.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <map>
#include <utility>
#include <vector>

#include "point3d_ref.h"   // Cam, Obs, trianglate2

namespace {

// Graph::QueryMatch(i1, i2): the stored matches of that pair, or none
void query_match(int n_pairs, const int* pair_img, const int* match_off, int i1, int i2, int* first, int* count) {
  *first = 0; *count = 0;
  for (int p = 0; p < n_pairs; p++)
    if (pair_img[2 * p] == i1 && pair_img[2 * p + 1] == i2) { *first = match_off[p]; *count = match_off[p + 1] - match_off[p]; return; }
}

struct NewPt { int cam2, f1, f2, vis_entry, pt_match, key; double X[3], mse; };

}  // namespace

// feat_off [n_images + 1]: first keypoint row of an image; feat_point: camera c starts at the sum of the feature counts of the
// cameras before it.  Point outputs have the capacity of the walk (sum of n_matches over all entries); the per-candidate
// diagnostics diag_* (each may be NULL; same capacity, *n_diag rows, in walk order) are what tests/test_newpoints_ref.py
// asserts its margins on: the state of Trianglate2 (0 / 1 / 2), sqrt(mse), the ray cosine and the cosine it was compared with.
extern "C" int nr_new_points(int n_pairs, const int* pair_img, const int* match_off, const int* matches, const int* feat_off,
                             const float* keypoints, int n_cams, const int* cam_img, const int* feat_point, const double* cam_R,
                             const double* cam_t, const double* cam_c, const double* cam_fk, int n_new, const int* new_cam, const int* vis_off,
                             const int* vis_cam, double th_mse_reprojection, double th_angle_small, double th_angle_large, int th_matches_large,
                             int* pt_off, int* cam2, int* feat1, int* feat2, int* vis_entry, int* pt_match, double* X, double* mse, uint8_t* takes1,
                             uint8_t* takes2, int* n_matches, uint8_t* large, int* n_candidates, int* n_accepted, int* n_diag, int* diag_state,
                             double* diag_rmse, double* diag_cos, double* diag_cos_min) {
  const double cos_small = std::cos(th_angle_small), cos_large = std::cos(th_angle_large);
  std::vector<Cam> cams(n_cams);
  std::vector<long> cam_fo(n_cams + 1, 0);
  for (int c = 0; c < n_cams; c++) {
    for (int k = 0; k < 9; k++) cams[c].R[k] = cam_R[9 * c + k];
    for (int k = 0; k < 3; k++) { cams[c].t[k] = cam_t[3 * c + k]; cams[c].c[k] = cam_c[3 * c + k]; cams[c].fk[k] = cam_fk[3 * c + k]; }
    const int im = cam_img[c];
    cam_fo[c + 1] = cam_fo[c] + (feat_off[im + 1] - feat_off[im]);
  }
  int nd = 0;
  pt_off[0] = 0;
  for (int k = 0; k < n_new; k++) {
    const int c1 = new_cam[k], i1 = cam_img[c1];
    std::vector<NewPt> pts_new;
    for (int q = vis_off[k]; q < vis_off[k + 1]; q++) {                    // :766
      const int c2 = vis_cam[q];
      n_matches[q] = 0; large[q] = 0; n_candidates[q] = 0; n_accepted[q] = 0;
      if (c2 == c1) continue;                                              // :769
      const int i2 = cam_img[c2];
      int m0, cnt;
      query_match(n_pairs, pair_img, match_off, i1, i2, &m0, &cnt);        // :777
      n_matches[q] = cnt;
      const bool lg = cnt > th_matches_large;                              // :780-784
      large[q] = lg ? 1 : 0;
      const double cos_min = lg ? cos_large : cos_small;
      for (int j = 0; j < cnt; j++) {
        const int f1 = matches[2 * (long)(m0 + j)], f2 = matches[2 * (long)(m0 + j) + 1];
        if (feat_point[cam_fo[c1] + f1] >= 0 || feat_point[cam_fo[c2] + f2] >= 0) continue;   // :804-808
        n_candidates[q]++;
        const long a = feat_off[i1] + f1, b = feat_off[i2] + f2;
        std::vector<Obs> obs;
        obs.push_back(Obs{&cams[c1], (double)keypoints[2 * a], (double)keypoints[2 * a + 1]});   // :811-818
        obs.push_back(Obs{&cams[c2], (double)keypoints[2 * b], (double)keypoints[2 * b + 1]});
        NewPt p{c2, f1, f2, q - vis_off[k], j, 0, {0, 0, 0}, 0.0};
        double cs = 0.0;
        const int st = trianglate2(obs, th_mse_reprojection, cos_min, p.X, &p.mse, &cs);          // :821
        if (diag_state) diag_state[nd] = st;
        if (diag_rmse) diag_rmse[nd] = st ? std::sqrt(p.mse) : 0.0;
        if (diag_cos) diag_cos[nd] = st ? cs : 0.0;
        if (diag_cos_min) diag_cos_min[nd] = cos_min;
        nd++;
        if (st == 2) {
          p.key = (int)p.mse;                                              // :829, pair<Point3DNew*, int>
          pts_new.push_back(p);
          n_accepted[q]++;
        }
      }
    }
    std::stable_sort(pts_new.begin(), pts_new.end(), [](const NewPt& l, const NewPt& r) { return l.key < r.key; });   // :897
    std::map<int, int> pts1;                       // cams_[c1]->pts_ of this round: local feature -> new point
    std::map<std::pair<int, int>, int> pts2;       // the same of every visible camera
    int e = pt_off[k];
    for (size_t i = 0; i < pts_new.size(); i++, e++) {                     // :899-910
      const NewPt& p = pts_new[i];
      cam2[e] = p.cam2; feat1[e] = p.f1; feat2[e] = p.f2; vis_entry[e] = p.vis_entry; pt_match[e] = p.pt_match;
      X[3 * e] = p.X[0]; X[3 * e + 1] = p.X[1]; X[3 * e + 2] = p.X[2];
      mse[e] = p.mse;
      takes1[e] = pts1.insert(std::make_pair(p.f1, (int)i)).second ? 1 : 0;
      takes2[e] = pts2.insert(std::make_pair(std::make_pair(p.cam2, p.f2), (int)i)).second ? 1 : 0;
    }
    pt_off[k + 1] = e;
  }
  if (n_diag) *n_diag = nd;
  return 0;
}
