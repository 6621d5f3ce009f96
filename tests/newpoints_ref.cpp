// Sequential restatement of IncrementalSfM::GenerateNew3DPoints (SfM/src/sfm_incremental.cc:755-915) for
// tests/newpoints_ref.py: per new camera the walk over its visible cameras (:766-894), QueryMatch, the angle threshold of the
// pair (:780-784), the candidate test (:804-808), a two-view Point3D::Trianglate2 per candidate (structure.cc:211-265,
// :267-300, :325-355), the sort by the mse truncated to int (:829, :897; stable here) and Camera::AddPoints' std::map::insert
// (:908-909).  Built with g++ -O2 -ffp-contract=off: + - * / sqrt only, so the library's newpoints.hip must agree bit for bit.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <map>
#include <utility>
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

// Point3D::SufficientTriangulationAngle, structure.cc:325-355; *cos_out = the cosine of the (only) pair of rays
bool sufficient_angle(const std::vector<Obs>& obs, const double* X, double cos_min, double* cos_out) {
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
      const double cs = a[0] * d[0] + a[1] * d[1] + a[2] * d[2];
      *cos_out = cs;
      if (cs < cos_min) return true;
    }
  }
  return false;
}

// Point3D::Trianglate2, structure.cc:211-265: sum of (I - d d^T) over the rays in homogeneous 4 x 4 form, Eigen::LLT
// returns 0: LLT failed, 1: solved but rejected, 2: accepted
int trianglate2(const std::vector<Obs>& obs, double th_error, double cos_min, double* X, double* mse, double* cos_out) {
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
  if (!pd) return 0;
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
  const bool angle_ok = sufficient_angle(obs, X, cos_min, cos_out);
  return !(std::sqrt(*mse) > th_error || !angle_ok) ? 2 : 1;
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
