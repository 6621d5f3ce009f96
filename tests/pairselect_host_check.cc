// The C++ host's InitialMatchingGraph::BuildInitialMatchGraphFeature (msfm_wordset_create + msfm_pair_select per chunk of
// images) against its literal walk MatchGraphFeatureHost (std::map per image, msfm_fundamental_ransac_batch on the same
// problem lists): fails when hypotheses, joined-match counts, inlier counts, verdicts or match_graph_init differ.
//   pairselect_host_check <in.bin> <out.bin>
// in.bin : int32 n, num_words, rows_per_call, max_hypotheses; int32 n_features[n]; int32 has_words[n]; int32 word ids of all
//          features, images back to back; float32 keypoints [sum][2]
// out.bin: int32 K; per image int32 hyp_img[K], n_init[K], n_inliers[K], verdict[K]
// Built with -DPAIRSELECT_ARGS_ONLY it needs neither the library nor a device: it runs the argument checks of
// metricsfm_amd/csrc/pairsel_args.h, the code msfm_wordset_create / msfm_pair_select refuse with, on bad and good input.
#include <cstdio>
#include <cstring>
#include <fstream>
#include <string>
#include <vector>

#include "../metricsfm_amd/csrc/pairsel_args.h"

static int fail(const char* what) {
  std::printf("pairselect_host_check FAILED: %s\n", what);
  return 1;
}

static int check_args() {
  const int nf[3] = {2, 0, 3};
  const uint8_t hw[3] = {1, 0, 1};
  int32_t words[5] = {4, 10, 7, 0, 10};
  const float kp[10] = {0};
  int K = -1;
  long total = -1;
  auto create = [&](int n, const int* f, const uint8_t* h, const int32_t* w, int num_words, const float* k, int max_hyp) {
    return pairsel_check_create(n, f, h, w, num_words, k, max_hyp, &K, &total);
  };
  if (!create(3, nf, hw, words, 10, kp, 0).empty() || K != 2 || total != 5) return fail("a good set is refused");
  if (!create(3, nf, hw, words, 10, kp, 1).empty() || K != 1) return fail("max_hypotheses = 1");
  if (create(1, nf, hw, words, 10, kp, 0).empty()) return fail("n_images = 1 accepted");
  if (create(3, nullptr, hw, words, 10, kp, 0).empty() || create(3, nf, nullptr, words, 10, kp, 0).empty()) return fail("null counts accepted");
  if (create(3, nf, hw, nullptr, 10, kp, 0).empty() || create(3, nf, hw, words, 10, nullptr, 0).empty()) return fail("null arrays accepted");
  if (create(3, nf, hw, words, 9, kp, 0).empty()) return fail("word id num_words + 1 accepted");
  if (create(3, nf, hw, words, 10, kp, 3).empty() || create(3, nf, hw, words, 10, kp, -1).empty()) return fail("max_hypotheses out of range accepted");
  words[0] = -1;
  if (create(3, nf, hw, words, 10, kp, 0).empty()) return fail("negative word id accepted");
  words[0] = 4;
  const int nf_bad[3] = {2, -1, 3};
  if (create(3, nf_bad, hw, words, 10, kp, 0).empty()) return fail("negative feature count accepted");
  msfm_pair_select_options o;
  std::memset(&o, 0, sizeof o);
  o.th_init_matches = 30; o.th_inliers = 20; o.fransac.threshold = 3.0; o.fransac.max_iterations = 2000;
  int Ks = -1;
  if (!pairsel_check_select(12, 11, 0, 12, &o, &Ks).empty() || Ks != 11) return fail("all rows refused");
  if (!pairsel_check_select(12, 11, 5, 7, &o, &Ks).empty()) return fail("the last chunk refused");
  if (pairsel_check_select(12, 11, 5, 8, &o, &Ks).empty() || pairsel_check_select(12, 11, -1, 2, &o, &Ks).empty() ||
      pairsel_check_select(12, 11, 0, 0, &o, &Ks).empty() || pairsel_check_select(12, 11, 12, 1, &o, &Ks).empty() ||
      pairsel_check_select(12, 11, 1, 0x7fffffff, &o, &Ks).empty())
    return fail("rows out of range accepted");
  o.max_hypotheses = 4;
  if (!pairsel_check_select(12, 11, 0, 12, &o, &Ks).empty() || Ks != 4) return fail("max_hypotheses = 4");
  o.max_hypotheses = 12;
  if (pairsel_check_select(12, 11, 0, 12, &o, &Ks).empty()) return fail("max_hypotheses above the set's accepted");
  o.max_hypotheses = 0; o.fransac.max_iterations = 0;
  if (pairsel_check_select(12, 11, 0, 12, &o, &Ks).empty()) return fail("max_iterations = 0 accepted");
  const int ks[3] = {pairsel_rule_k(12), pairsel_rule_k(2500), pairsel_rule_k(6000)};
  if (ks[0] != 11 || ks[1] != 250 || ks[2] != 500) return fail("the rule for K");
  std::printf("pairselect_host_check ok: argument checks\n");
  return 0;
}

#ifdef PAIRSELECT_ARGS_ONLY
int main() { return check_args(); }
#else
#include "objectsfm.h"

using namespace objectsfm;

int main(int argc, char** argv) {
  if (argc < 3) return fail("usage: pairselect_host_check <in.bin> <out.bin>");
  if (check_args()) return 1;
  std::ifstream in(argv[1], std::ios::binary);
  if (!in) return fail("cannot open the input");
  int head[4];
  in.read((char*)head, sizeof head);
  const int n = head[0], num_words = head[1];
  std::vector<int> nf(n), hw(n);
  in.read((char*)nf.data(), sizeof(int) * n);
  in.read((char*)hw.data(), sizeof(int) * n);
  std::vector<std::vector<int>> words(n);
  for (int i = 0; i < n; i++) {
    std::vector<int> w(nf[i]);
    in.read((char*)w.data(), sizeof(int) * (size_t)nf[i]);
    if (hw[i]) words[i] = w;
  }
  std::vector<std::vector<Point2f>> kp(n);
  for (int i = 0; i < n; i++) {
    kp[i].resize(nf[i]);
    in.read((char*)kp[i].data(), sizeof(Point2f) * (size_t)nf[i]);
  }
  if (!in) return fail("short input");
  InitialMatchingGraph dev, host;
  dev.rows_per_call_ = host.rows_per_call_ = head[2];
  dev.max_hypotheses_ = host.max_hypotheses_ = head[3];
  dev.BuildInitialMatchGraphFeature(words, num_words, kp);
  host.MatchGraphFeatureHost(words, num_words, kp);
  if (dev.hyp_img_ != host.hyp_img_) return fail("hypotheses differ");
  if (dev.n_init_ != host.n_init_) return fail("joined-match counts differ");
  if (dev.n_inliers_ != host.n_inliers_) return fail("inlier counts differ");
  if (dev.verdict_ != host.verdict_) return fail("verdicts differ");
  if (dev.match_graph_init != host.match_graph_init) return fail("match_graph_init differs");
  const int K = n ? (int)dev.hyp_img_[0].size() : 0;
  std::ofstream out(argv[2], std::ios::binary);
  out.write((const char*)&K, sizeof K);
  int kept = 0;
  for (int i = 0; i < n; i++) {
    std::vector<int> ver(dev.verdict_[i].begin(), dev.verdict_[i].end());
    out.write((const char*)dev.hyp_img_[i].data(), sizeof(int) * K);
    out.write((const char*)dev.n_init_[i].data(), sizeof(int) * K);
    out.write((const char*)dev.n_inliers_[i].data(), sizeof(int) * K);
    out.write((const char*)ver.data(), sizeof(int) * K);
    kept += (int)dev.match_graph_init[i].size();
  }
  std::printf("pairselect_host_check ok: %d images, K = %d, %d pairs kept\n", n, K, kept);
  return 0;
}
#endif
