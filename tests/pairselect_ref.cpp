// One-thread C++ restatement of InitialMatchingGraph::match_graph_feature (SfM/src/graph/initial_matching_graph.cc:164-294)
// for scripts/pairselect_bench.py: the inverted-file similarity, the ranking, a std::map per image and the std::map walk per
// hypothesis as the reference writes them, and its GeoVerificationFundamental as one msfm_fundamental_ransac_batch call per
// hypothesis of 30 or more joined matches - one pair at a time, as a caller without the batched call would.
//   pairselect_ref <in.bin (tests/pairselect_data.py::write_image_set)> <max timed RANSAC calls>
// prints: restate_ms (everything before the verification), n_hyp, n_ransac (hypotheses that reach the verification),
// ransac_timed, ransac_ms (of the timed ones), kept (among the timed ones), n_init_total
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <map>
#include <vector>

#include "msfm.h"

static double now_ms() {
  return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

int main(int argc, char** argv) {
  if (argc < 3) return 2;
  std::ifstream in(argv[1], std::ios::binary);
  int head[4];
  in.read((char*)head, sizeof head);
  const int n = head[0], num_words = head[1], max_timed = std::atoi(argv[2]);
  std::vector<int> nf(n), hw(n);
  in.read((char*)nf.data(), sizeof(int) * n);
  in.read((char*)hw.data(), sizeof(int) * n);
  std::vector<std::vector<int>> words(n);
  for (int i = 0; i < n; i++) {
    std::vector<int> w(nf[i]);
    in.read((char*)w.data(), sizeof(int) * (size_t)nf[i]);
    if (hw[i]) words[i] = w;
  }
  std::vector<std::vector<float>> kp(n);
  for (int i = 0; i < n; i++) {
    kp[i].resize(2 * (size_t)nf[i]);
    in.read((char*)kp[i].data(), sizeof(float) * kp[i].size());
  }
  if (!in) return 3;
  const double t0 = now_ms();
  int K = head[3] > 0 ? head[3] : std::min(std::max(200, n / 10), n - 1);
  if (K > 500) K = 500;
  // inverted file and similarity
  std::vector<std::vector<int>> inverted(num_words);
  for (int i = 0; i < n; i++) {
    if (words[i].empty()) continue;
    std::vector<int> d = words[i];
    std::sort(d.begin(), d.end());
    int v = d[0];
    bool uniq = true;
    for (int x : d) {
      if (x != v) { if (uniq) inverted[v].push_back(i); v = x; uniq = true; }
      else uniq = false;
    }
  }
  std::vector<std::vector<float>> S(n, std::vector<float>(n, 0.f));
  for (auto& bin : inverted) {
    if (bin.size() > (size_t)(num_words / 100)) bin.clear();
    for (size_t a = 0; a + 1 < bin.size(); a++)
      for (size_t b = a + 1; b < bin.size(); b++) { S[bin[a]][bin[b]]++; S[bin[b]][bin[a]]++; }
  }
  // word tables
  std::vector<std::map<int, int>> table(n);
  for (int i = 0; i < n; i++) {
    if (words[i].empty()) continue;
    std::vector<std::pair<int, int>> d(words[i].size());
    for (size_t f = 0; f < d.size(); f++) d[f] = {(int)f, words[i][f]};
    std::stable_sort(d.begin(), d.end(), [](const std::pair<int, int>& a, const std::pair<int, int>& b) { return a.second < b.second; });
    int v = d[0].second;
    bool uniq = true;
    for (const auto& e : d) {
      if (e.second != v) { if (uniq) table[i].insert({e.second, e.first}); v = e.second; uniq = true; }
      else uniq = false;
    }
  }
  // hypotheses and joins
  std::vector<int> off(1, 0);
  std::vector<float> p1, p2;
  for (int i = 0; i < n; i++) {
    std::vector<std::pair<int, float>> order;
    for (int j = 0; j < n; j++) if (j != i) order.push_back({j, S[i][j]});
    std::stable_sort(order.begin(), order.end(), [](const std::pair<int, float>& a, const std::pair<int, float>& b) { return a.second > b.second; });
    for (int s = 0; s < K; s++) {
      const int j = order[s].first;
      int cnt = 0;
      for (const auto& e : table[i]) {
        const auto hit = table[j].find(e.first);
        if (hit == table[j].end()) continue;
        p1.push_back(kp[i][2 * e.second]); p1.push_back(kp[i][2 * e.second + 1]);
        p2.push_back(kp[j][2 * hit->second]); p2.push_back(kp[j][2 * hit->second + 1]);
        cnt++;
      }
      off.push_back(off.back() + cnt);
    }
  }
  const double restate_ms = now_ms() - t0;
  const int H = n * K;
  int n_ransac = 0;
  for (int h = 0; h < H; h++) n_ransac += off[h + 1] - off[h] >= 30;
  // the verification, one hypothesis per call
  msfm_ctx* ctx = nullptr;
  if (msfm_ctx_create(-1, &ctx) != MSFM_OK) return 4;
  msfm_fransac_options fo;
  msfm_fransac_default_options(&fo);
  int timed = 0, kept = 0;
  double ransac_ms = 0;
  for (int h = 0; h < H && timed < max_timed; h++) {
    const int cnt = off[h + 1] - off[h];
    if (cnt < 30) continue;
    const int o[2] = {0, cnt};
    double F[9];
    std::vector<uint8_t> inl(cnt);
    int nin = 0;
    uint8_t ok = 0;
    const double t1 = now_ms();
    if (msfm_fundamental_ransac_batch(ctx, 1, o, p1.data() + 2 * (size_t)off[h], p2.data() + 2 * (size_t)off[h], &fo, F, inl.data(), &nin, &ok) != MSFM_OK)
      return 5;
    if (timed > 0) ransac_ms += now_ms() - t1;   // (the first call warms up)
    timed++;
    kept += ok && nin > 20;
  }
  msfm_ctx_destroy(ctx);
  std::printf("restate_ms %.3f n_hyp %d n_ransac %d ransac_timed %d ransac_ms %.3f kept %d n_init_total %d\n", restate_ms, H, n_ransac,
              std::max(0, timed - 1), ransac_ms, kept, off[H]);
  return 0;
}
