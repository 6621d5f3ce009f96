// Builds the launch schedule (metricsfm_amd/csrc/chol_schedule.h) of hand-written elimination plans on the CPU and checks every
// part of it against brute force written here: what a node's panels reach, the row tiles of both factorisation forms, the task
// table of the persistent form, the corner ranges, the back-substitution launches, the residency rule and the refusals.
// Stand-alone (tests/test_chol_schedule_host.py builds it with the address and undefined-behaviour sanitizers); needs no GPU.
#include "chol_schedule.h"

#include <cstdlib>
#include <map>
#include <set>
#include <tuple>

static const char* g_case = "";
#define CHECK(cond)                                                                             \
  do {                                                                                          \
    if (!(cond)) {                                                                              \
      fprintf(stderr, "%s:%d: [%s] CHECK(%s) failed\n", __FILE__, __LINE__, g_case, #cond);      \
      exit(1);                                                                                  \
    }                                                                                           \
  } while (0)

static int ceil_div(long a, long b) { return (int)((a + b - 1) / b); }
static double g_corners_dummy[1];

struct Case {
  std::string name;
  int n = 0, npad = 0;
  bool tree = false;
  msfm_chol_plan plan;
};

static Case dense_case(int n) {
  Case c;
  c.name = "dense n=" + std::to_string(n);
  c.n = n; c.npad = 64 * ceil_div(n + 1, 64);
  return c;
}
// A complete binary tree: widths[lv][k] = 64-column blocks of node k of level lv (level 0: the leaves), then root_cols columns
// of root separator and intrinsics.  Node k of level lv covers the leaves [k 2^lv, (k + 1) 2^lv - 1].
static Case tree_case(const std::string& name, const std::vector<std::vector<int>>& widths, int root_cols) {
  Case c;
  c.name = name; c.tree = true;
  int col = 0;
  c.plan.n_levels = (int)widths.size();
  for (int lv = 0; lv < (int)widths.size(); lv++) {
    msfm_chol_level& L = c.plan.level[lv];
    L.K = (int)widths[lv].size();
    L.begin = col;
    for (int k = 0; k < L.K; k++) {
      L.node[k] = msfm_chol_node{col, col + 64 * widths[lv][k], k << lv, ((k + 1) << lv) - 1};
      col += 64 * widths[lv][k];
    }
    L.b0 = col;
  }
  c.n = col + root_cols;
  c.npad = 64 * ceil_div(c.n + 1, 64);
  c.plan.corners = g_corners_dummy;
  c.plan.ldc = 64 * ceil_div(c.n + 1 - c.plan.level[0].b0, 64);
  return c;
}

// ---- brute force ----
struct Range { int r0, r1; };   // rows [r0, r1)
static bool contains(const msfm_chol_node& a, const msfm_chol_node& d) { return a.leaf_lo <= d.leaf_lo && d.leaf_hi <= a.leaf_hi; }
// the rows below node (lv, k) that its panels reach: its ancestors level by level, then the root with the rhs row
static std::vector<Range> reach_of(const Case& c, int lv, int k) {
  std::vector<Range> out;
  const msfm_chol_node& nd = c.plan.level[lv].node[k];
  for (int h = lv + 1; h < c.plan.n_levels; h++) {
    int found = 0;
    for (int q = 0; q < c.plan.level[h].K; q++)
      if (contains(c.plan.level[h].node[q], nd)) { out.push_back(Range{c.plan.level[h].node[q].begin, c.plan.level[h].node[q].end}); found++; }
    CHECK(found <= 1);
  }
  out.push_back(Range{c.plan.level[c.plan.n_levels - 1].b0, c.n + 1});
  return out;
}
// first rows of the 16-row tiles that carry data, from range A = [a0, a1) on
static std::vector<int> tiles_of(Range A, const std::vector<Range>& B) {
  std::vector<int> rows;
  for (int r = A.r0; r < A.r1; r += 16) rows.push_back(r);
  for (const Range& b : B)
    for (int r = b.r0; r < b.r1; r += 16) rows.push_back(r);
  return rows;
}
struct Chain { int lv, k; Range A; std::vector<Range> B; int P, nA, nB; std::vector<int> rows; };
// the chains of group g (a level's nodes of non-zero width in order, or the root chain)
static std::vector<Chain> chains_of(const Case& c, int g) {
  std::vector<Chain> out;
  const int n_levels = c.tree ? c.plan.n_levels : 0;
  if (g < n_levels) {
    for (int k = 0; k < c.plan.level[g].K; k++) {
      const msfm_chol_node& nd = c.plan.level[g].node[k];
      if (nd.end == nd.begin) continue;
      Chain ch;
      ch.lv = g; ch.k = k; ch.A = Range{nd.begin, nd.end}; ch.B = reach_of(c, g, k);
      ch.P = ch.nA = (nd.end - nd.begin) / 64;
      int brows = 0;
      for (const Range& b : ch.B) brows += 16 * ceil_div(b.r1 - b.r0, 16);
      ch.nB = ceil_div(brows, 64);
      ch.rows = tiles_of(ch.A, ch.B);
      out.push_back(ch);
    }
  } else {
    const int begin = n_levels ? c.plan.level[n_levels - 1].b0 : 0;
    if (begin < c.n) {
      Chain ch;
      ch.lv = g; ch.k = 0; ch.A = Range{begin, c.n + 1};
      ch.P = ceil_div(c.n - begin, 64); ch.nA = ceil_div(c.n + 1 - begin, 64); ch.nB = 0;
      ch.rows = tiles_of(ch.A, {});
      out.push_back(ch);
    }
  }
  return out;
}
static int owners(int nrt) { return std::max(1, ceil_div(nrt - 4, 3)); }
// the trailing tiles of step l of a chain: (I, J), 1 <= J < nA - l, J <= I < nA - l + nB
static std::vector<std::pair<int, int>> step_tiles(const Chain& ch, int l) {
  std::vector<std::pair<int, int>> t;
  if (l < 1 || l >= ch.P) return t;
  for (int J = 1; J < ch.nA - l; J++)
    for (int I = J; I < ch.nA - l + ch.nB; I++) t.push_back({I, J});
  return t;
}

static void check_factor_forms(const Case& c, const CholSchedule& S, int capacity, int share) {
  const int n_levels = c.tree ? c.plan.n_levels : 0;
  const int row_end = 16 * ceil_div(c.n + 1, 16);
  CHECK(S.n_levels == n_levels && (int)S.group.size() == n_levels + 1 && S.nblk == ceil_div(c.n, 64));
  size_t task_cursor = 0;
  for (int g = 0; g <= n_levels; g++) {
    const ChainGroup& G = S.group[g];
    const std::vector<Chain> chains = chains_of(c, g);
    const ChainJobs& J = G.chain.jobs;
    CHECK(J.count == (int)chains.size());
    int wg = 0, maxp = 0;
    for (int k = 0; k < J.count; k++) {
      const ChainJob& jb = J.job[k];
      const Chain& ch = chains[k];
      // 1. segments: the ancestors in level order, then the root with the rhs row
      CHECK(jb.begin == ch.A.r0 && jb.P == ch.P && jb.na16 == 4 * ch.nA);
      CHECK(jb.nseg == (int)ch.B.size() && jb.nseg <= 4);
      for (int s = 0; s < jb.nseg; s++) {
        CHECK(jb.sb0[s] == ch.B[s].r0 && jb.sn16[s] == ceil_div(ch.B[s].r1 - ch.B[s].r0, 16));
        if (s + 1 < jb.nseg) CHECK(jb.sn16[s] % 4 == 0);
      }
      CHECK(jb.nrt == (int)ch.rows.size());
      // 2. row tiles: strictly increasing, inside [begin, 16 ceil((n + 1) / 16)), and where brute force puts them
      for (int at = 0; at < jb.nrt; at++) {
        const int r = row16(jb, at);
        CHECK(r == ch.rows[at] && r >= jb.begin && r + 16 <= row_end);
        if (at) CHECK(r > row16(jb, at - 1));
      }
      // 4. the row owners cover the tiles behind the diagonal block; workgroup ranges are contiguous
      CHECK(jb.ncw == owners(jb.nrt) && 4 + 3 * jb.ncw >= jb.nrt);
      CHECK(jb.wg0 == wg && jb.flag0 == k * (c.npad / 16) && jb.nrt <= c.npad / 16);
      wg += jb.ncw;
      maxp = std::max(maxp, ch.P);
    }
    CHECK(J.n_row_wg == wg && J.n_steps == std::max(0, maxp - 1) && G.chain.steps == maxp);
    // 3. the launch form names the same rows: tile rt of step l is tile 4 l + rt of the chain job
    CHECK((int)G.panels.size() == maxp);
    for (int l = 0; l < maxp; l++) {
      const PanelLaunch& PL = G.panels[l];
      int grid = 0, count = 0;
      bool full = true;
      for (int k = 0; k < J.count; k++) {
        if (l >= chains[k].P) continue;
        CHECK(count < PL.jobs.count);
        const PanelJob& pj = PL.jobs.job[count++];
        const ChainJob& cj = J.job[k];
        CHECK(pj.begin == cj.begin + 64 * l && pj.j0 == (l ? cj.begin + 64 * (l - 1) : -1));
        CHECK(pj.nrt == cj.nrt - 4 * l && pj.na16 == cj.na16 - 4 * l && pj.na16 % 4 == 0);
        for (int rt = 0; rt < pj.nrt; rt++) CHECK(row16(pj, rt) == row16(cj, 4 * l + rt) && row16(pj, rt) == chains[k].rows[4 * l + rt]);
        CHECK(pj.ncw == owners(pj.nrt) && 4 + 3 * pj.ncw >= pj.nrt);
        CHECK(pj.ntile == (int)step_tiles(chains[k], l).size());
        CHECK(pj.wg0 == grid && pj.nwg == pj.ncw + pj.ntile);
        grid += pj.nwg;
        if (g == n_levels) full = c.n - pj.begin >= 64;
        // the far corner of the job's last tile lies inside the matrix
        if (pj.ntile) CHECK(row16(pj, 4 * (pj.na16 / 4 + chains[k].nB - 1)) + 64 <= c.npad);
      }
      CHECK(count == PL.jobs.count && count > 0 && PL.grid == grid && PL.full == full);
    }
    // 5. the task table holds every trailing tile exactly once; 6. sorted by the priority key, a linear extension of the
    // dependencies, `urgent` exactly on the column behind the diagonal
    CHECK(G.chain.task_off == (int)task_cursor);
    std::map<std::tuple<int, int, int, int>, int> pos;   // (job, l, ti, tj) -> place in the launch's list
    int last_key = -1;
    for (int t = 0; t < G.chain.n_tasks; t++) {
      CHECK(task_cursor + t < S.tasks.size());
      const ChainTask& q = S.tasks[task_cursor + t];
      CHECK(q.k >= 0 && q.k < J.count && q.l >= 1 && q.l < chains[q.k].P && q.ti % 4 == 0 && q.tj % 4 == 0);
      const int I = q.ti / 4 - q.l, Jc = q.tj / 4 - q.l;
      CHECK(Jc >= 1 && Jc < chains[q.k].nA - q.l && I >= Jc && I < chains[q.k].nA - q.l + chains[q.k].nB);
      CHECK(pos.emplace(std::make_tuple((int)q.k, (int)q.l, (int)q.ti, (int)q.tj), t).second);
      const int key = 10 * q.l + 6 * (Jc - 1);
      CHECK(key >= last_key);
      last_key = key;
      CHECK(q.urgent == (Jc == 1 ? 1 : 0));
      if (q.l >= 2) {
        auto before = pos.find(std::make_tuple((int)q.k, q.l - 1, (int)q.ti, (int)q.tj));
        CHECK(before != pos.end() && before->second < t);
      }
    }
    int total = 0, max_step_tasks = 0;
    for (int l = 1; l < maxp; l++) {
      int step = 0;
      for (const Chain& ch : chains) step += (int)step_tiles(ch, l).size();
      total += step;
      max_step_tasks = std::max(max_step_tasks, step);
    }
    CHECK(G.chain.n_tasks == total);   // (all distinct and all of them real tiles: exactly once each)
    task_cursor += G.chain.n_tasks;
    // 9. bulk count and `usable`
    const int room = capacity - wg;
    CHECK(J.n_bulk_wg == std::max(1, std::min(room, max_step_tasks)));
    const bool fits = share == 1 ? wg <= capacity / 2 - 2 : (long)wg * share <= 3L * capacity / 4;
    const bool usable = !chains.empty() && fits && (max_step_tasks == 0 || 3 * room >= max_step_tasks) && maxp < 4000;
    CHECK(G.chain.usable == usable);
    // 7. corner ranges
    if (g < n_levels) {
      CHECK(G.has_corner == !chains.empty() && G.corner.sb == c.plan.level[g].b0);
      if (!G.has_corner) continue;
      const CornerPlan& C = G.corner;
      CHECK(C.nB64 == ceil_div(c.n + 1 - C.sb, 64) && C.nB64 <= MSFM_CORNER_MAX_BLOCKS && C.ntile == C.nB64 * (C.nB64 + 1) / 2);
      std::vector<std::set<int>> panels(C.nB64);
      for (int I = 0; I < C.nB64; I++) {
        const int row = C.sb + 64 * I;
        const msfm_chol_node* above = nullptr;   // the node of block I; nullptr: the root, above everything
        for (int h = g + 1; h < n_levels; h++)
          for (int q = 0; q < c.plan.level[h].K; q++)
            if (row >= c.plan.level[h].node[q].begin && row < c.plan.level[h].node[q].end) above = &c.plan.level[h].node[q];
        for (int q = 0; q < c.plan.level[g].K; q++) {
          const msfm_chol_node& nd = c.plan.level[g].node[q];
          if (above && !contains(*above, nd)) continue;
          for (int p = nd.begin / 64; p < nd.end / 64; p++) panels[I].insert(p);
        }
        for (int p = 0; p < c.npad / 64; p++) CHECK((p >= C.R.plo[I] && p < C.R.phi[I]) == (panels[I].count(p) == 1));
      }
      long wgs = 0;
      int smax = 1;
      for (int I = 0; I < C.nB64; I++)
        for (int Jc = 0; Jc <= I; Jc++) {
          int both = 0;
          for (int p : panels[I]) both += (int)panels[Jc].count(p);
          const int sp = std::min(MSFM_CORNER_SPLIT_MAX, std::max(1, ceil_div(both, C.target)));
          CHECK(sp == corner_splits(std::min((int)C.R.phi[I], (int)C.R.phi[Jc]) - std::max((int)C.R.plo[I], (int)C.R.plo[Jc]), C.target));
          wgs += sp;
          smax = std::max(smax, sp);
        }
      CHECK(C.smax == smax && C.target >= 1 && (wgs <= 560 || C.target == 64));
    }
  }
  CHECK(task_cursor == S.tasks.size());
}

// 8. the launch form of the back substitution
static void check_back(const Case& c, const CholSchedule& S) {
  const int n_levels = c.tree ? c.plan.n_levels : 0, nblk = ceil_div(c.n, 64);
  const int root_blk = n_levels ? c.plan.level[n_levels - 1].b0 / 64 : 0;
  CHECK(S.trinv_grid == nblk + ceil_div(c.npad, 256));
  CHECK(S.tree.n_levels == n_levels && S.tree.root_blk == root_blk);
  for (int lv = 0; lv < n_levels; lv++) {
    CHECK(S.tree.level[lv].K == c.plan.level[lv].K);
    for (int k = 0; k < c.plan.level[lv].K; k++) {
      const msfm_chol_node& nd = c.plan.level[lv].node[k];
      CHECK(S.tree.level[lv].node[k].b0 == nd.begin / 64 && S.tree.level[lv].node[k].b1 == nd.end / 64);
      CHECK(S.tree.level[lv].node[k].leaf_lo == nd.leaf_lo && S.tree.level[lv].node[k].leaf_hi == nd.leaf_hi);
    }
  }
  // what block j couples to among the earlier blocks: the earlier blocks of its own node and all blocks of its descendants;
  // a block of the root: everything before it
  auto earlier = [&](int j) {
    std::set<int> e;
    if (j >= root_blk) { for (int i = 0; i < j; i++) e.insert(i); return e; }
    for (int lv = 0; lv < n_levels; lv++)
      for (int k = 0; k < c.plan.level[lv].K; k++) {
        const msfm_chol_node& nd = c.plan.level[lv].node[k];
        if (j < nd.begin / 64 || j >= nd.end / 64) continue;
        for (int i = nd.begin / 64; i < j; i++) e.insert(i);
        for (int lo = 0; lo < lv; lo++)
          for (int q = 0; q < c.plan.level[lo].K; q++)
            if (contains(nd, c.plan.level[lo].node[q]))
              for (int i = c.plan.level[lo].node[q].begin / 64; i < c.plan.level[lo].node[q].end / 64; i++) e.insert(i);
      }
    return e;
  };
  std::vector<int> solved(nblk, 0);
  for (const BackLaunch& B : S.back) {
    CHECK(B.jobs.count >= 1 && B.jobs.count <= 16);
    std::map<int, std::set<int>> ranges;   // block jb -> the blocks its jobs update
    int wg = 0;
    for (int q = 0; q < B.jobs.count; q++) {
      const BackJob& j = B.jobs.job[q];
      CHECK(j.wg0 == wg && j.ni >= 0 && j.jb >= (B.pair ? 1 : 0) && j.jb < nblk);
      wg += std::max(1, j.ni);
      std::set<int>& r = ranges[j.jb];
      for (int i = j.ib; i < j.ib + j.ni; i++) CHECK(r.insert(i).second);
    }
    CHECK(B.grid == wg);
    for (auto& kv : ranges) {
      const int jb = kv.first, low = B.pair ? jb - 1 : jb;   // the launch solves blocks [low, jb]
      std::set<int> want = earlier(low);
      if (B.pair) {
        // the pair shares its ranges: both blocks couple to the same earlier blocks, and to each other
        std::set<int> w2 = earlier(jb);
        CHECK(w2.count(low) == 1);
        w2.erase(low);
        CHECK(w2 == want);
      }
      CHECK(kv.second == want);
      for (int i : want) CHECK(!solved[i]);   // nothing it updates has been solved yet
      for (int b = low; b <= jb; b++) { CHECK(!solved[b]); solved[b] = 1; }
    }
  }
  for (int b = 0; b < nblk; b++) CHECK(solved[b] == 1);
}

static void check_case(const Case& c) {
  static std::string label;
  const int caps[3][2] = {{512, 1}, {16, 1}, {512, 2}};
  unsigned long long sigs[3];
  for (int v = 0; v < 3; v++) {
    label = c.name + " capacity " + std::to_string(caps[v][0]) + " share " + std::to_string(caps[v][1]);
    g_case = label.c_str();
    CholSchedule S;
    std::string err;
    const int rc = chol_schedule_build(c.n, c.npad, c.tree ? &c.plan : nullptr, caps[v][0], caps[v][1], false, S, &err);
    CHECK(rc == MSFM_OK && err.empty());
    sigs[v] = S.sig;
    CHECK(S.sig != 0 && S.sig == chol_schedule_sig(c.n, c.npad, c.tree ? &c.plan : nullptr, caps[v][0], caps[v][1], false));
    check_factor_forms(c, S, caps[v][0], caps[v][1]);
    check_back(c, S);
    // MSFM_CHAIN_FORCE lifts the tile-count part of the rule and nothing else
    CholSchedule F;
    CHECK(chol_schedule_build(c.n, c.npad, c.tree ? &c.plan : nullptr, caps[v][0], caps[v][1], true, F, &err) == MSFM_OK);
    CHECK(F.sig != S.sig && F.group.size() == S.group.size());
    for (size_t g = 0; g < S.group.size(); g++) {
      const int wg = S.group[g].chain.jobs.n_row_wg;
      const bool fits = caps[v][1] == 1 ? wg <= caps[v][0] / 2 - 2 : (long)wg * caps[v][1] <= 3L * caps[v][0] / 4;
      CHECK(F.group[g].chain.usable == (S.group[g].chain.jobs.count > 0 && fits));
      CHECK(!S.group[g].chain.usable || F.group[g].chain.usable);
    }
  }
  CHECK(sigs[0] != sigs[1] && sigs[0] != sigs[2] && sigs[1] != sigs[2]);
}

// 10. a plan that cannot run is refused with MSFM_E_INVAL and nothing is built
static void check_refusal(const char* name, Case c, const char* text) {
  g_case = name;
  CholSchedule S;
  std::string err;
  CHECK(chol_schedule_build(c.n, c.npad, &c.plan, 512, 1, false, S, &err) == MSFM_E_INVAL);
  CHECK(err.find(text) != std::string::npos && S.sig == 0 && S.group.empty() && S.tasks.empty() && S.back.empty());
}

int main() {
  std::vector<Case> cases;
  for (int n : {1, 63, 64, 65, 141, 1011}) cases.push_back(dense_case(n));
  cases.push_back(tree_case("K=2, ragged last block", {{2, 3}}, 70));
  cases.push_back(tree_case("4 | 2 | root", {{3, 1, 2, 4}, {1, 2}}, 64 + 17));
  cases.push_back(tree_case("8 | 4 | 2 | root", {{2, 1, 3, 1, 2, 2, 1, 4}, {1, 1, 2, 1}, {1, 2}}, 131));
  cases.push_back(tree_case("8 | 4 | 2 | root, long chains", {{9, 7, 8, 10, 9, 8, 7, 9}, {2, 3, 2, 2}, {3, 2}}, 200));
  cases.push_back(tree_case("4 | 2 | root, a leaf of zero width", {{3, 0, 2, 4}, {1, 2}}, 99));
  cases.push_back(tree_case("4 | 2 | root, a separator of zero width", {{2, 2, 1, 3}, {0, 1}}, 40));
  cases.push_back(tree_case("K=2, a level of zero width", {{0, 0}}, 150));
  cases.push_back(tree_case("4 | 2 | root, the root holds only the intrinsics", {{1, 2, 2, 1}, {1, 1}}, 3));
  cases.push_back(tree_case("K=2, the rhs row opens a block of its own", {{2, 2}}, 64));
  for (const Case& c : cases) check_case(c);

  const Case good = tree_case("refusals", {{2, 2}}, 70);
  { Case c = good; c.plan.level[0].K = 9; check_refusal("K = 9", c, "bad plan level"); }
  { Case c = good; c.plan.level[0].b0 += 16; check_refusal("unaligned b0", c, "bad plan level"); }
  { Case c = good; c.plan.ldc -= 64; check_refusal("ldc too small", c, "bad plan level"); }
  { Case c = good; c.plan.corners = nullptr; check_refusal("no corner scratch", c, "cholesky: bad plan"); }
  { Case c = good; c.plan.n_levels = 4; check_refusal("four levels", c, "cholesky: bad plan"); }
  check_refusal("more than MSFM_CORNER_MAX_BLOCKS separator blocks", tree_case("", {{1, 1}}, 64 * MSFM_CORNER_MAX_BLOCKS + 1), "separator part too large");
  {
    // three levels of eight nodes, node k above node k: a back-substitution launch of the top level would hold 24 ranges
    Case c = tree_case("", {{2, 2, 2, 2, 2, 2, 2, 2}, {2, 2, 2, 2, 2, 2, 2, 2}, {2, 2, 2, 2, 2, 2, 2, 2}}, 70);
    for (int lv = 0; lv < 3; lv++)
      for (int k = 0; k < 8; k++) c.plan.level[lv].node[k].leaf_lo = c.plan.level[lv].node[k].leaf_hi = k;
    check_refusal("too many back-substitution ranges", c, "too many back-substitution ranges");
  }
  { Case c = good; c.npad = 128; check_refusal("chain job larger than the flag table", c, "larger than the flag table"); }
  printf("chol_schedule_host_check ok: %zu plans x 3 devices, 8 refusals\n", cases.size());
  return 0;
}
