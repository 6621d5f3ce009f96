// The launch schedule of an elimination plan: everything msfm_chol_factor_solve (chol.hip) launches for the plan - both
// factorisation forms of every tree level and of the root, the corner updates, both back-substitution forms - as the
// kernel-argument structs themselves, built once per plan by chol_schedule_build() and kept in the solver's workspace.  The
// driver only reads it, the kernels only decode it.  Plain C++ without HIP: tests/chol_schedule_host_check.cc builds schedules
// on the CPU and checks them against brute force.
// Both factorisation forms are made from chains of panels (ChainRows: the 64-column steps of a tree node or of the root, and the
// rows they reach), derived in one place (chol_sched::node_rows / root_rows): k_chain's ChainJob is the whole chain,
// k_panel_v2's PanelJob of step l the chain from its row tile 4 l on.
#pragma once
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/msfm.h"
#include "chol_plan.h"

#ifdef __HIPCC__
#define MSFM_SCHED_HD __host__ __device__ __forceinline__
#else
#define MSFM_SCHED_HD inline
#endif

// ---- the rows of a job, as both factorisation kernels decode them ----
// Row tiles (16 rows each) counted from `begin`: range A = na16 tiles from row `begin` on (the rest of the job's own node,
// starting with the 64 x 64 block to factor; na16 a multiple of 4), then range B in up to four segments (the node's
// ancestors, one per level, then the root with the rhs row): segment g starts at row sb0[g] and holds sn16[g] tiles, every
// segment but the last a multiple of four.  The root chain has no range B: A runs down to the rhs row.
struct RowRanges { int begin, na16, nseg, sb0[4], sn16[4]; };
MSFM_SCHED_HD int row16(const RowRanges& R, int at) {   // first row of row tile `at`
  if (at < R.na16) return R.begin + 16 * at;
  int r = at - R.na16, g = 0;
  while (g + 1 < R.nseg && r >= R.sn16[g]) { r -= R.sn16[g]; g++; }
  return R.sb0[g] + 16 * r;
}

// ---- k_panel_v2: one launch per 64-column step ----
// A launch carries the step of every chain of a tree level side by side, one job each.  A job factors the block at `begin`
// behind the panel at j0 and applies that panel to its rows; the B x B tiles, which every job of the level would write, are
// left out and formed afterwards by one SYRK over all panels (k_corner_syrk, then k_merge_corners).
struct PanelJob : RowRanges {
  int j0;          // panel to apply, < 0: none (first block of a chain)
  int nrt;         // 16-row tiles that carry data, over A then B
  int ncw;         // column-0 workgroups
  int wg0, nwg;    // workgroups [wg0, wg0 + nwg) of the launch: ncw column-0 ones, then the bulk ones
  int ntile;       // 64x64 tiles of the trailing update, one per bulk workgroup
};
struct PanelJobs { int count; PanelJob job[8]; };

// ---- k_chain: the chains of a tree level (or the root chain) as one persistent launch ----
struct ChainJob : RowRanges {   // begin: first column of the node
  int P;                // factor steps = 64-column blocks of the node
  int nrt;              // 16-row tiles that carry data, A then B, counted from the node's first row
  int ncw, wg0;         // row-owner workgroups [wg0, wg0 + ncw)
  int flag0;            // first entry of the job in rowflag
};
struct ChainJobs { int count, n_row_wg, n_bulk_wg, n_steps; ChainJob job[8]; };   // n_steps: the longest chain's steps - 1
// A bulk task: apply the panel of step l - 1 of job k to the 64 x 64 tile at row tiles (ti, tj) of the job; urgent: the next
// step's row owners wait for it (the column right behind the diagonal block)
struct ChainTask { short k, l, ti, tj, urgent; };

// ---- k_corner_syrk / k_merge_corners: the deferred B x B update of a tree level ----
#define MSFM_CORNER_SPLIT_MAX 8
struct CornerRanges { short plo[MSFM_CORNER_MAX_BLOCKS], phi[MSFM_CORNER_MAX_BLOCKS]; };
MSFM_SCHED_HD int corner_splits(int panels, int target) {
  const int s = (panels + target - 1) / target;
  return s < 1 ? 1 : (s > MSFM_CORNER_SPLIT_MAX ? MSFM_CORNER_SPLIT_MAX : s);
}
// Per 64-row block of the B square (rows from sb on) the panels of the level that lie under the block's node, and into how
// many pieces a tile's panels are cut: ceil(panels / target), at most MSFM_CORNER_SPLIT_MAX; smax = the largest count.
struct CornerPlan {
  CornerRanges R = {};
  int sb = 0, nB64 = 0, ntile = 0;   // first row of the square, its 64-row blocks, its lower 64 x 64 tiles
  int target = 1, smax = 1;
};

// ---- back substitution ----
struct BackJob { int jb, ib, ni, wg0; };
struct BackJobs { int count; BackJob job[16]; };
struct BackTree {
  int n_levels;
  int root_blk;                       // first block of the root chain
  struct { int K; struct { int b0, b1, leaf_lo, leaf_hi; } node[8]; } level[3];   // block ranges of the nodes
};

// ---- the schedule ----
struct ChainLaunch {
  ChainJobs jobs;
  int task_off = 0, n_tasks = 0;   // the launch's tiles in CholSchedule::tasks, in ticket order
  int steps = 0;        // panel steps on its critical path (for the timers)
  bool usable = false;  // the device holds the launch's row owners and enough bulk workgroups at once
};
struct PanelLaunch { PanelJobs jobs; int grid; bool full; };   // k_panel_v2<full>
struct BackLaunch { BackJobs jobs; int grid; bool pair; };     // k_backsolve_pair or k_backsolve_step
// The panel chains of a tree level side by side, or the root chain
struct ChainGroup {
  ChainLaunch chain;                 // the persistent form: one k_chain launch
  std::vector<PanelLaunch> panels;   // the launch form: one k_panel_v2 launch per step
  bool has_corner = false;           // (levels) the level has panels, so a corner update follows
  CornerPlan corner;
};
struct CholSchedule {
  unsigned long long sig = 0;        // chol_schedule_sig of what it was built for; 0: none
  int n_levels = 0, nblk = 0;        // tree levels; 64-column blocks of the system
  std::vector<ChainGroup> group;     // [n_levels + 1]: the levels in order, then the root
  std::vector<ChainTask> tasks;      // the bulk tiles of all k_chain launches
  BackTree tree;                     // k_backsolve_chain
  int trinv_grid = 0;                // k_trinv64_full: a workgroup per block, then 256 entries of w each
  std::vector<BackLaunch> back;      // the launch form: the root from its last block up, then level by level
};

namespace chol_sched {
inline int cdiv(long a, long b) { return (int)((a + b - 1) / b); }

// A chain of panels and the rows it reaches: P factor steps from column `begin` on, nb16 tiles in range B, nrt tiles with data
struct ChainRows : RowRanges { int P, nb16, nrt; };
inline int row_owners(int nrt) { return std::max(1, cdiv(nrt - 4, 3)); }   // three 16-row tiles each, behind the diagonal block
inline int root_begin(const msfm_chol_plan* plan) { return plan && plan->n_levels > 0 ? plan->level[plan->n_levels - 1].b0 : 0; }
inline bool under(const msfm_chol_node& d, const msfm_chol_node& a) { return a.leaf_lo <= d.leaf_lo && a.leaf_hi >= d.leaf_hi; }

// Node k of level lv: its own blocks, then its ancestors (one node per higher level), then the root chain with the rhs row -
// everything else from the level's b0 on is structurally zero in its columns
inline ChainRows node_rows(const msfm_chol_plan& plan, int lv, int k, int nrows) {
  const msfm_chol_node& nd = plan.level[lv].node[k];
  ChainRows R = {};
  R.begin = nd.begin; R.P = (nd.end - nd.begin) / 64; R.na16 = 4 * R.P;
  for (int h = lv + 1; h < plan.n_levels; h++)
    for (int q = 0; q < plan.level[h].K; q++) {
      const msfm_chol_node& a = plan.level[h].node[q];
      if (under(nd, a)) { R.sb0[R.nseg] = a.begin; R.sn16[R.nseg] = (a.end - a.begin) / 16; R.nb16 += R.sn16[R.nseg]; R.nseg++; break; }
    }
  R.sb0[R.nseg] = root_begin(&plan); R.sn16[R.nseg] = cdiv(nrows - root_begin(&plan), 16); R.nb16 += R.sn16[R.nseg]; R.nseg++;
  R.nrt = 4 * R.P + R.nb16;
  return R;
}
// The root chain (or the whole system in dense order): range A runs down to the rhs row, there is no range B
inline ChainRows root_rows(const msfm_chol_plan* plan, int n) {
  ChainRows R = {};
  R.begin = root_begin(plan); R.P = cdiv(n - R.begin, 64); R.na16 = 4 * cdiv(n + 1 - R.begin, 64);
  R.nrt = cdiv(n + 1 - R.begin, 16);
  return R;
}
inline ChainJob chain_job(const ChainRows& R, int wg0, int flag0) {
  ChainJob jb = {};
  static_cast<RowRanges&>(jb) = R;
  jb.P = R.P; jb.nrt = R.nrt; jb.ncw = row_owners(R.nrt); jb.wg0 = wg0; jb.flag0 = flag0;
  return jb;
}
// Step l of the chain: factor block l behind its panel l - 1
inline PanelJob panel_job(const ChainRows& R, int l, int wg0) {
  PanelJob jb = {};
  static_cast<RowRanges&>(jb) = R;
  jb.begin += 64 * l; jb.na16 -= 4 * l;
  const int nA = jb.na16 / 4, nB = cdiv(R.nb16, 4);
  jb.j0 = l > 0 ? R.begin + 64 * (l - 1) : -1;
  jb.nrt = R.nrt - 4 * l; jb.ncw = row_owners(jb.nrt);
  // the trailing tiles (I, J), 1 <= J < nA, J <= I < nA + nB: the column-0 workgroups own J = 0, and the tiles among the rows
  // of range B are formed once, after the chains (k_corner_syrk)
  jb.ntile = l > 0 ? nA * (nA - 1) / 2 + nB * (nA - 1) : 0;
  jb.wg0 = wg0; jb.nwg = jb.ncw + jb.ntile;
  return jb;
}

// Block jb of a node of level lv couples, in the back substitution, to its descendants in level lo < lv: blocks [rb, rb + rn)
inline bool descendants(const msfm_chol_plan& plan, const msfm_chol_node& nd, int lo, int& rb, int& rn) {
  const msfm_chol_level& D = plan.level[lo];
  int d0 = -1, d1 = -1;
  for (int q = 0; q < D.K; q++)
    if (under(D.node[q], nd)) { if (d0 < 0) d0 = q; d1 = q; }
  if (d0 < 0) return false;
  rb = D.node[d0].begin / 64; rn = (D.node[d1].end - D.node[d0].begin) / 64;
  return rn > 0;
}

// The persistent form of a group: its jobs, its bulk tiles in ticket order (appended to `tasks`) and whether the device can
// hold it.  capacity = workgroups of k_chain resident at once; share = contexts that launch it on the device at the same time.
inline ChainLaunch chain_launch(const std::vector<ChainRows>& rows, int npad, int capacity, int share, bool force, std::vector<ChainTask>& tasks) {
  ChainLaunch L;
  ChainJobs& J = L.jobs;
  memset(&J, 0, sizeof J);
  int wg = 0, maxp = 0;
  for (const ChainRows& R : rows) {
    J.job[J.count] = chain_job(R, wg, J.count * (npad / 16));
    wg += J.job[J.count].ncw;
    maxp = std::max(maxp, R.P);
    J.count++;
  }
  J.n_row_wg = wg;
  J.n_steps = std::max(0, maxp - 1);
  L.steps = maxp;
  L.task_off = (int)tasks.size();
  // Every tile of every launch step in priority order (chain_bulk, chol.hip): tile (I, J) of step l - "apply the panel of step
  // l - 1" - has the key l + 0.6 (J - 1).  Stable: equal keys stay in (step, job, column-major) order.
  struct Keyed { int key; ChainTask t; };
  std::vector<Keyed> lt;
  int max_step_tasks = 0;
  for (int l = 1; l <= J.n_steps; l++) {
    int step_tasks = 0;
    for (int k = 0; k < J.count; k++) {
      if (l >= rows[k].P) continue;
      const int nA = rows[k].na16 / 4 - l, nB = cdiv(rows[k].nb16, 4);
      for (int Jc = 1; Jc < nA; Jc++)
        for (int I = Jc; I < nA + nB; I++) {
          lt.push_back(Keyed{10 * l + 6 * (Jc - 1), ChainTask{(short)k, (short)l, (short)(4 * (I + l)), (short)(4 * (Jc + l)), (short)(Jc == 1 ? 1 : 0)}});
          step_tasks++;
        }
    }
    max_step_tasks = std::max(max_step_tasks, step_tasks);
  }
  std::stable_sort(lt.begin(), lt.end(), [](const Keyed& a, const Keyed& b) { return a.key < b.key; });
  for (const Keyed& q : lt) tasks.push_back(q.t);
  L.n_tasks = (int)lt.size();
  // bulk workgroups: what the device holds beside the row owners, at most one per tile of the busiest step
  const int room = capacity - wg;
  J.n_bulk_wg = std::max(1, std::min(room, max_step_tasks));
  // usable: every row owner resident with room to spare, a bulk workgroup for every three tiles of the busiest step at least
  // (force, MSFM_CHAIN_FORCE: whatever the tile count).  Contexts that share the device and launch the kernel at the same time
  // (share > 1: ranks are synchronised by the reduction in front of the factorisation) must all have their row owners resident,
  // or none makes progress.  One context: just under half of the resident workgroups - two independent PROCESSES on one GPU
  // each see share == 1, and with exactly half each their row owners could fill the device and leave no bulk workgroup of
  // either resident; two short of half, one bulk workgroup always finds a slot, its launch drains (whoever holds the lowest open
  // ticket can finish) and the other follows.  (A quarter would send systems of more than ~170 blocks - config 5 in full - back
  // to the launch form for a case the bounded polls already turn into an error.)
  const bool fits = share <= 1 ? wg <= capacity / 2 - 2 : (long)wg * share <= 3L * capacity / 4;
  L.usable = J.count > 0 && fits && (max_step_tasks == 0 || 3 * room >= max_step_tasks || force) && maxp < 4000;   // (steps and tiles are shorts)
  return L;
}

// The launch form of a group: step l of every chain that still has a block, side by side
inline std::vector<PanelLaunch> panel_launches(const std::vector<ChainRows>& rows, int n) {
  std::vector<PanelLaunch> out;
  int maxp = 0;
  for (const ChainRows& R : rows) maxp = std::max(maxp, R.P);
  for (int l = 0; l < maxp; l++) {
    PanelLaunch PL = {};
    PL.full = true;
    for (const ChainRows& R : rows) {
      if (l >= R.P) continue;
      const PanelJob jb = panel_job(R, l, PL.grid);
      PL.grid += jb.nwg;
      PL.full = PL.full && (R.nseg > 0 || n - jb.begin >= 64);   // (only the system's last block can be partial: the end of the root chain)
      PL.jobs.job[PL.jobs.count++] = jb;
    }
    out.push_back(PL);
  }
  return out;
}

inline CornerPlan corner_plan(const msfm_chol_plan& plan, int lv, int nrows) {
  const msfm_chol_level& L = plan.level[lv];
  CornerPlan C;
  C.sb = L.b0;
  C.nB64 = cdiv(nrows - L.b0, 64);
  C.ntile = C.nB64 * (C.nB64 + 1) / 2;
  CornerRanges& R = C.R;
  for (int I = 0; I < C.nB64; I++) {
    const int row = C.sb + 64 * I;
    int lo = 0, hi = 0x7fffffff;   // leaf interval of the block's node; the root covers everything
    for (int h = lv + 1; h < plan.n_levels; h++)
      for (int q = 0; q < plan.level[h].K; q++)
        if (row >= plan.level[h].node[q].begin && row < plan.level[h].node[q].end) { lo = plan.level[h].node[q].leaf_lo; hi = plan.level[h].node[q].leaf_hi; }
    int plo = 0, phi = 0;
    bool any = false;
    for (int q = 0; q < L.K; q++)
      if (L.node[q].leaf_lo >= lo && L.node[q].leaf_hi <= hi) { if (!any) plo = L.node[q].begin / 64; phi = L.node[q].end / 64; any = true; }
    R.plo[I] = (short)plo; R.phi[I] = (short)phi;
  }
  // panels per piece: the smallest count with which the pieces cover the chip about once
  for (C.target = 1;; C.target++) {
    long wgs = 0;
    C.smax = 1;
    for (int I = 0; I < C.nB64; I++)
      for (int J = 0; J <= I; J++) {
        const int sp = corner_splits(std::min((int)R.phi[I], (int)R.phi[J]) - std::max((int)R.plo[I], (int)R.plo[J]), C.target);
        wgs += sp;
        C.smax = std::max(C.smax, sp);
      }
    if (wgs <= 560 || C.target >= 64) break;
  }
  return C;
}

inline BackTree back_tree(const msfm_chol_plan* plan) {
  BackTree bt;
  memset(&bt, 0, sizeof bt);
  bt.n_levels = plan ? plan->n_levels : 0;
  bt.root_blk = root_begin(plan) / 64;
  for (int lv = 0; lv < bt.n_levels; lv++) {
    bt.level[lv].K = plan->level[lv].K;
    for (int k = 0; k < plan->level[lv].K; k++) {
      const msfm_chol_node& nd = plan->level[lv].node[k];
      bt.level[lv].node[k].b0 = nd.begin / 64; bt.level[lv].node[k].b1 = nd.end / 64;
      bt.level[lv].node[k].leaf_lo = nd.leaf_lo; bt.level[lv].node[k].leaf_hi = nd.leaf_hi;
    }
  }
  return bt;
}

// The back substitution as launches: two adjacent blocks per launch (k_backsolve_pair), a chain's odd first block alone
// (k_backsolve_step); every job recomputes z of its blocks and takes it out of one range of earlier blocks.  False: a launch
// would need more than the sixteen jobs it can hold.
inline bool back_launches(const msfm_chol_plan* plan, int nblk, std::vector<BackLaunch>& out) {
  const int n_levels = plan ? plan->n_levels : 0, first_dense = root_begin(plan) / 64;
  auto launch = [](bool pair) { BackLaunch B; memset(&B.jobs, 0, sizeof B.jobs); B.grid = 0; B.pair = pair; return B; };
  bool ok = true;
  auto add = [&ok](BackLaunch& B, int jb, int ib, int ni) {
    if (B.jobs.count >= 16) { ok = false; return; }
    B.jobs.job[B.jobs.count++] = BackJob{jb, ib, ni, B.grid}; B.grid += std::max(1, ni);
  };
  // the root chain (or everything): a block couples to every block before it
  for (int jb = nblk - 1; jb >= first_dense;) {
    const bool pair = jb - 1 >= first_dense;
    BackLaunch B = launch(pair);
    add(B, jb, 0, pair ? jb - 1 : jb);
    out.push_back(B);
    jb -= pair ? 2 : 1;
  }
  for (int lv = n_levels - 1; lv >= 0; lv--) {
    // Blocks P_k - 1 - 2l and P_k - 2 - 2l of every node of the level in one launch (a node's last odd block alone).  A
    // block couples to the earlier blocks of its own node and to its descendants in the lower levels (contiguous in
    // every level: tree order) - one job per range; siblings never touch the same rows.
    const msfm_chol_level& L = plan->level[lv];
    int maxp = 0;
    for (int k = 0; k < L.K; k++) maxp = std::max(maxp, (L.node[k].end - L.node[k].begin) / 64);
    for (int l = 0; 2 * l < maxp; l++) {
      BackLaunch pj = launch(true), sj = launch(false);
      for (int k = 0; k < L.K; k++) {
        const int ib = L.node[k].begin / 64, P = (L.node[k].end - L.node[k].begin) / 64;
        if (2 * l >= P) continue;
        const int jb = ib + P - 1 - 2 * l;
        const bool pair = jb - 1 >= ib;
        BackLaunch& B = pair ? pj : sj;
        add(B, jb, ib, pair ? jb - 1 - ib : jb - ib);   // earlier blocks of the node itself
        int rb, rn;
        for (int lo = lv - 1; lo >= 0; lo--)
          if (descendants(*plan, L.node[k], lo, rb, rn)) add(B, jb, rb, rn);
      }
      if (pj.jobs.count) out.push_back(pj);
      if (sj.jobs.count) out.push_back(sj);
    }
  }
  return ok;
}

inline int refuse(std::string* err, const char* text, int v = 0) {
  char buf[160];
  snprintf(buf, sizeof buf, text, v);
  if (err) *err = buf;
  return MSFM_E_INVAL;
}
// Everything that makes a plan unusable, checked before anything is built or launched: a refusal must not leave half a
// factorisation behind
inline int validate(int n, int npad, const msfm_chol_plan* plan, std::string* err) {
  const int nrows = n + 1, n_levels = plan ? plan->n_levels : 0;
  if (n_levels <= 0) return MSFM_OK;
  if (n_levels > 3 || !plan->corners) return refuse(err, "cholesky: bad plan");
  for (int lv = 0; lv < n_levels; lv++) {
    const msfm_chol_level& L = plan->level[lv];
    if (L.K < 1 || L.K > 8 || L.b0 % 64 || L.begin % 64 || plan->ldc < 64 * cdiv(nrows - L.b0, 64)) return refuse(err, "cholesky: bad plan level");
    if (cdiv(nrows - L.b0, 64) > MSFM_CORNER_MAX_BLOCKS)
      return refuse(err, "cholesky: separator part too large for the corner update (%d blocks)", cdiv(nrows - L.b0, 64));
  }
  for (int lv = 0; lv < n_levels; lv++)
    for (int k = 0; k < plan->level[lv].K; k++)
      if (node_rows(*plan, lv, k, nrows).nrt > npad / 16) return refuse(err, "cholesky: chain job larger than the flag table");
  std::vector<BackLaunch> back;
  if (!back_launches(plan, 0, back)) return refuse(err, "cholesky: too many back-substitution ranges in one launch");
  return MSFM_OK;
}
}  // namespace chol_sched

// What a schedule depends on
inline unsigned long long chol_schedule_sig(int n, int npad, const msfm_chol_plan* plan, int capacity, int share, bool force) {
  unsigned long long sig = 1469598103934665603ull;
  auto mix = [&](long v) { sig = (sig ^ (unsigned long long)v) * 1099511628211ull; };
  const int n_levels = plan ? plan->n_levels : 0;
  mix(n); mix(npad); mix(capacity); mix(std::max(1, share)); mix(force); mix(n_levels);
  for (int lv = 0; lv < n_levels && lv < 3; lv++) {
    const msfm_chol_level& L = plan->level[lv];
    mix(L.K); mix(L.b0); mix(L.begin);
    for (int k = 0; k < L.K && k < 8; k++) { mix(L.node[k].begin); mix(L.node[k].end); mix(L.node[k].leaf_lo); mix(L.node[k].leaf_hi); }
  }
  if (plan) mix(plan->ldc);
  return sig ? sig : 1;
}

// The schedule of `plan` (nullptr or no levels: dense order) for a system of n columns in an npad x npad matrix.
// capacity: workgroups of k_chain the device keeps resident (0: the persistent form is never usable); share: contexts that
// use the device at the same time; force: MSFM_CHAIN_FORCE.  MSFM_E_INVAL with a text in *err, and S untouched, for a plan
// that cannot run.
inline int chol_schedule_build(int n, int npad, const msfm_chol_plan* plan, int capacity, int share, bool force, CholSchedule& S, std::string* err) {
  namespace cs = chol_sched;
  const int rc = cs::validate(n, npad, plan, err);
  if (rc != MSFM_OK) return rc;
  const int nrows = n + 1;
  CholSchedule N;
  N.n_levels = plan ? std::max(0, plan->n_levels) : 0;
  N.nblk = cs::cdiv(n, 64);
  for (int lv = 0; lv <= N.n_levels; lv++) {
    ChainGroup G;
    std::vector<cs::ChainRows> rows;
    if (lv < N.n_levels) {
      for (int k = 0; k < plan->level[lv].K; k++) {
        const cs::ChainRows R = cs::node_rows(*plan, lv, k, nrows);
        if (R.P > 0) rows.push_back(R);
      }
      G.has_corner = !rows.empty();
      if (G.has_corner) G.corner = cs::corner_plan(*plan, lv, nrows);
      else G.corner.sb = plan->level[lv].b0;
    } else if (cs::root_begin(plan) < n) {
      rows.push_back(cs::root_rows(plan, n));
    }
    G.chain = cs::chain_launch(rows, npad, capacity, share, force, N.tasks);
    G.panels = cs::panel_launches(rows, n);
    N.group.push_back(G);
  }
  N.tree = cs::back_tree(plan);
  N.trinv_grid = N.nblk + cs::cdiv(npad, 256);
  cs::back_launches(plan, N.nblk, N.back);
  N.sig = chol_schedule_sig(n, npad, plan, capacity, share, force);
  S = std::move(N);
  return MSFM_OK;
}
