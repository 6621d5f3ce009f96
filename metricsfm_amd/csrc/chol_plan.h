// Elimination structure of the reduced system (chol.hip): a nested-dissection tree of the camera graph laid out level
// by level.  Level 0 holds the leaf domains, level 1 the deepest separators, ... ; the nodes of one level are mutually
// uncoupled (their panel chains share launches), each is 64-aligned (identity padding inside) and couples only to its own
// descendants and to later columns.  Columns from the last level's b0 on (root separator + intrinsics) form the final
// dense chain.  n_levels = 0: plain dense order.  A node's descendants in a lower level are the nodes whose leaf interval
// lies inside its own (tree order inside every level makes them contiguous).
// corners: scratch for the deferred separator x separator updates, `nsplit` buffers of ldc x ldc doubles.
// Plain C++ without HIP: common.h and chol_schedule.h include it.
#pragma once

#define MSFM_CORNER_MAX_BLOCKS 128   // 64-column blocks behind the leaf level that k_corner_syrk's range table holds
struct msfm_chol_node { int begin, end, leaf_lo, leaf_hi; };
struct msfm_chol_level { int K = 0; msfm_chol_node node[8]; int begin = 0, b0 = 0; };
struct msfm_chol_plan {
  int n_levels = 0;
  msfm_chol_level level[3];
  double* corners = nullptr;
  int ldc = 0;
};
