// Host walk of the point-workgroup geometry (PtMap, metricsfm_amd/csrc/ba_device.h): for random class counts, zeros and exact
// multiples of the workgroup sizes included, every point lies in exactly the workgroup ptmap_wg_of names, the workgroups
// tile the points in order with no gap, none mixes classes, each has the lane width of its class and at most 256 lanes, and
// ptmap_n_wg is the number of workgroups that hold points.  A stand-alone program: it is compiled for the host only and
// never loaded into another process, so it can also be built with -fsanitize=address,undefined.
#include <cstdio>
#include <cstdlib>
#include <random>

#include "ba_device.h"

static int fails = 0;
#define CHECK(c, ...) do { if (!(c)) { if (fails++ < 20) { std::printf("FAIL %s:%d %s | ", __FILE__, __LINE__, #c); std::printf(__VA_ARGS__); std::printf("\n"); } } } while (0)

static const int kLanes[PTMAP_CLASSES] = {4, 8, 16, 0}, kPoints[PTMAP_CLASSES] = {64, 32, 16, 32};

static void check_counts(const int (&n)[PTMAP_CLASSES]) {
  const PtMap m = ptmap_make(n, true);
  const int npb = n[0] + n[1] + n[2] + n[3];
  int first_of[PTMAP_CLASSES + 1] = {0};
  for (int c = 0; c < PTMAP_CLASSES; c++) first_of[c + 1] = first_of[c] + n[c];
  auto class_of_point = [&](int pb) { int c = 0; while (pb >= first_of[c + 1]) c++; return c; };
  const int n_wg = ptmap_n_wg(m);
  // the workgroups in order: consecutive, non-empty (but for the single workgroup of an empty problem), one class each
  int next = 0, visited = 0;
  for (int w = 0; w < n_wg; w++) {
    const int f = ptmap_wg_first(m, w), e = ptmap_wg_end(m, w);
    if (npb == 0) { CHECK(n_wg == 1 && f == 0 && e == 0, "empty problem: n_wg %d first %d end %d", n_wg, f, e); continue; }
    CHECK(f == next, "w %d first %d, expected %d", w, f, next);
    CHECK(e > f, "w %d is empty: [%d, %d)", w, f, e);
    if (e <= f) break;
    const int c = class_of_point(f);
    CHECK(class_of_point(e - 1) == c, "w %d mixes classes %d and %d", w, c, class_of_point(e - 1));
    CHECK(ptmap_lanes(m, w) == kLanes[c], "w %d of class %d has %d lanes", w, c, ptmap_lanes(m, w));
    CHECK(ptmap_wg_points(ptmap_lanes(m, w)) == kPoints[c], "class %d: %d points per workgroup", c, ptmap_wg_points(ptmap_lanes(m, w)));
    CHECK(e - f <= kPoints[c] && (e - f) * (kLanes[c] ? kLanes[c] : 8) <= 256, "w %d holds %d points of class %d", w, e - f, c);
    // only the last workgroup of a class may be partly filled
    CHECK(e - f == kPoints[c] || e == first_of[c + 1], "w %d of class %d is short (%d points) before the class ends", w, c, e - f);
    for (int pb = f; pb < e; pb++) CHECK(ptmap_wg_of(m, pb) == w, "point %d: wg_of %d, lies in %d", pb, ptmap_wg_of(m, pb), w);
    next = e;
    visited++;
  }
  if (npb) {
    CHECK(next == npb, "the workgroups end at %d of %d points", next, npb);
    CHECK(visited == n_wg, "visited %d workgroups, ptmap_n_wg %d", visited, n_wg);
  }
  // and from the points' side
  for (int pb = 0; pb < npb; pb++) {
    const int w = ptmap_wg_of(m, pb);
    CHECK(w >= 0 && w < n_wg, "point %d: workgroup %d of %d", pb, w, n_wg);
    if (w < 0 || w >= n_wg) continue;
    CHECK(ptmap_wg_first(m, w) <= pb && pb < ptmap_wg_end(m, w), "point %d outside its workgroup %d: [%d, %d)", pb, w, ptmap_wg_first(m, w), ptmap_wg_end(m, w));
  }
}

// Without a point of up to 4 rows the workgroups are those of the three-class map (S up to 8 rows, L, X) that preceded the
// 4-lane class, stated here on its own: the point order and every sum over workgroups then stay what they were.
static void check_three_class(int nS, int nL, int nX) {
  // (and so does a problem too small for the 4-lane class: its short points are S points)
  const int n[PTMAP_CLASSES] = {nS / 3, nS - nS / 3, nL, nX};
  const PtMap m = ptmap_make(n, false);
  const int wS = (nS + 31) / 32, wL = (nL + 15) / 16, n_wg = wS + wL + (nX + 31) / 32;
  CHECK(ptmap_n_wg(m) == (n_wg > 0 ? n_wg : 1), "n_wg %d, three-class %d", ptmap_n_wg(m), n_wg);
  for (int w = 0; w < n_wg; w++) {
    const int lanes = w < wS ? 8 : w < wS + wL ? 16 : 0;
    const int first = w < wS ? 32 * w : w < wS + wL ? nS + 16 * (w - wS) : nS + nL + 32 * (w - wS - wL);
    const int cap = w < wS ? nS : w < wS + wL ? nS + nL : nS + nL + nX;
    const int end = first + (lanes == 16 ? 16 : 32) < cap ? first + (lanes == 16 ? 16 : 32) : cap;
    CHECK(ptmap_lanes(m, w) == lanes && ptmap_wg_first(m, w) == first && ptmap_wg_end(m, w) == end, "w %d: %d lanes [%d, %d), three-class %d lanes [%d, %d)",
          w, ptmap_lanes(m, w), ptmap_wg_first(m, w), ptmap_wg_end(m, w), lanes, first, end);
  }
}

int main() {
  CHECK(!ptmap_use_lanes4(24576, -1) && ptmap_use_lanes4(24577, -1) && ptmap_use_lanes4(1, 0) && !ptmap_use_lanes4(0, 0) && !ptmap_use_lanes4(100, 100) && ptmap_use_lanes4(101, 100),
        "ptmap_use_lanes4 thresholds");
  // track length -> class
  for (int rows = 0; rows <= 40; rows++) {
    const int want = rows <= 4 ? 0 : rows <= 8 ? 1 : rows <= 16 ? 2 : 3;
    CHECK(ptmap_class(rows) == want, "rows %d: class %d", rows, ptmap_class(rows));
  }
  // every combination of the edge counts of each class: none, one, a full workgroup, one short, one over, two and one over
  int cases = 0;
  for (int a : {0, 1, 63, 64, 65, 129})
    for (int b : {0, 1, 31, 32, 33, 65})
      for (int c : {0, 1, 15, 16, 17, 33})
        for (int d : {0, 1, 31, 32, 33, 65}) { const int n[PTMAP_CLASSES] = {a, b, c, d}; check_counts(n); cases++; }
  for (int b : {0, 1, 31, 32, 33, 65, 1000})
    for (int c : {0, 1, 15, 16, 17, 33, 500})
      for (int d : {0, 1, 31, 32, 33, 65}) { check_three_class(b, c, d); cases++; }
  std::mt19937 rng(20240611);
  for (int it = 0; it < 400; it++) {
    int n[PTMAP_CLASSES];
    for (int c = 0; c < PTMAP_CLASSES; c++) {
      const unsigned r = rng();
      n[c] = (r & 3) == 0 ? 0 : (r & 3) == 1 ? (int)((r >> 2) % 5) * kPoints[c] : (int)((r >> 2) % 3000);   // zeros, exact multiples, anything
    }
    check_counts(n);
    cases++;
  }
  if (fails) { std::printf("ptmap_host_check: %d failures\n", fails); return 1; }
  std::printf("ptmap_host_check ok: %d class-count cases\n", cases);
  return 0;
}
