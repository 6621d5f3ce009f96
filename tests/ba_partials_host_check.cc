// Host walk of the layout of the BA partial-sum buffers (BaPartials, metricsfm_amd/csrc/ba_partials.h): for the edge values of
// every input and seeded random cases, the segments of each buffer lie in order without gap or overlap, every reduce count is
// the sum of the segments its rank includes, nothing reaches past the stated need of its buffer, and - where the size formula
// that preceded the layout sufficed - the need does not exceed that formula, slack included (the layout did not grow memory).
// A stand-alone program: host only, never loaded into another process, built with -fsanitize=address,undefined.
#include <algorithm>
#include <cstdio>
#include <random>
#include <vector>

#include "ba_partials.h"

static int fails = 0;
#define CHECK(c, ...) do { if (!(c)) { if (fails++ < 20) { std::printf("FAIL %s:%d %s | ", __FILE__, __LINE__, #c); std::printf(__VA_ARGS__); std::printf("\n"); } } } while (0)

static int cdiv(long a, long b) { return (int)((a + b - 1) / b); }

// the segments of one buffer in order; returns their end
static int walk(const char* name, const std::vector<BaSeg>& segs, int need) {
  int at = 0;
  for (size_t i = 0; i < segs.size(); i++) {
    CHECK(segs[i].n >= 0, "%s: segment %zu has %d entries", name, i, segs[i].n);
    CHECK(segs[i].off == at, "%s: segment %zu starts at %d, the one before ends at %d", name, i, segs[i].off, at);
    at = segs[i].off + segs[i].n;
    CHECK(at <= need, "%s: segment %zu ends at %d, need %d", name, i, at, need);
  }
  return at;
}

struct Case { int A, AE, ncb, nmb, npb, nblk_pt; bool has_gps; };

static void check(const Case& c) {
  const int nred = 6 * c.ncb + 3 * c.nmb;   // (0 without a camera or intrinsics block: no reduced system)
  const BaPartials L = ba_partials(c.A, c.AE, c.ncb, c.nmb, nred, c.npb, c.nblk_pt, c.has_gps);
  const int n_gps = c.has_gps ? cdiv(c.ncb, 256) : 0, nbp = c.npb ? c.nblk_pt : 0;
  // the segments are what the kernels' launches write (stated here on their own)
  CHECK(L.x_point.n == c.nblk_pt && L.x_frozen.n == cdiv(c.A - c.AE, 256) && L.x_gps.n == n_gps, "partial_x segments");
  CHECK(L.u_step.n == (nred > 0 ? cdiv(nred, 256) : 0) && L.u_point.n == nbp, "partial2 segments");
  CHECK(L.m_point.n == nbp && L.m_rest[0].n == cdiv(c.A - c.AE, 256) && L.m_rest[1].n == cdiv(c.A - c.AE + (c.has_gps ? c.ncb : 0), 256), "partial segments");
  CHECK(L.c_rows.n == cdiv(std::max(1, c.A), 256) && L.c_gps.n == n_gps, "partial4 segments");
  CHECK(L.g_point.n == c.nblk_pt && L.g_cam.n == 6 * c.ncb && L.g_model.n == 3 * c.nmb, "gmax_buf segments");
  // in order, disjoint, without gap, inside the need; the reduce counts are the sums of the segments the rank includes
  const int ex = walk("partial_x", {L.x_point, L.x_frozen, L.x_gps}, L.need_x);
  CHECK(L.sum_x[1] == ex && L.sum_x[0] == ex - L.x_gps.n, "partial_x counts %d / %d, end %d", L.sum_x[1], L.sum_x[0], ex);
  const int eu = walk("partial2", {L.u_step, L.u_point}, L.need_u);
  CHECK(L.sum_u == eu, "partial2 count %d, end %d", L.sum_u, eu);
  for (int lead = 0; lead < 2; lead++) {
    const int em = walk("partial", {L.m_point, L.m_rest[lead]}, L.need_m);
    CHECK(L.sum_m[lead] == em, "partial count %d of rank kind %d, end %d", L.sum_m[lead], lead, em);
  }
  const int ec = walk("partial4", {L.c_rows, L.c_gps}, L.need_c);
  CHECK(L.sum_c[1] == ec && L.sum_c[0] == ec - L.c_gps.n, "partial4 counts %d / %d, end %d", L.sum_c[1], L.sum_c[0], ec);
  const int eg = walk("gmax_buf", {L.g_point, L.g_cam, L.g_model}, L.need_g);
  CHECK(L.sum_g == eg, "gmax_buf count %d, end %d", L.sum_g, eg);
  // the needs are exact: the end of the lead rank's last segment (another rank's reach less far)
  CHECK(L.need_x == ex && L.need_u == eu && L.need_m == L.sum_m[1] && L.need_m >= L.sum_m[0] && L.need_c == ec && L.need_g == eg, "needs");
  // the size every one of the five buffers had before: nblk_obs + nblk_pt + cdiv(max(1, ncb), 256) + 64 (and gmax_buf's own + 8)
  const long before = (long)cdiv(std::max(1, c.A), 256) + c.nblk_pt + cdiv(std::max(1, c.ncb), 256) + 64;
  if (std::max(eu, std::max(ex, std::max(ec, L.sum_m[1]))) <= before)
    CHECK(L.need_x <= before && L.need_u <= before && L.need_m <= before && L.need_c <= before, "needs %d %d %d %d exceed the size before, %ld",
          L.need_x, L.need_u, L.need_m, L.need_c, before);
  // only the step's partials can need more than that, and only by their own segment
  CHECK(L.need_x <= before - 64 && L.need_m <= before - 64 && L.need_c <= before - 64, "partial_x / partial / partial4 need %d %d %d, before %ld", L.need_x,
        L.need_m, L.need_c, before);
  CHECK(L.need_g <= (long)c.nblk_pt + 6L * c.ncb + 3L * c.nmb + 8, "gmax_buf needs %d", L.need_g);
}

int main() {
  int cases = 0;
  // the edge values of every input, in every combination
  for (int AE : {0, 1, 255, 256, 257, 70000})
    for (int frozen : {0, 1, 256, 1000})           // A - AE (0: A == AE; with AE = 0, frozen = 0: A = 0)
      for (int ncb : {0, 1, 42, 43, 256, 257, 4000})
        for (int nmb : {0, 1, 7})
          for (int npb : {0, 1, 5000})
            for (int gps = 0; gps < 2; gps++) {
              const int nblk_pt = npb == 0 ? 1 : npb == 1 ? 1 : 180;   // (no eliminated point: k_point's one workgroup)
              const Case c{AE + frozen, AE, ncb, nmb, npb, nblk_pt, gps != 0};
              check(c);
              cases++;
            }
  // far more scalars in the reduced system than rows: the step's partials need more than the size before
  {
    const Case c{20, 20, 4000, 0, 4, 1, true};
    const BaPartials L = ba_partials(c.A, c.AE, c.ncb, c.nmb, 6 * c.ncb, c.npb, c.nblk_pt, true);
    CHECK(L.u_step.n == 94 && L.need_u == 95 && L.need_u > 1 + 1 + 16 + 64, "the many-cameras case needs %d", L.need_u);
    check(c);
    cases++;
  }
  std::mt19937 rng(20241019);
  auto draw = [&](int hi) { const unsigned r = rng(); return (r & 3) == 0 ? 0 : (r & 3) == 1 ? (int)((r >> 2) % 5) * 256 : (int)((r >> 2) % (unsigned)hi); };
  for (int it = 0; it < 600; it++) {
    Case c;
    c.AE = draw(300000); c.A = c.AE + draw(5000);
    c.ncb = draw(6000); c.nmb = draw(40);
    c.npb = c.AE ? 1 + draw(c.AE) % c.AE : 0;
    c.nblk_pt = c.npb ? 1 + (c.npb - 1) / (16 << (rng() % 3)) : 1;
    c.has_gps = (rng() & 1) != 0;
    check(c);
    cases++;
  }
  if (fails) { std::printf("ba_partials_host_check: %d failures\n", fails); return 1; }
  std::printf("ba_partials_host_check ok: %d cases\n", cases);
  return 0;
}
