// PrimTmp and the rocPRIM wrappers (metricsfm_amd/csrc/prim_device.h), and wg_rank (common.h), on their own: a stand-alone
// program with its own context, error sink and block "pool", like devscope_check.cc.  The pool counts the allocations, records
// hipStreamQuery(stream) at every free and keeps the block until the case is over.
//   case 1  a function with a PrimTmp, a DevScope and a 512 MiB hipMemsetAsync in flight enqueues a small scan, a larger sort and a
//           scan in between; left through finish() and through HIP_TRY, it gives nothing back before it returns, every free finds
//           the stream drained, and fit allocates exactly as often as the need grows
//   case 2  the wrappers' results against the host, exactly; n == 0
//   case 3  wg_rank<W>, twice per round on one `part`, against the host's ordered compaction
// tests/test_gpu_primtmp.py builds and runs it.
#include <numeric>

#include "prim_device.h"

typedef unsigned long long u64;

static hipStream_t g_stream;
static hipEvent_t g_ev0, g_ev1;
static std::vector<hipError_t> g_query;   // the stream's state at each free
static std::vector<void*> g_freed;
static int g_allocs = 0, g_errors_set = 0;

int msfm_set_error(msfm_ctx*, int code, const char*, ...) { g_errors_set++; return code; }
hipError_t msfm_pool_alloc(void** p, size_t bytes, size_t* capacity) { g_allocs++; *capacity = bytes; return hipMalloc(p, bytes); }
void msfm_pool_free(void* p, size_t) {
  g_query.push_back(hipStreamQuery(g_stream));
  g_freed.push_back(p);
}

#define CHECK(e)                                                                                  \
  do {                                                                                            \
    const hipError_t e_ = (e);                                                                    \
    if (e_ != hipSuccess) { printf("%s:%d %s -> %s\n", __FILE__, __LINE__, #e, hipGetErrorString(e_)); return 3; } \
  } while (0)

static const size_t BIG = (size_t)512 << 20;
static const size_t N_SCAN1 = 1000, N_SORT = 300000, N_SCAN2 = 200000, N_INCL = 70000, SEG_LEN[3] = {0, 5, 4000};
static const unsigned SORT_BITS = 10;   // keys below 1000
static hipError_t refused() { return hipErrorInvalidValue; }   // (no call is made that could fail)

static int drop_freed() {
  for (void* p : g_freed) CHECK(hipFree(p));
  g_freed.clear();
  g_query.clear();
  return 0;
}

// what fit has to allocate for this sequence of needs, starting without a block
static int grows(std::initializer_list<size_t> needs) {
  size_t cap = 0;
  int n = 0;
  for (size_t b : needs)
    if (n == 0 || b > cap) { cap = std::max<size_t>(1, b); n++; }
  return n;
}

struct Case1 { size_t frees_inside = 0; int fit_allocs = 0, last_scan_allocs = 0, blocks = 0; };

// the small scan, the sort, the scan in between, behind the memset; leave 0: HIP_TRY, 1: finish()
static int owner(msfm_ctx* ctx, int leave, Case1* r) {
  hipStream_t s = ctx->stream;
  DevBuf<char> big;
  DevBuf<int> a, a_out, v, v_out, b, b_out;
  DevBuf<u64> k, k_out;
  PrimTmp tmp;
  DevScope sc(ctx);
  const int allocs_at_entry = g_allocs;
  HIP_TRY(ctx, big.alloc(BIG));
  HIP_TRY(ctx, hip_first_error({a.alloc(N_SCAN1), a_out.alloc(N_SCAN1), k.alloc(N_SORT), k_out.alloc(N_SORT), v.alloc(N_SORT), v_out.alloc(N_SORT),
                                b.alloc(N_SCAN2), b_out.alloc(N_SCAN2)}));
  HIP_TRY(ctx, hipMemsetAsync(a.p, 0, sizeof(int) * N_SCAN1, s)); HIP_TRY(ctx, hipMemsetAsync(k.p, 0, sizeof(u64) * N_SORT, s));
  HIP_TRY(ctx, hipMemsetAsync(v.p, 0, sizeof(int) * N_SORT, s)); HIP_TRY(ctx, hipMemsetAsync(b.p, 0, sizeof(int) * N_SCAN2, s));
  HIP_TRY(ctx, hipEventRecord(g_ev0, s));
  HIP_TRY(ctx, hipMemsetAsync(big.p, 1, BIG, s));
  HIP_TRY(ctx, hipEventRecord(g_ev1, s));
  const int before_prims = g_allocs;
  HIP_TRY(ctx, prim_scan_excl(tmp, a.p, a_out.p, N_SCAN1, s));
  HIP_TRY(ctx, prim_sort_pairs(tmp, k.p, k_out.p, v.p, v_out.p, N_SORT, 0u, SORT_BITS, s));
  const int before_last = g_allocs;
  HIP_TRY(ctx, prim_scan_excl(tmp, b.p, b_out.p, N_SCAN2, s));
  r->fit_allocs = g_allocs - before_prims;
  r->last_scan_allocs = g_allocs - before_last;
  r->blocks = g_allocs - allocs_at_entry;
  r->frees_inside = g_query.size();
  if (leave == 0) HIP_TRY(ctx, refused());
  HIP_TRY(ctx, sc.finish());
  r->frees_inside = g_query.size();   // (behind the wait, and still nothing has gone back)
  return MSFM_OK;
}

static int case1(msfm_ctx* ctx, int* bad) {
  // the three needs, asked of rocPRIM directly
  size_t need[3] = {0, 0, 0};
  CHECK(rocprim::exclusive_scan(nullptr, need[0], (const int*)nullptr, (int*)nullptr, 0, N_SCAN1, rocprim::plus<int>(), g_stream));
  CHECK(rocprim::radix_sort_pairs(nullptr, need[1], (const u64*)nullptr, (u64*)nullptr, (const int*)nullptr, (int*)nullptr, N_SORT, 0u, SORT_BITS, g_stream));
  CHECK(rocprim::exclusive_scan(nullptr, need[2], (const int*)nullptr, (int*)nullptr, 0, N_SCAN2, rocprim::plus<int>(), g_stream));
  const int want = grows({need[0], need[1], need[2]});
  const char* name[2] = {"HIP_TRY", "finish"};
  for (int leave = 0; leave < 2; leave++) {
    const int errors_before = g_errors_set;
    Case1 r;
    const int rc = owner(ctx, leave, &r);
    CHECK(hipStreamSynchronize(g_stream));
    float ms = 0.f;
    CHECK(hipEventElapsedTime(&ms, g_ev0, g_ev1));
    int not_ready = 0;
    for (hipError_t q : g_query) not_ready += q != hipSuccess;
    const bool rc_ok = leave == 0 ? (rc == MSFM_E_DEVICE && g_errors_set == errors_before + 1) : rc == MSFM_OK;
    const bool ok = rc_ok && r.frees_inside == 0 && not_ready == 0 && r.fit_allocs == want && r.last_scan_allocs == 0 && (int)g_query.size() == r.blocks;
    printf("case 1 %-8s rc=%d needs=%zu,%zu,%zu fit_allocs=%d (want %d) last_scan_allocs=%d frees_inside=%zu frees=%zu of %d busy_at_free=%d memset_us=%.1f %s\n",
           name[leave], rc, need[0], need[1], need[2], r.fit_allocs, want, r.last_scan_allocs, r.frees_inside, g_query.size(), r.blocks, not_ready, ms * 1e3,
           ok ? "ok" : "FAILED");
    if (!ok) *bad = 1;
    if (ms * 1e3 < 50.0) { printf("the memset took under 50 us: the case proves nothing\n"); *bad = 2; }
    if (drop_freed()) return 3;
  }
  return 0;
}

static uint32_t lcg(uint32_t& x) { x = x * 1664525u + 1013904223u; return x >> 8; }

static int results(msfm_ctx* ctx, bool* ok) {
  hipStream_t s = ctx->stream;
  uint32_t seed = 12345u;
  std::vector<int> a(N_SCAN1), b(N_SCAN2), v(N_SORT);
  std::vector<u64> k(N_SORT), w(N_INCL), g(SEG_LEN[0] + SEG_LEN[1] + SEG_LEN[2]);
  for (int& x : a) x = (int)(lcg(seed) % 7);
  for (int& x : b) x = (int)(lcg(seed) % 5);
  for (u64& x : k) x = lcg(seed) % 1000;   // 300 copies of every key: the values show the order among them
  std::iota(v.begin(), v.end(), 0);
  for (u64& x : w) x = ((u64)lcg(seed) << 20) | lcg(seed);
  for (u64& x : g) x = ((u64)lcg(seed) << 40) ^ lcg(seed);
  const std::vector<int> seg_b = {0, 0, (int)SEG_LEN[1]}, seg_e = {0, (int)SEG_LEN[1], (int)g.size()};
  DevBuf<int> d_a, d_ao, d_b, d_bo, d_v, d_vo, d_sb, d_se;
  DevBuf<u64> d_k, d_ko, d_w, d_wo, d_g, d_go;
  PrimTmp tmp;
  DevScope sc(ctx);
  HIP_TRY(ctx, hip_first_error({sc.up(d_a, a), sc.up(d_b, b), sc.up(d_v, v), sc.up(d_k, k), sc.up(d_w, w), sc.up(d_g, g), sc.up(d_sb, seg_b), sc.up(d_se, seg_e)}));
  HIP_TRY(ctx, hip_first_error({d_ao.alloc(a.size()), d_bo.alloc(b.size()), d_vo.alloc(v.size()), d_ko.alloc(k.size()), d_wo.alloc(w.size()), d_go.alloc(g.size())}));
  HIP_TRY(ctx, prim_scan_excl(tmp, d_a.p, d_ao.p, a.size(), s));
  HIP_TRY(ctx, prim_sort_pairs(tmp, d_k.p, d_ko.p, d_v.p, d_vo.p, k.size(), 0u, SORT_BITS, s));
  HIP_TRY(ctx, prim_scan_excl(tmp, d_b.p, d_bo.p, b.size(), s));
  HIP_TRY(ctx, prim_scan_incl(tmp, d_w.p, d_wo.p, w.size(), s));
  HIP_TRY(ctx, prim_seg_sort_keys(tmp, d_g.p, d_go.p, (unsigned)g.size(), 3u, d_sb.p, d_se.p, 0u, 64u, s));
  std::vector<int> ao(a.size()), bo(b.size()), vo(v.size());
  std::vector<u64> ko(k.size()), wo(w.size()), go(g.size());
  HIP_TRY(ctx, hip_first_error({sc.down(ao.data(), d_ao.p, ao.size()), sc.down(bo.data(), d_bo.p, bo.size()), sc.down(vo.data(), d_vo.p, vo.size()),
                                sc.down(ko.data(), d_ko.p, ko.size()), sc.down(wo.data(), d_wo.p, wo.size()), sc.down(go.data(), d_go.p, go.size())}));
  HIP_TRY(ctx, sc.finish());
  // the host's answers
  std::vector<int> ar(a.size()), br(b.size()), vr = v;
  std::vector<u64> kr(k.size()), wr(w.size()), gr = g;
  int run = 0;
  for (size_t i = 0; i < a.size(); i++) { ar[i] = run; run += a[i]; }
  run = 0;
  for (size_t i = 0; i < b.size(); i++) { br[i] = run; run += b[i]; }
  std::stable_sort(vr.begin(), vr.end(), [&](int x, int y) { return k[x] < k[y]; });
  for (size_t i = 0; i < k.size(); i++) kr[i] = k[vr[i]];
  u64 sum = 0;
  for (size_t i = 0; i < w.size(); i++) { sum += w[i]; wr[i] = sum; }
  for (int j = 0; j < 3; j++) std::sort(gr.begin() + seg_b[j], gr.begin() + seg_e[j]);
  const bool o_a = ao == ar, o_b = bo == br, o_s = ko == kr && vo == vr, o_w = wo == wr, o_g = go == gr;
  printf("case 2 scan %zu %s, sort %zu %s, scan %zu %s, inclusive u64 scan %zu %s, segmented sort 0+5+4000 %s\n", a.size(), o_a ? "ok" : "FAILED", k.size(),
         o_s ? "ok" : "FAILED", b.size(), o_b ? "ok" : "FAILED", w.size(), o_w ? "ok" : "FAILED", o_g ? "ok" : "FAILED");
  *ok = o_a && o_b && o_s && o_w && o_g;
  return MSFM_OK;
}

static bool nothing(hipStream_t s) {   // n == 0: success, no rocPRIM, no block
  PrimTmp tmp;
  const int before = g_allocs;
  const hipError_t e = hip_first_error({prim_scan_excl(tmp, (const int*)nullptr, (int*)nullptr, 0, s), prim_scan_incl(tmp, (const u64*)nullptr, (u64*)nullptr, 0, s),
                                        prim_sort_pairs(tmp, (const u64*)nullptr, (u64*)nullptr, (const int*)nullptr, (int*)nullptr, 0, 0u, 64u, s),
                                        prim_sort_keys(tmp, (const u64*)nullptr, (u64*)nullptr, 0, 0u, 64u, s),
                                        prim_seg_sort_keys(tmp, (const u64*)nullptr, (u64*)nullptr, 0u, 3u, (const int*)nullptr, (const int*)nullptr, 0u, 64u, s),
                                        prim_seg_sort_pairs(tmp, (const u64*)nullptr, (u64*)nullptr, (const int*)nullptr, (int*)nullptr, 0u, 3u, (const int*)nullptr,
                                                            (const int*)nullptr, 0u, 64u, s)});
  const bool ok = e == hipSuccess && g_allocs == before && tmp.cur.p == nullptr && tmp.retired.empty();
  printf("case 2 n == 0 %s\n", ok ? "ok" : "FAILED");
  return ok;
}

// one workgroup of 64 * W lanes walks n flags in rounds; the set flags' indices to out_set in order, the clear ones' to out_clr
template <int W>
__global__ __launch_bounds__(64 * W) void k_rank(int n, const uint8_t* __restrict__ flag, int* __restrict__ out_set, int* __restrict__ out_clr,
                                                 int* __restrict__ totals) {
  __shared__ int part[W];
  int ns = 0, nc = 0;
  for (int c0 = 0; c0 < n; c0 += 64 * W) {   // (uniform trip count)
    const int i = c0 + threadIdx.x;
    const bool set = i < n && flag[i] != 0, clr = i < n && flag[i] == 0;
    int tot;
    const int rs = wg_rank<W>(set, part, tot);
    if (set) out_set[ns + rs] = i;
    ns += tot;
    const int rc = wg_rank<W>(clr, part, tot);   // the same `part` at once
    if (clr) out_clr[nc + rc] = i;
    nc += tot;
  }
  if (threadIdx.x == 0) { totals[0] = ns; totals[1] = nc; }
}

template <int W>
static int ranks(msfm_ctx* ctx, bool* ok) {
  const int n = 2 * 64 * W + 37;
  const char* name[4] = {"none", "all", "every third", "pseudo-random"};
  *ok = true;
  for (int pat = 0; pat < 4; pat++) {
    uint32_t seed = 777u + W;
    std::vector<uint8_t> f(n);
    for (int i = 0; i < n; i++) f[i] = pat == 0 ? 0 : pat == 1 ? 1 : pat == 2 ? (i % 3 == 0) : (lcg(seed) & 1);
    std::vector<int> want_set, want_clr;
    for (int i = 0; i < n; i++) (f[i] ? want_set : want_clr).push_back(i);
    DevBuf<uint8_t> d_f;
    DevBuf<int> d_set, d_clr, d_tot;
    DevScope sc(ctx);
    HIP_TRY(ctx, sc.up(d_f, f));
    HIP_TRY(ctx, hip_first_error({d_set.alloc(n), d_clr.alloc(n), d_tot.alloc(2)}));
    HIP_TRY(ctx, hipMemsetAsync(d_set.p, 0xff, sizeof(int) * n, sc.s)); HIP_TRY(ctx, hipMemsetAsync(d_clr.p, 0xff, sizeof(int) * n, sc.s));
    hipLaunchKernelGGL(k_rank<W>, dim3(1), dim3(64 * W), 0, sc.s, n, d_f.p, d_set.p, d_clr.p, d_tot.p);
    HIP_TRY(ctx, hipGetLastError());
    std::vector<int> set(n), clr(n);
    int tot[2] = {-1, -1};
    HIP_TRY(ctx, hip_first_error({sc.down(set.data(), d_set.p, set.size()), sc.down(clr.data(), d_clr.p, clr.size()), sc.down(tot, d_tot.p, 2)}));
    HIP_TRY(ctx, sc.finish());
    const bool totals_ok = tot[0] == (int)want_set.size() && tot[1] == (int)want_clr.size();
    want_set.resize(n, -1); want_clr.resize(n, -1);   // (behind the last rank nothing was written)
    const bool o = totals_ok && set == want_set && clr == want_clr;
    printf("case 3 wg_rank<%d> %-13s n=%d set=%d clear=%d %s\n", W, name[pat], n, tot[0], tot[1], o ? "ok" : "FAILED");
    if (!o) *ok = false;
  }
  return MSFM_OK;
}

int main() {
  CHECK(hipSetDevice(0));
  CHECK(hipStreamCreate(&g_stream));
  CHECK(hipEventCreate(&g_ev0)); CHECK(hipEventCreate(&g_ev1));
  msfm_ctx ctx;
  ctx.stream = g_stream;
  {   // a first touch of the device, so that no case pays for it
    void* warm = nullptr;
    CHECK(hipMalloc(&warm, BIG));
    CHECK(hipMemsetAsync(warm, 0, BIG, g_stream));
    CHECK(hipStreamSynchronize(g_stream));
    CHECK(hipFree(warm));
  }
  int bad = 0;
  if (case1(&ctx, &bad)) return 3;
  bool ok = false;
  if (results(&ctx, &ok) != MSFM_OK || !ok) bad = 1;
  if (!nothing(g_stream)) bad = 1;
  bool r1 = false, r2 = false, r4 = false, r16 = false;
  if (ranks<1>(&ctx, &r1) != MSFM_OK || ranks<2>(&ctx, &r2) != MSFM_OK || ranks<4>(&ctx, &r4) != MSFM_OK || ranks<16>(&ctx, &r16) != MSFM_OK ||
      !r1 || !r2 || !r4 || !r16)
    bad = 1;
  if (drop_freed()) return 3;
  CHECK(hipEventDestroy(g_ev0)); CHECK(hipEventDestroy(g_ev1));
  CHECK(hipStreamDestroy(g_stream));
  if (!bad) printf("primtmp_check ok\n");
  return bad;
}
