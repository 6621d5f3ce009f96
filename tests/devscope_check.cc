// DevScope (metricsfm_amd/csrc/common.h) on its own: a stand-alone program with its own context, error sink and block "pool".
// The pool's free records hipStreamQuery(stream) at the moment of each free and keeps the block until the case is over, so the
// queries of a case do not depend on each other.  Three ways out of a function that owns three blocks and has enqueued a
// 512 MiB hipMemsetAsync inside the scope - HIP_TRY on a made-up error value, finish(), dismiss() behind an explicit wait -
// must all free every block on a drained stream.  Then the counting of up().
// tests/test_gpu_devscope.py builds and runs it.
#include "common.h"

static hipStream_t g_stream;
static hipEvent_t g_ev0, g_ev1;
static std::vector<hipError_t> g_query;   // the stream's state at each free
static std::vector<void*> g_freed;
static int g_errors_set = 0;

int msfm_set_error(msfm_ctx*, int code, const char*, ...) { g_errors_set++; return code; }
hipError_t msfm_pool_alloc(void** p, size_t bytes, size_t* capacity) { *capacity = bytes; return hipMalloc(p, bytes); }
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
static hipError_t refused() { return hipErrorInvalidValue; }   // (no call is made that could fail)

// three blocks, the memset between two events; `leave` picks the way out
static int owner(msfm_ctx* ctx, int leave) {
  DevBuf<char> big;
  DevBuf<int> a;
  DevBuf<double> b;
  DevScope sc(ctx);
  HIP_TRY(ctx, big.alloc(BIG)); HIP_TRY(ctx, a.alloc(5)); HIP_TRY(ctx, b.alloc(7));
  HIP_TRY(ctx, hipEventRecord(g_ev0, ctx->stream));
  HIP_TRY(ctx, hipMemsetAsync(big.p, 1, BIG, ctx->stream));
  HIP_TRY(ctx, hipEventRecord(g_ev1, ctx->stream));
  if (leave == 0) HIP_TRY(ctx, refused());
  if (leave == 1) HIP_TRY(ctx, sc.finish());
  if (leave == 2) {
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    sc.dismiss();
  }
  return MSFM_OK;
}

template <typename T>
static int counting(msfm_ctx* ctx, bool* ok) {
  std::vector<T> none, five(5, T(1)), thousand(1000, T(2));
  DevBuf<T> d0, d5, d1000;
  DevScope sc(ctx);
  HIP_TRY(ctx, sc.up(d0, none.data(), none.size())); HIP_TRY(ctx, sc.up(d5, five)); HIP_TRY(ctx, sc.up(d1000, thousand.data(), thousand.size()));
  std::vector<T> back(1000, T(0));
  HIP_TRY(ctx, sc.down(back.data(), d1000.p, back.size()));
  HIP_TRY(ctx, sc.finish());
  *ok = sc.h2d == (int64_t)((5 + 1000) * sizeof(T)) && d0.p != nullptr && d0.cap >= sizeof(T) && back == thousand;
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
  const char* name[3] = {"HIP_TRY", "finish", "dismiss"};
  for (int leave = 0; leave < 3; leave++) {
    g_query.clear();
    const int errors_before = g_errors_set;
    const int rc = owner(&ctx, leave);
    CHECK(hipStreamSynchronize(g_stream));
    float ms = 0.f;
    CHECK(hipEventElapsedTime(&ms, g_ev0, g_ev1));
    int not_ready = 0;
    for (hipError_t q : g_query) not_ready += q != hipSuccess;
    const bool rc_ok = leave == 0 ? (rc == MSFM_E_DEVICE && g_errors_set == errors_before + 1) : rc == MSFM_OK;
    const bool ok = rc_ok && g_query.size() == 3 && not_ready == 0;
    printf("case %-8s rc=%d frees=%zu busy_at_free=%d memset_us=%.1f %s\n", name[leave], rc, g_query.size(), not_ready, ms * 1e3, ok ? "ok" : "FAILED");
    if (!ok) bad = 1;
    if (ms * 1e3 < 50.0) { printf("the memset took under 50 us: the case proves nothing\n"); bad = 2; }
    for (void* p : g_freed) CHECK(hipFree(p));
    g_freed.clear();
  }
  bool ok_i = false, ok_d = false;
  if (counting<int>(&ctx, &ok_i) != MSFM_OK || counting<double>(&ctx, &ok_d) != MSFM_OK || !ok_i || !ok_d) {
    printf("counting FAILED (int %d, double %d)\n", (int)ok_i, (int)ok_d);
    bad = 1;
  } else {
    printf("counting ok\n");
  }
  for (void* p : g_freed) CHECK(hipFree(p));
  CHECK(hipEventDestroy(g_ev0)); CHECK(hipEventDestroy(g_ev1));
  CHECK(hipStreamDestroy(g_stream));
  if (!bad) printf("devscope_check ok\n");
  return bad;
}
