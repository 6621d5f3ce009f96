// The children of a context (metricsfm_amd/csrc/common.h: child_new, Child, msfm_child_destroy) on their own: a stand-alone
// program with its own context, error sink, block "pool" and msfm_ctx_child_released.  The pool's free records
// hipStreamQuery(stream) at the moment of each free and keeps the block until the case is over; the release is recorded in the
// same log, so the order "frees on a drained stream, then the release" can be read off it.  A dummy child type with two blocks:
//   1  a create that fails through HIP_TRY on a made-up error value with a 512 MiB hipMemsetAsync in flight in its own block
//   2  the same create succeeds; the child is destroyed with a second memset in flight
//   3  a child that holds no block is destroyed with a memset in flight elsewhere: no wait
//   4  destroy of a null pointer
// tests/test_gpu_child.py builds and runs it.
#include "common.h"

static hipStream_t g_stream;
static hipEvent_t g_ev0, g_ev1;
struct Entry { char what; hipError_t query; };   // 'F' a free and the stream's state at it, 'R' a release
static std::vector<Entry> g_log;
static std::vector<void*> g_freed;
static int g_errors_set = 0;

int msfm_set_error(msfm_ctx*, int code, const char*, ...) { g_errors_set++; return code; }
hipError_t msfm_pool_alloc(void** p, size_t bytes, size_t* capacity) { *capacity = bytes; return hipMalloc(p, bytes); }
void msfm_pool_free(void* p, size_t) {
  g_log.push_back({'F', hipStreamQuery(g_stream)});
  g_freed.push_back(p);
}
void msfm_ctx_child_released(msfm_ctx* ctx) {
  ctx->children--;
  g_log.push_back({'R', hipSuccess});
}

#define CHECK(e)                                                                                  \
  do {                                                                                            \
    const hipError_t e_ = (e);                                                                    \
    if (e_ != hipSuccess) { printf("%s:%d %s -> %s\n", __FILE__, __LINE__, #e, hipGetErrorString(e_)); return 3; } \
  } while (0)

static const size_t BIG = (size_t)512 << 20;
static hipError_t refused() { return hipErrorInvalidValue; }   // (no call is made that could fail)

struct Dummy {
  msfm_ctx* ctx = nullptr;
  DevBuf<char> big;
  DevBuf<int> small;
};
static inline bool child_holds_blocks(const Dummy* D) { return D->big.p != nullptr; }

static hipError_t timed_memset(void* p, hipStream_t s) {
  return hip_first_error({hipEventRecord(g_ev0, s), hipMemsetAsync(p, 1, BIG, s), hipEventRecord(g_ev1, s)});
}

static int dummy_create(msfm_ctx* ctx, bool fail, Dummy** out) {
  *out = nullptr;
  Child<Dummy> D = child_new<Dummy>(ctx);
  HIP_TRY(ctx, D->big.alloc(BIG)); HIP_TRY(ctx, D->small.alloc(5));
  HIP_TRY(ctx, timed_memset(D->big.p, ctx->stream));
  if (fail) HIP_TRY(ctx, refused());
  *out = D.release();
  return MSFM_OK;
}

// the log of a case: `frees` frees, each on a drained stream, then exactly one release
static bool log_ok(size_t frees) {
  if (g_log.size() != frees + 1) return false;
  for (size_t i = 0; i < frees; i++)
    if (g_log[i].what != 'F' || g_log[i].query != hipSuccess) return false;
  return g_log[frees].what == 'R';
}
static int memset_long_enough(int* bad) {
  float ms = 0.f;
  CHECK(hipStreamSynchronize(g_stream));
  CHECK(hipEventElapsedTime(&ms, g_ev0, g_ev1));
  if (ms * 1e3 < 50.0) { printf("the memset took under 50 us: the case proves nothing\n"); *bad = 2; }
  return 0;
}
static int end_case() {
  g_log.clear();
  for (void* p : g_freed) CHECK(hipFree(p));
  g_freed.clear();
  return 0;
}

int main() {
  CHECK(hipSetDevice(0));
  CHECK(hipStreamCreate(&g_stream));
  CHECK(hipEventCreate(&g_ev0)); CHECK(hipEventCreate(&g_ev1));
  msfm_ctx ctx;
  ctx.stream = g_stream;
  void* other = nullptr;   // a block no child owns; its first memset is the first touch of the device, so that no case pays for it
  CHECK(hipMalloc(&other, BIG));
  CHECK(hipMemsetAsync(other, 0, BIG, g_stream));
  CHECK(hipStreamSynchronize(g_stream));
  int bad = 0;
  {   // 1: the failed create takes the destroy path
    const int children = ctx.children, errors = g_errors_set;
    Dummy* D = reinterpret_cast<Dummy*>(&ctx);   // (anything but null)
    const int rc = dummy_create(&ctx, true, &D);
    const bool ok = rc == MSFM_E_DEVICE && g_errors_set == errors + 1 && D == nullptr && ctx.children == children && log_ok(2);
    printf("case failed-create  rc=%d log=%zu children=%d %s\n", rc, g_log.size(), ctx.children, ok ? "ok" : "FAILED");
    if (!ok) bad = 1;
    if (memset_long_enough(&bad) || end_case()) return 3;
  }
  {   // 2: hand-over, then destroy with work in flight
    const int children = ctx.children;
    Dummy* D = nullptr;
    const int rc = dummy_create(&ctx, false, &D);
    bool ok = rc == MSFM_OK && D != nullptr && ctx.children == children + 1 && g_log.empty();
    if (D) {
      CHECK(timed_memset(D->big.p, g_stream));
      msfm_child_destroy(D);
    }
    ok = ok && ctx.children == children && log_ok(2);
    printf("case destroy        rc=%d log=%zu children=%d %s\n", rc, g_log.size(), ctx.children, ok ? "ok" : "FAILED");
    if (!ok) bad = 1;
    if (memset_long_enough(&bad) || end_case()) return 3;
  }
  {   // 3: no block, no wait
    const int children = ctx.children;
    Dummy* D = child_new<Dummy>(&ctx).release();
    CHECK(timed_memset(other, g_stream));
    msfm_child_destroy(D);
    const hipError_t q = hipStreamQuery(g_stream);
    const bool ok = q == hipErrorNotReady && ctx.children == children && log_ok(0);
    printf("case no-block       query=%d log=%zu children=%d %s\n", (int)q, g_log.size(), ctx.children, ok ? "ok" : "FAILED");
    if (q == hipSuccess) { printf("the memset had finished before the query: the case proves nothing\n"); bad = 2; }
    else if (!ok) bad = 1;
    if (memset_long_enough(&bad) || end_case()) return 3;
  }
  {   // 4: null
    const int children = ctx.children;
    msfm_child_destroy(static_cast<Dummy*>(nullptr));
    const bool ok = ctx.children == children && g_log.empty();
    printf("case null           log=%zu children=%d %s\n", g_log.size(), ctx.children, ok ? "ok" : "FAILED");
    if (!ok) bad = 1;
  }
  CHECK(hipFree(other));
  CHECK(hipEventDestroy(g_ev0)); CHECK(hipEventDestroy(g_ev1));
  CHECK(hipStreamDestroy(g_stream));
  if (!bad) printf("child_check ok\n");
  return bad;
}
