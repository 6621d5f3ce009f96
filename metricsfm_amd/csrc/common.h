// Internal header of libmsfm (not part of the C ABI).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <algorithm>
#include <cstdlib>
#include <functional>
#include <initializer_list>
#include <list>
#include <memory>
#include <string>
#include <thread>
#include <utility>
#include <vector>

#include "../../include/msfm.h"
#include "chol_plan.h"

#define MSFM_API extern "C" __attribute__((visibility("default")))

// Every environment switch of the library, with its default (INTEGRATION.md says what each does).  msfm_env_read() in
// ctx.hip is the only reader of the environment:
//  - the bundle-adjustment and factorisation switches are copied into a problem at msfm_ba_create (msfm_ba::env) and read
//    from there by msfm_ba_run and the factorisation it calls: set them before creating the problem;
//  - the process-wide settings are read once, at first use (msfm_env_process());
//  - MSFM_MULTI_FAIL_RANK is read at the entry of msfm_multi_ba_solve, before the rank threads start.
struct msfm_env {
  int chol_domains = -1;          // MSFM_CHOL_DOMAINS: -1 automatic, 0 dense order, 1..3 that bisection depth
  bool chol_launches = false;     // MSFM_CHOL_LAUNCHES (set): one launch per 64-column panel instead of the persistent chain
  bool chain_force = false;       // MSFM_CHAIN_FORCE (set): the persistent chain whatever the tile count
  bool chain_trace = false;       // MSFM_CHAIN_TRACE (set): the shape of every k_chain launch to stderr (MSFM_CHAIN_BARCHECK build)
  bool create_host = false;       // MSFM_CREATE_HOST=1: msfm_ba_create builds its index structures on the host
  long fold_min = 262144;         // MSFM_FOLD_MIN: camera pairs below which a problem keeps the gather path
  bool no_fold = false;           // MSFM_NO_FOLD (set): the gather path whatever the size
  long lanes4_min = -1;           // MSFM_LANES4_MIN: eliminated points above which those of up to 4 rows get 4 lanes (ptmap_use_lanes4; -1: default)
  bool asm_beside = true;         // MSFM_ASM_BESIDE=0: the Schur fold partials summed after the per-camera sums (k_asm_all), not beside them
  bool spec = true;               // MSFM_SPEC=0: the next linearisation enqueued only after the step's read-back
  bool solve_riders = true;      // MSFM_SOLVE_RIDERS=0: k_modelsum and k_update_params as launches of their own, not inside the factor-and-solve's
  // process-wide
  size_t pool_bytes = (size_t)16384 << 20;   // MSFM_POOL_MB: freed device blocks the cache keeps
  bool pool_debug = false;        // MSFM_POOL_DEBUG (set): a free that disagrees with the pool's record aborts
  int host_threads = 0;           // MSFM_HOST_THREADS (1..64; default min(hardware threads, 8))
  double sync_timeout_s = 120.0;  // MSFM_SYNC_TIMEOUT_S: bound of every host and device wait on a stream or a peer
  int device_share = 1;           // MSFM_DEVICE_SHARE: processes that use this device at the same time
  bool verbose = false;           // MSFM_VERBOSE (set): set-up and solve timings to stderr
  int multi_fail_rank = -1;       // MSFM_MULTI_FAIL_RANK (test hook): this rank of msfm_multi_ba_solve fails before it joins
  int localize_lds_max = 4096;    // MSFM_LOCALIZE_LDS_MAX: longest segment msfm_localize_candidates sorts in LDS (0: all through rocPRIM); read per call
};
msfm_env msfm_env_read();              // the environment as it is now
const msfm_env& msfm_env_process();    // its first reading, kept for the life of the process

struct msfm_ctx {
  int device = 0;
  // the context's one stream: the library opens no other on a context, so whoever waits for it has waited for everything
  // the context enqueued
  hipStream_t stream = nullptr;
  std::string err;
  // multi-GPU hook
  msfm_allreduce_fn allreduce = nullptr;
  void* allreduce_user = nullptr;
  int rank = 0, world = 1;
  // contexts (of this or of other processes) that use this device at the same time, as far as the host has said so
  // (msfm_ctx_create_multi with a shared device; MSFM_DEVICE_SHARE for several processes on one GPU): kernels whose workgroups
  // wait for each other inside a launch must leave room for the others' resident workgroups
  int device_share = 1;
  // per-kernel-class timing (HIP events on `stream`)
  bool profile = false;
  struct Stat { std::string name; uint64_t launches = 0; double ms = 0; };
  std::vector<Stat> stats;
  struct Pending { int stat; hipEvent_t a, b; };
  std::vector<Pending> pending;
  std::vector<hipEvent_t> event_pool;
  // host work arrays of msfm_ba_create, kept between calls (ba.hip): a C3-sized problem touches ~150 MB of them, and
  // mapping + unmapping that much fresh memory on every call cost a quarter of the setup time
  void* ba_scratch = nullptr;
  void (*ba_scratch_free)(void*) = nullptr;
  // objects created from this context that are still alive (Child below); msfm_ctx_destroy refuses while there are any, and
  // the last child of an orphaned context destroys it
  int children = 0;
  bool orphaned = false;
  // native collective (msfm_ctx_init_rccl): librccl handle, communicator and the entry points resolved from it
  void* rccl_lib = nullptr;
  void* rccl_comm = nullptr;
  void* rccl_allreduce = nullptr;
  void* rccl_comm_destroy = nullptr;
  void* rccl_error_string = nullptr;
};
void msfm_ctx_child_released(msfm_ctx* ctx);

// A child of a context: an object the library hands to the caller that keeps its msfm_ctx* (member `ctx`) and, most of them,
// device blocks.  child_new counts it from the moment it exists; the hand-over is `*out = X.release()`.  It goes one way only,
// msfm_child_destroy, which is every public msfm_*_destroy of a child and the deleter of Child: wait for the stream if the
// object holds blocks (they go back to the cache only behind the work that may still use them), delete, and last the release,
// which may destroy the context and the stream with it.  A create that fails with the object in hand therefore takes the same
// path as a destroy.  Whether an object holds blocks: always, unless its type says otherwise beside its definition
// (msfm_seed_set, msfm_localize_set: one block tells; msfm_round_set: host memory only, never).
template <class T>
static inline bool child_holds_blocks(const T*) { return true; }
template <class T>
static inline void msfm_child_destroy(T* obj) {
  if (!obj) return;
  msfm_ctx* ctx = obj->ctx;
  if (child_holds_blocks(obj)) {
    (void)hipSetDevice(ctx->device);   // the caller's thread may have another device current (Python __del__ after set_device)
    (void)hipStreamSynchronize(ctx->stream);
  }
  delete obj;
  msfm_ctx_child_released(ctx);
}
struct ChildDelete {
  template <class T>
  void operator()(T* obj) const { msfm_child_destroy(obj); }
};
template <class T>
using Child = std::unique_ptr<T, ChildDelete>;
template <class T>
static inline Child<T> child_new(msfm_ctx* ctx) {
  Child<T> c(new T());
  c->ctx = ctx;
  ctx->children++;
  return c;
}

int msfm_set_error(msfm_ctx* ctx, int code, const char* fmt, ...);

#define HIP_TRY(ctx, expr)                                                                      \
  do {                                                                                          \
    hipError_t e_ = (expr);                                                                     \
    if (e_ != hipSuccess)                                                                       \
      return msfm_set_error((ctx), MSFM_E_DEVICE, "%s:%d %s -> %s", __FILE__, __LINE__, #expr,  \
                            hipGetErrorString(e_));                                             \
  } while (0)

#define MSFM_TRY(expr)            \
  do {                            \
    int rc_ = (expr);             \
    if (rc_ != MSFM_OK) return rc_; \
  } while (0)

// Scoped kernel-class timer: records two events around a group of launches when
// profiling is on; resolved lazily in msfm_ctx_profile_get.
struct KTimer {
  msfm_ctx* ctx;
  int idx = -1;
  int count = 1;   // kernel launches between the two events (a chain of dependent launches is timed as a whole: an event
                   // pair around every single launch would put its own few microseconds into each of them)
  hipEvent_t a = nullptr, b = nullptr;
  KTimer(msfm_ctx* c, const char* name);
  void stop();   // records the closing event now (the destructor then does nothing)
  ~KTimer();
};

// Device memory comes from a per-process cache of freed blocks (ctx.hip): a bundle adjustment of the incremental loop
// allocates ~60 buffers / > 1 GB, and a fresh VRAM allocation costs far more than the hipMalloc call itself (the first
// kernels that touch it wait 10-20 ms at config 3).  Blocks are returned only after their stream has been synchronised.
// Host wait for a stream that carries a collective: bounded (MSFM_SYNC_TIMEOUT_S, default 120 s) - a peer rank that never
// joins must surface as MSFM_E_DEVICE, not as a host thread inside hipStreamSynchronize for good (ctx.hip).
int msfm_stream_wait_bounded(msfm_ctx* ctx, hipStream_t s, const char* what);
// Single-process multi-GPU (multi.hip): the communicator of this context was aborted (ncclCommAbort frees it) - forget it.
void msfm_ctx_forget_rccl(msfm_ctx* ctx);
hipError_t msfm_pool_alloc(void** p, size_t bytes, size_t* capacity);
void msfm_pool_free(void* p, size_t capacity);
void msfm_pool_trim(int device);

// Simple owning device buffer.
template <typename T>
struct DevBuf {
  T* p = nullptr;
  size_t n = 0;
  size_t cap = 0;  // bytes of the underlying block
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  ~DevBuf() { release(); }
  void swap(DevBuf& o) {  // exchanges the blocks (same element count expected by the callers), capacities included
    std::swap(p, o.p); std::swap(n, o.n); std::swap(cap, o.cap);
  }
  void release() {
    if (p) msfm_pool_free(p, cap);
    p = nullptr;
    n = 0;
    cap = 0;
  }
  hipError_t alloc(size_t count) {
    release();
    n = count;
    if (count == 0) return hipSuccess;
    void* q = nullptr;
    const hipError_t e = msfm_pool_alloc(&q, count * sizeof(T), &cap);
    p = static_cast<T*>(q);
    if (e != hipSuccess) { p = nullptr; n = 0; cap = 0; }
    return e;
  }
  hipError_t upload(const T* h, size_t count, hipStream_t s) {
    if (count == 0) return hipSuccess;
    return hipMemcpyAsync(p, h, count * sizeof(T), hipMemcpyHostToDevice, s);
  }
  hipError_t from(const std::vector<T>& v, hipStream_t s) {
    hipError_t e = alloc(v.size());
    if (e != hipSuccess) return e;
    return upload(v.data(), v.size(), s);
  }
};

// Pinned staging of what one call of a resident object uploads (msfm_sgm, msfm_rectifier): two slots in turn, each with the event
// behind its copy, so the caller's buffers are free on return and the call does not wait for its own copy.  The slot of the call
// before last is taken again: its copy has long run unless the caller is two calls ahead of the device.
struct StageSlots {
  uint8_t* buf[2] = {nullptr, nullptr};
  hipEvent_t staged[2] = {nullptr, nullptr};
  bool in_flight[2] = {false, false};
  int slot = 0;
  StageSlots() = default;
  StageSlots(const StageSlots&) = delete;
  StageSlots& operator=(const StageSlots&) = delete;
  ~StageSlots() {
    for (int i = 0; i < 2; i++) {
      if (buf[i]) (void)hipHostFree(buf[i]);
      if (staged[i]) (void)hipEventDestroy(staged[i]);
    }
  }
  hipError_t create(size_t bytes) {
    for (int i = 0; i < 2; i++) {
      hipError_t e = hipHostMalloc((void**)&buf[i], bytes);
      if (e != hipSuccess) { buf[i] = nullptr; return e; }
      if ((e = hipEventCreateWithFlags(&staged[i], hipEventDisableTiming)) != hipSuccess) return e;
    }
    return hipSuccess;
  }
  // -> *out: the slot to fill; *waits is counted up if its earlier copy had to be waited for
  hipError_t take(uint8_t** out, int64_t* waits) {
    if (in_flight[slot] && hipEventQuery(staged[slot]) != hipSuccess) {
      (void)hipGetLastError();
      const hipError_t e = hipEventSynchronize(staged[slot]);
      if (e != hipSuccess) return e;
      (*waits)++;
    }
    *out = buf[slot];
    return hipSuccess;
  }
  // bytes of the taken slot to dst on s, the event behind the copy, and the turn to the other slot
  hipError_t send(void* dst, size_t bytes, hipStream_t s) {
    hipError_t e = hipMemcpyAsync(dst, buf[slot], bytes, hipMemcpyHostToDevice, s);
    if (e != hipSuccess) return e;
    if ((e = hipEventRecord(staged[slot], s)) != hipSuccess) return e;
    in_flight[slot] = true;
    slot ^= 1;
    return hipSuccess;
  }
};

// rectify.hip, for msfm_sgm_execute_rectified: the rectified pair [2][h][w] of a rectifier on the device (nullptr before its
// first rectify), its context and its size
struct msfm_rectifier;
const uint8_t* rectifier_planes(const msfm_rectifier* rect, msfm_ctx** ctx, int* width, int* height);

// The device scratch of one call: what a function enqueues on ctx->stream while it owns local blocks happens inside a DevScope.
// Its destructor waits for the stream unless the scope has been settled, so a return at any point - HIP_TRY, MSFM_TRY - gives no
// block back to the cache that the stream still uses (the cache hands a freed block to the next context at once).
// A destructor runs before those of the objects declared earlier: declare the scope AFTER every DevBuf, and every scratch struct
// that holds DevBufs, of the function.  (DevBuf's constructor does nothing: a block that is allocated late is declared early.)
// Blocks that move into a result object by swap after finish() are not the scope's business any more.
struct DevScope {
  hipStream_t s;
  int64_t h2d = 0;        // bytes the up() calls have moved
  bool settled = false;
  explicit DevScope(msfm_ctx* ctx) : s(ctx->stream) {}
  DevScope(const DevScope&) = delete;
  DevScope& operator=(const DevScope&) = delete;
  ~DevScope() { if (!settled) (void)hipStreamSynchronize(s); }
  // a block of max(1, count, capacity) elements, and count elements of h into it
  template <typename T, typename U>
  hipError_t up(DevBuf<T>& buf, const U* h, size_t count, size_t capacity = 0) {
    const hipError_t e = buf.alloc(std::max<size_t>(1, std::max(count, capacity)));
    if (e != hipSuccess) return e;
    h2d += (int64_t)(count * sizeof(U));
    return buf.upload(h, count, s);
  }
  template <typename T, typename U>
  hipError_t up(DevBuf<T>& buf, const std::vector<U>& v) { return up(buf, v.data(), v.size()); }
  template <typename T>
  hipError_t down(T* h, const T* d, size_t count) {   // (a null h: the caller does not want the array)
    if (!h || !count) return hipSuccess;
    return hipMemcpyAsync(h, d, count * sizeof(T), hipMemcpyDeviceToHost, s);
  }
  hipError_t finish() { settled = true; return hipStreamSynchronize(s); }   // the call's last wait; its error is the caller's to report
  // only directly behind a wait the code can point to (a callee's finish(), msfm_ba_download_params), or where every block
  // has gone to a result object that the caller gets
  void dismiss() { settled = true; }
};

// The temporary block of every rocPRIM call that one function enqueues.  A call that needs more than the block holds gets a
// larger one, and the smaller one is retired: kept until the PrimTmp is destroyed, because the calls enqueued before may still
// run in it.  Nothing goes back to the cache between construction and destruction.  The rule is DevBuf's: declare the PrimTmp
// BEFORE the function's DevScope, so that it is destroyed behind the scope's wait.
struct PrimTmp {
  DevBuf<char> cur;
  std::list<DevBuf<char>> retired;   // (a DevBuf neither copies nor moves: a default-made node, then swap)
  hipError_t fit(size_t bytes) {
    if (cur.p && cur.cap >= bytes) return hipSuccess;
    if (cur.p) {
      retired.emplace_back();
      retired.back().swap(cur);
    }
    return cur.alloc(std::max<size_t>(1, bytes));
  }
};

static inline int bits_for(unsigned v) {   // bits that hold every value 0 .. v
  int b = 1;
  while (b < 32 && (v >> b)) b++;
  return b;
}

static inline int cdiv(long a, long b) { return (int)((a + b - 1) / b); }

// splitmix64: the counter-based samplers of geo.hip and pose.hip draw from it, each with its own salts and key mixing
__host__ __device__ static inline uint64_t sm64(uint64_t& s) {
  s += 0x9E3779B97F4A7C15ull;
  uint64_t z = s;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

// The sum of an int over the 64 lanes of a wave (butterfly 32 .. 1), in every lane.
__device__ static inline int wave_sum_int(int c) {
  for (int d = 32; d > 0; d >>= 1) c += __shfl_xor(c, d);
  return c;
}

// the ordered position of a set flag among the flags of a workgroup of 64 * WAVES lanes, and their count; part [WAVES] in LDS.
// Two barriers; every lane of the workgroup calls it.  Safe to call again with the same `part` at once.
template <int WAVES>
__device__ static inline int wg_rank(bool flag, int* part, int& total) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const unsigned long long bal = __ballot(flag);
  if (lane == 0) part[wv] = __popcll(bal);
  __syncthreads();
  int before = __popcll(bal & ((1ull << lane) - 1)), sum = 0;
#pragma unroll
  for (int w = 0; w < WAVES; w++) {
    const int c = part[w];
    if (w < wv) before += c;
    sum += c;
  }
  __syncthreads();
  total = sum;
  return before;
}

// the segment of position x in CSR offsets: off[lo] <= x < off[lo + 1] (empty segments are stepped over)
__device__ static inline int csr_segment_of(const int* __restrict__ off, int n, int x) {
  int lo = 0, hi = n;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (off[mid] <= x) lo = mid; else hi = mid;
  }
  return lo;
}

// The CSR offsets of a batch call (n + 1 entries, n > 0); `who` prefixes the message.
static inline int msfm_check_offsets(msfm_ctx* ctx, const char* who, int n, const int* offsets) {
  if (offsets[0] != 0) return msfm_set_error(ctx, MSFM_E_INVAL, "%s: offsets[0] must be 0", who);
  for (int p = 0; p < n; p++)
    if (offsets[p + 1] < offsets[p]) return msfm_set_error(ctx, MSFM_E_INVAL, "%s: offsets must be non-decreasing", who);
  return MSFM_OK;
}

// Host-side helper: the index structures of a 10^6-observation problem (msfm_ba_create) and the per-pair iteration tables
// of the RANSAC (geo.hip) are built by a few threads (MSFM_HOST_THREADS, default min(hardware threads, 8));
// fn(t, begin, end) gets one contiguous range per thread.
static inline int host_threads() { return msfm_env_process().host_threads; }
template <class F>
static inline void par_ranges(size_t n, int nt, F&& fn, size_t grain = 4096) {   // at least `grain` items per thread
  nt = (int)std::max<size_t>(1, std::min<size_t>(nt, n / grain + 1));
  if (nt == 1) { fn(0, (size_t)0, n); return; }
  std::vector<std::thread> th;
  th.reserve(nt - 1);
  for (int t = 1; t < nt; t++) th.emplace_back([&fn, t, n, nt] { fn(t, n * t / nt, n * (t + 1) / nt); });
  fn(0, (size_t)0, n / nt);
  for (auto& x : th) x.join();
}

// ---- device-array cores shared with chain.hip (the resident chain from match codes to a bundle adjustment) ----
struct msfm_fransac_options;
int geo_fransac_dev(msfm_ctx* ctx, int n_pairs, const int* h_offsets, const int* d_off, const float* d1, const float* d2,
                    const msfm_fransac_options* opt, double* dF, uint8_t* d_in, int* d_nin, uint8_t* d_ok);
struct msfm_hransac_options;
// active (host, may be NULL): pairs with active[p] == 0 are skipped (no model); the sampler index of pair p stays p
int geo_hransac_dev(msfm_ctx* ctx, int n_pairs, const int* h_offsets, const int* d_off, const float* d1, const float* d2,
                    const msfm_hransac_options* opt, const uint8_t* active, double* dH, uint8_t* d_in, int* d_nin, uint8_t* d_ok);
int geo_hransac_check(msfm_ctx* ctx, int n_pairs, const int* h_offsets, const msfm_hransac_options* opt);
int geo_epipolar_batch_dev(msfm_ctx* ctx, int total, const int* d_pair_of, const float* d1, const float* d2, const double* dF,
                           const uint8_t* d_ok, double th, uint8_t* d_in);
struct msfm_track_dev {   // CSR tracks on the device: observations of a track in ascending image order
  DevBuf<int> off, img, feat;
  int n_tracks = 0, n_obs = 0;
};
// What chain.hip needs of a match result and its descriptor set (both defined in knn.hip)
struct msfm_match_result;
struct MatchView {
  msfm_ctx* ctx;
  int n_images, n_pairs;
  long total_q;
  const int* pairs;              // host [n_pairs][2]
  const int* out_off;            // host [n_pairs]: first code of the pair
  const int* nq;                 // host [n_pairs]: query features of the pair
  const int32_t* code;           // device [total_q]
  const int* n_all; const int* n_good;   // device [n_pairs]
  std::vector<int> count;        // features per image
  std::vector<const float*> kp;  // device [count][2] per image, nullptr: no keypoints uploaded
  bool slam;
};
int match_result_view(msfm_match_result* R, MatchView* out);   // MSFM_E_INVAL when the result is stale or orphaned
// What localize.hip needs of a verified chain (chain.hip) to make a match store of its own
struct ChainMatchView {
  msfm_ctx* ctx;
  int n_images, n_pairs;
  const int* pairs;              // host [n_pairs][2]
  const int* count;              // host [n_images]: features per image
  const int* match_off;          // host [n_pairs + 1]
  const int* d_match;            // device [match_off[n_pairs]][2]
  const float* d_kp;             // device [sum of count][2], images in order
  std::vector<const float*> kp;  // per image, nullptr: no keypoints
};
int chain_match_view(msfm_chain* C, ChainMatchView* out);   // MSFM_E_INVAL before msfm_chain_verify

// A resident copy of the verified matches (localize.hip creates and destroys it; seed.hip reads it too)
struct msfm_match_store {
  msfm_ctx* ctx = nullptr;
  int n_images = 0, n_pairs = 0, M = 0;
  std::vector<int> n_features, feat_off, pair_img, match_off;
  std::vector<int> row_off;       // [n_images + 1]: the pairs with idx1 = i are row_off[i] .. row_off[i + 1]  ("QueryMatch(i, j)" = row i, entry j)
  std::vector<uint8_t> has_kp;    // per image: d_kp holds its keypoints (a store made from a chain)
  DevBuf<int> d_match;            // [M][2]
  DevBuf<float> d_kp;             // [feat_off[n_images]][2]
};

// What msfm_seed_hypotheses leaves behind (seed.hip creates and destroys it; recon.hip starts a model from its winner).  The
// answer of every hypothesis is host memory; the winner's accepted points stay on the device as well, in blocks sized by the
// longest hypothesis of the call (the winner is not known on the host when they are made), with its place in the store.
struct msfm_seed_set {
  msfm_ctx* ctx = nullptr;
  const msfm_match_store* store = nullptr;
  int n = 0, winner = -1;
  std::vector<uint8_t> arm, pose_ok, pass;
  std::vector<int> n_matches, pt_off, pt_match;
  std::vector<double> f, R, t, c, X, mse;
  int64_t h2d_bytes = 0;
  // the winner (winner >= 0 only)
  int win_img[2] = {-1, -1};      // id_img1, id_img2
  int win_m0 = 0;                 // its first match in the store
  int win_kp[2] = {0, 0};         // the first keypoint row of either image in an array of every image's rows (feat_off)
  DevBuf<int> d_ptm;              // [n_points of the winner] pt_match
  DevBuf<double> d_X, d_mse;      // [..][3], [..]
};
static inline bool child_holds_blocks(const msfm_seed_set* R) { return R->d_ptm.p != nullptr; }

// What msfm_localize_candidates leaves behind (localize.hip creates and destroys it; localize_pose.hip reads it).  A set made
// with point_xyz keeps the device arrays its gather kernel wrote - corr_point, pts_w, pts_2d in the layout of corr_off - until
// msfm_localize_set_destroy, so msfm_localize_poses moves no correspondence over PCIe.
struct msfm_localize_set {
  msfm_ctx* ctx = nullptr;
  std::vector<int> rank, corr_off, corr_feat, corr_point, vis_off, vis_cam;
  std::vector<double> pts_w, pts_2d;
  bool have_pts = false;
  int64_t h2d_bytes = 0;
  DevBuf<int> d_cp;               // [n_corr]           (have_pts and n_corr > 0 only)
  DevBuf<int> d_cf;               // [n_corr] corr_feat (sets of localize_candidates_dev with resident arrays only)
  DevBuf<double> d_pw, d_p2;      // [n_corr][3], [n_corr][2]
};
static inline bool child_holds_blocks(const msfm_localize_set* R) { return R->d_cp.p != nullptr; }

struct LocalizeDev {   // the bulk arrays of the state on the device (recon.hip's); kp: every image's rows, or NULL = the store's
  const int* feat_point; const uint8_t* pt_bad; const double* pt_mse; const int* pt_views; const double* point_xyz; const float* kp;
};
struct msfm_localize_problem;
int localize_candidates_dev(msfm_ctx* ctx, const char* who, const msfm_match_store* S, const msfm_localize_problem* P, const LocalizeDev* dev,
                            msfm_localize_set** out);
struct msfm_localize_pose_set {   // host memory only
  int n = 0, n_corr = 0, n_tried = 0, winner = -1, next_row = -1;
  std::vector<uint8_t> tried, arm, pass, state;
  std::vector<double> f, R, t, avg, errors;
  std::vector<int> best_step, best_iter, n_in, n_out;
};
struct msfm_localize_pose_options;
int localize_poses_dev(msfm_ctx* ctx, const char* who, const msfm_localize_set* L, const double* row_f, const double* row_f_init, int n_points,
                       const uint8_t* pt_new_added, const uint8_t* d_added_dev, const msfm_localize_pose_options* opt_in, msfm_localize_pose_set** out,
                       DevBuf<uint8_t>* keep_state, int64_t* h2d_bytes);

// The device halves of the four pose initialisers (pose.hip): msfm_epnp_ransac_batch, msfm_epnpf_sweep_batch,
// msfm_relpose_5pt_batch, msfm_relpose_8pt_batch.  An export is its checks, sc.up of the inputs, the result's alloc, the _dev
// call and sc.down of the outputs; localize_pose.hip and seed.hip call the same _dev functions on the buffers their gather
// kernels wrote.  A _dev function sizes the result's candidate scratch from the sample count and enqueues the launches; it
// does not synchronise, so the result (outputs and scratch) lives until its caller has: declare it before the DevScope.
struct PoseView {         // the problems of one call, device pointers
  int n;                  // problems (images / pairs)
  const int* off;         // [n + 1]
  const double *a, *b;    // [off[n]] rows: absolute pose: world points [3] and image points [2]; relative pose: ref and cur [2]
  const double *f1, *f2;  // [n] or null: EPnP f / sweep f_init in f1; five-point f_ref, f_cur; eight-point none
};
static inline hipError_t hip_first_error(std::initializer_list<hipError_t> es) {   // (a braced list is evaluated left to right)
  for (const hipError_t e : es) if (e != hipSuccess) return e;
  return hipSuccess;
}
struct EpnpResult {
  DevBuf<double> R, t, avg, err; DevBuf<int> best_iter;   // [n] records; err [total]
  DevBuf<double> hyp;                                      // scratch
  hipError_t alloc(size_t n, size_t total) {
    return hip_first_error({R.alloc(9 * n), t.alloc(3 * n), avg.alloc(n), err.alloc(std::max<size_t>(1, total)), best_iter.alloc(n)});
  }
};
struct EpnpfResult {
  DevBuf<double> f, R, t, avg, err; DevBuf<int> best_step, best_iter;
  DevBuf<double> step_err, step_pose; DevBuf<int> step_it;   // scratch; step_err [n][n_steps] is the public step_error
  hipError_t alloc(size_t n, size_t total) {
    return hip_first_error({f.alloc(n), R.alloc(9 * n), t.alloc(3 * n), avg.alloc(n), err.alloc(std::max<size_t>(1, total)), best_step.alloc(n),
                            best_iter.alloc(n)});
  }
};
struct Relpose5Result {
  DevBuf<double> E, R, t; DevBuf<uint8_t> ok; DevBuf<int> n_cand;   // [n] records
  DevBuf<double> cE, ce; DevBuf<int> cn;                            // scratch
  hipError_t alloc(size_t n, size_t /*total*/) { return hip_first_error({E.alloc(9 * n), R.alloc(9 * n), t.alloc(3 * n), ok.alloc(n), n_cand.alloc(n)}); }
};
struct Relpose8Result {
  DevBuf<double> F, f_ref, f_cur, E, R, t, best_error; DevBuf<uint8_t> ok; DevBuf<int> best_iter, n_cand;
  DevBuf<double> cF, ce; DevBuf<uint8_t> cok;                       // scratch
  hipError_t alloc(size_t n, size_t /*total*/) {
    return hip_first_error({F.alloc(9 * n), f_ref.alloc(n), f_cur.alloc(n), E.alloc(9 * n), R.alloc(9 * n), t.alloc(3 * n), best_error.alloc(n),
                            ok.alloc(n), best_iter.alloc(n), n_cand.alloc(n)});
  }
};
struct msfm_epnpf_options;
int pose_epnp_dev(msfm_ctx* ctx, const PoseView& V, int max_iter, uint64_t seed, EpnpResult& out);
int pose_epnpf_dev(msfm_ctx* ctx, const PoseView& V, int n_steps, const msfm_epnpf_options* opt, EpnpfResult& out);
int pose_relpose5_dev(msfm_ctx* ctx, const PoseView& V, int ransac_times, uint64_t seed, Relpose5Result& out);
int pose_relpose8_dev(msfm_ctx* ctx, const PoseView& V, int ransac_times, uint64_t seed, Relpose8Result& out);

struct TrackPtrs {   // tri.hip: CSR tracks + cameras as the reference keeps them, device pointers
  int n_tracks;
  const int *off, *cam;
  const double *xy, *R, *t, *c, *fk;
};
int tri_midpoint_dev(msfm_ctx* ctx, const TrackPtrs& T, double th_error, double th_angle, double* dX, double* dmse, uint8_t* dok);
// ---- registering the SLAM model on its GPS track (gpsreg.hip): device-array cores, no synchronisation ----
struct AccuracyPtrs {   // GetAccuracy on CSR tracks; dc [n_cams][2] or nullptr = 0; the last four are written
  int n_tracks;
  const int *off, *cam;
  const double *xy, *R, *t, *fk, *dc, *X;
  const uint8_t* ok_in;
  int min_views;
  double th_outlier;
  double *e_avg, *e_mse;
  int* n_used;
  uint8_t* ok_out;   // may be ok_in: a track's flag is read and written by one thread
};
struct RegisterPtrs {   // the point loop of GPSRegistration2; cam_offset [n_cams][3] = gps - cam_c; X in / out
  int n_tracks;
  const int *off, *cam;
  const uint8_t* ok;
  const double *cam_c, *cam_offset;
  double* X;
};
int gps_accuracy_dev(msfm_ctx* ctx, const AccuracyPtrs& P, int n_rows, int* d_n_outliers);
int gps_register_dev(msfm_ctx* ctx, const RegisterPtrs& P);
int gps_store_points_dev(msfm_ctx* ctx, int n_points, const int* d_track_of_point, const double* d_point, double* dX);
std::vector<double> gps_cam_offsets(int n_cams, const double* cam_c, const double* gps);

struct msfm_ba_problem;
struct msfm_ba;
// msfm_ba_create with the bulk arrays of the problem (obs_cam, obs_pt, obs_xy, point, pt_weight, pt_mutable) in DEVICE memory
int ba_create_impl(msfm_ctx* ctx, const msfm_ba_problem* P, bool bulk_on_device, msfm_ba** out);
const double* ba_device_points(const msfm_ba* ba);   // the resident points [n_points][3] of a problem (adjust.hip scatters them on the device)

// ---- adjusting a round (adjust.hip): msfm_round_adjust is its checks + upload + round_adjust_dev + download; recon.hip calls
// the same core on the arrays it keeps resident ----
struct msfm_round_set {
  msfm_ctx* ctx = nullptr;
  int n_cams = 0, n_models = 0, n_points = 0;   // (n_points = 0 and empty point arrays: a set of msfm_recon_adjust, whose points stay on the device)
  std::vector<double> cam_pose, cam_model, cam_R, cam_t, cam_c, cam_fk, point_xyz, pt_mse;
  std::vector<uint8_t> pt_mutable, pt_bad, pt_new_added;
  std::vector<int> pt_views;
  int counts[3] = {0, 0, 0};        // count_outliers, count_new_add, count_outliers_new_add
  int adjust[2][2] = {{0, 0}, {0, 0}};   // "adjust cams", "adjust pts" of each solve
  int solved[2] = {0, 0};
  msfm_ba_summary summary[2];
  std::vector<msfm_ba_iteration> rows[2];
  bool keep_problem = false;
  struct Problem {
    int n_points = 0, n_obs = 0;
    std::vector<int> kept, obs_cam, obs_pt;
    std::vector<double> obs_xy, pt_weight;
    std::vector<uint8_t> cam_mutable, pt_mutable;
  } problem[2];
  int64_t h2d_bytes = 0;
};
static inline bool child_holds_blocks(const msfm_round_set*) { return false; }   // its destroy runs between the rounds of a model: no wait
struct RoundArgs {     // counts and the O(cameras) arguments, host pointers
  int n_cams = 0, n_models = 0, n_points = 0, n_obs = 0;
  const int* cam_img = nullptr; const int* cam_model_of_cam = nullptr; const uint8_t* model_mutable = nullptr;
  const int *h_obs_point = nullptr, *h_obs_cam = nullptr, *h_obs_feat = nullptr;   // the rows on the host, where the caller has them (a refusal's text)
  int new_cam = -1, n_visible = 0;
  const int* visible = nullptr;
  bool do_partial = false, do_full = false, do_outliers = false;
};
struct RoundTables {   // what round_tables makes of them
  std::vector<int> cam_fo, rank, cam_of_rank, kp_base;   // kp_base[c]: the first keypoint row of camera c in RoundDev::kp
  std::vector<uint8_t> cam_free, cam_all;
  int max_feat = 1, bf = 1;
  long kp_rows = 0;        // packed_kp: rows of a keypoint array that holds the cameras' images only, in camera order
  bool all_kp = true;      // !packed_kp: the store has the keypoints of every camera's image
};
struct RoundDev {      // the bulk arrays, device pointers; the point arrays and flags are written in place
  const int *feat_point = nullptr, *obs_point = nullptr, *obs_cam = nullptr, *obs_feat = nullptr;
  double *point_xyz = nullptr, *pt_mse = nullptr;
  uint8_t *pt_bad = nullptr, *pt_mutable = nullptr, *pt_new_added = nullptr;
  const float* kp = nullptr;
};
// packed_kp: kp_base counts rows of a packed upload; otherwise it is the store's feat_off (a resident array of every image's rows)
int round_tables(msfm_ctx* ctx, const char* who, const msfm_match_store* S, const RoundArgs& A, bool packed_kp, const msfm_round_options& opt,
                 RoundTables* T);
// the two refusals of the device-side index check, worded once: x = the first bad feat_point entry / row = the first bad row
int round_fp_error(msfm_ctx* ctx, const char* who, const std::vector<int>& cam_fo, int n_cams, int n_points, int x);
int round_row_error(msfm_ctx* ctx, const char* who, int row, int point, int cam, int feat);
int round_key_check(msfm_ctx* ctx, const char* who, int n_cams, const RoundTables& T);
int round_adjust_dev(msfm_ctx* ctx, const char* who, const RoundArgs& A, const RoundTables& T, const RoundDev& D, const msfm_round_options& opt,
                     int64_t* h2d_bytes, msfm_round_set* R, bool fetch_points);

// ---- a new camera's points (newpoints.hip): msfm_new_points is newpoints_plan + a packed upload of the involved cameras' rows +
// newpoints_dev + download; recon.hip runs plan and kernels on its resident feat_point and keypoints and appends on the device ----
struct msfm_new_points_set {
  int n_new = 0, n_entries = 0;
  std::vector<int> pt_off, cam2, feat1, feat2, vis_entry, pt_match, n_matches, n_candidates, n_accepted;
  std::vector<double> X, mse;
  std::vector<uint8_t> takes1, takes2, large;
  int64_t h2d_bytes = 0;
};
struct NewPointsEnt {   // one visible entry of one new camera
  int m0;             // first match of the pair in the store
  int fp1, fp2;       // first feat_point row of camera 1 / 2 in the feat_point array the kernels get
  int kp1, kp2;       // first keypoint row of image 1 / 2
  int cam1, cam2;     // rows of the uploaded camera table
  int slot1, slot2;   // first claim slot of camera 1 / 2 in this new camera's slot table
  int k;              // the new camera
  int large;          // th_angle_large applies (:781)
};
struct NewPointsArgs {   // host pointers: the cameras and the lists
  int n_cams = 0;
  const int* cam_img = nullptr;
  const double *cam_R = nullptr, *cam_t = nullptr, *cam_c = nullptr, *cam_fk = nullptr;
  int n_new = 0;
  const int *new_cam = nullptr, *vis_off = nullptr, *vis_cam = nullptr;
};
#define NP_KP_STORE 0    // the store's keypoints (made from a chain): a camera's rows start at feat_off of its image
#define NP_KP_PACKED 1   // a packed upload of the involved cameras' rows
#define NP_KP_ALL 2      // an array of every image's rows in the store's order (a resident state's)
struct NewPointsPlan {
  int nn = 0, E = 0, M = 0;   // new cameras, visible entries, matches of the walk
  long fp_rows = 0, kp_rows = 0, n_slots = 0;
  std::vector<NewPointsEnt> ent;
  std::vector<int> cam_fo, off_all, blk_off, cam_off, involved, fp_base, kp_base;
};
struct NewPointsDev {   // what newpoints_dev allocates; d_out is the result block, the o_* its layout (newpoints.hip)
  DevBuf<NewPointsEnt> d_ent;
  DevBuf<int> d_offa, d_blk, d_val, d_val_s, d_slot;
  DevBuf<double> d_cam, d_Xall, d_mseall;
  DevBuf<unsigned long long> d_key, d_key_s;
  PrimTmp tmp;          // of the sort: the owner of a NewPointsDev declares it before its DevScope
  DevBuf<char> d_out;
  size_t o_mse = 0, o_w = 0, o_f1 = 0, o_f2 = 0, o_nc = 0, o_na = 0, o_t1 = 0, o_t2 = 0, out_bytes = 0;
};
struct msfm_new_points_options;
int newpoints_plan(msfm_ctx* ctx, const char* who, const msfm_match_store* S, const NewPointsArgs& P, const msfm_new_points_options& opt,
                   bool fp_resident, int kp_mode, NewPointsPlan* L, msfm_new_points_set* R);
int newpoints_dev(msfm_ctx* ctx, const msfm_match_store* S, const NewPointsArgs& P, const NewPointsPlan& L, const msfm_new_points_options& opt,
                  const int* d_fp, const float* d_kp, DevScope& sc, NewPointsDev* W);
void newpoints_collect(const NewPointsArgs& P, const NewPointsPlan& L, const NewPointsDev& W, const char* hb, msfm_new_points_set* R);
int tracks_build_dev(msfm_ctx* ctx, int n_images, const std::vector<int>& feat_off, const int* d_nf, const int* d_fo, int n_pairs,
                     const int* d_pair, const int* d_moff, const int* d_match, int M, msfm_track_dev* out);

// ---- the visual words (words.hip): msfm_descset_words reads the set's resident rows, msfm_wordset_create_from_words hands word
// ids and keypoints to pairsel.hip's core without leaving the device ----
struct msfm_descset;
struct DescView {   // what words.hip needs of a descriptor set (defined in knn.hip)
  msfm_ctx* ctx;
  int n_images;
  unsigned long generation;
  std::vector<int> count;          // features per image
  std::vector<const float*> f32;   // device [count][128] per image, nullptr: nothing uploaded
  std::vector<const float*> kp;    // device [count][2] per image, nullptr: no keypoints
};
void descset_view(const msfm_descset* s, DescView* out);
// msfm_descset_upload is its checks + this core with a fill that copies from the host; msfm_descset_describe (sift.hip) fills the
// same blocks by kernel.  fill(rows, kp, stream) enqueues what writes rows [count][128] and, with_kp, kp [count][2].
typedef std::function<hipError_t(float*, float*, hipStream_t)> DescFill;
int descset_put_dev(msfm_descset* s, int image, int count, bool with_kp, const char* prep_stat, const DescFill& fill);
struct voctrain_stats {   // what msfm_voctree_train_stats reports (include/msfm.h)
  int64_t n_features = 0, n_leaves = 0;
  int n_images = 0, n_blocks = 0, depth = 0, weight_shift = 0, sum_shift = 0, host_waits = 0;
  int level_nodes[32] = {}, level_split[32] = {}, level_max_iters[32] = {}, level_capped[32] = {};
};
struct msfm_voctree {   // words.hip uploads one, voctrain.hip trains one; both leave it in the layout k_descend reads
  msfm_ctx* ctx = nullptr;
  int k = 0, n_blocks = 0, depth = 0;
  int64_t n_leaves = 0, h2d_bytes = 0;
  bool trained = false;        // made by msfm_descset_voctree_train: `train` holds its statistics
  voctrain_stats train;
  DevBuf<uint16_t> d_n;        // [n_blocks]
  DevBuf<float> d_desc;        // [n_blocks][k][8][16]
  DevBuf<uint32_t> d_link;     // [n_blocks][k]
  DevBuf<float> d_weight;      // [n_blocks][k]
};
// msfm_wordset_create is its checks + the upload of the four arrays + this core.  feat_off [n + 1] on the host and on the device;
// d_feat_off and d_kp move into the set, d_hw [n] and d_word [feat_off[n]] are read only and may be freed on return (the core
// waits for the stream before it returns, also when it fails).  h2d_bytes: what the caller sent, kept for msfm_wordset_size.
int wordset_create_dev(msfm_ctx* ctx, int n, int K, int num_words, const std::vector<int>& feat_off, DevBuf<int>& d_feat_off, const uint8_t* d_hw,
                       const int* d_word, DevBuf<float>& d_kp, int64_t h2d_bytes, msfm_wordset** out);

// bits of the device-side failure word of a solve: 1 = reduced system not positive definite, 2 = a 3x3 point block, 4 = non-finite step;
// MSFM_FAIL_SYNC = a bounded in-kernel wait ran out (the host turns it into MSFM_E_DEVICE)
#define MSFM_FAIL_SYNC (1 << 20)
// msfm_chol_plan (chol_plan.h): the elimination structure of the reduced system
struct msfm_chol_ws;   // hand-off state of the persistent panel chain (chol.hip): flags, hand-off buffers, ticket counters
int msfm_chol_ws_create(msfm_ctx* ctx, int npad, msfm_chol_ws** out);
void msfm_chol_ws_destroy(msfm_chol_ws* ws);
// env: the problem's copy of the switches (MSFM_CHOL_LAUNCHES, MSFM_CHAIN_FORCE, MSFM_CHAIN_TRACE); paths: the
// MSFM_PATH_* bits of msfm_ba_layout.solve_paths for the launches this call enqueued
// riders: work of the caller's that the call's launches take along (solve_riders.h), either of them optional.
//   modelsum  run by extra workgroups of the level-0 corner update, in front of that level's merge; the caller gives it only
//             with a plan of at least one level, and a call that returns MSFM_OK has launched it.
//   epilogue  run by k_backsolve_chain behind the publication of every block; `epilogue_ran` says whether the back
//             substitution took that form - if not, the caller does the work itself.
struct ModelSumArgs;
struct SolveEpilogue;
struct msfm_chol_riders {
  const ModelSumArgs* modelsum = nullptr;
  const SolveEpilogue* epilogue = nullptr;
  bool epilogue_ran = false;
};
int msfm_chol_factor_solve(msfm_ctx* ctx, const msfm_env& env, double* M, int npad, int n, double* work, double* w, double* z, int* fail,
                           const msfm_chol_plan* plan, double* z_next, msfm_chol_ws* ws, int* paths, msfm_chol_riders* riders);
int msfm_chol_fill_pending(msfm_ctx* ctx, double* z, int npad);   // "not solved yet" marks of k_backsolve_chain
