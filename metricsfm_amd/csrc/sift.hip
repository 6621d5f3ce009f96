// Describing given SIFT frames: the given-frames arm of
//   Database::ExtractImageFeatures                     SfM/src/database.cc:289-349
//   VLSiftExtractor::initialize (the stretch)          SfM/src/feature/feature_extractor_vl_sift.h:41-71
//   VLSiftExtractor::run_sift, nikeys >= 0             SfM/src/feature/feature_extractor_vl_sift.cpp:75-216
// from uint8 pixels to rows that lie in a descriptor set.  include/msfm.h states the definitions (they are this project's: VLFeat's
// sources are not in the reference tree); every kernel below follows them operation for operation, and nothing here is contracted
// into an FMA (the pragma below holds for the whole file, as words_dist.h does per function).
//
// msfm_scalespace_create    k_minmax (integer reduction) and one wait for the range, then per octave: k_stretch (octave 0) or
//                           k_decimate, and per level k_blur_rows + k_blur_cols - one thread per output pixel, the source tile
//                           with its halo in LDS, the taps added in ascending order - and k_gradient on the levels 0 .. S - 1.
//                           One block per octave holds its S + 3 levels and 2 S gradient planes.
// msfm_descset_describe     k_describe: one workgroup of 128 lanes per frame, lane = histogram bin.  The window's pixels are
//                           taken 128 at a time in raster order; every lane makes one pixel's record (win * mod, the three bin
//                           indices, the three remainders), the records that can touch a bin are packed in order into LDS (a
//                           ballot per wave), and every lane walks them in order and adds what touches its bin: each bin is
//                           the sum of its contributions in raster order.  The two norms are ordered sums by lane 0.  The rows
//                           go into the set through descset_put_dev (knn.hip), the core msfm_descset_upload shares.
#include <memory>

#include "common.h"
#include "sift_args.h"

#pragma clang fp contract(off)

struct msfm_scalespace {
  msfm_ctx* ctx = nullptr;
  int w = 0, h = 0, O = 0, S = 0;
  int ow[SIFT_MAX_OCTAVES] = {}, oh[SIFT_MAX_OCTAVES] = {};
  int64_t h2d_bytes = 0;
  DevBuf<float> oct[SIFT_MAX_OCTAVES];   // [S + 3 levels, then S x (modulus, angle)][oh][ow]
  DevBuf<float> table;                   // T[257]
  size_t npx(int o) const { return (size_t)ow[o] * oh[o]; }
  const float* level(int o, int s) const { return oct[o].p + (size_t)(s + 1) * npx(o); }
  const float* grad(int o, int s, int which) const { return oct[o].p + (size_t)(S + 3 + 2 * s + which) * npx(o); }
};

namespace sift {

#define SIFT_EPS 1.19209290e-07f
#define SIFT_PI2 6.28318548f

struct Levels {   // what k_describe needs of a scale space
  const float* base[SIFT_MAX_OCTAVES];
  int w[SIFT_MAX_OCTAVES], h[SIFT_MAX_OCTAVES];
  int S;
};

// mm[0] = min, mm[1] = max over the width x height pixels: a workgroup walks the rows blockIdx.x, blockIdx.x + gridDim.x, ...,
// and every wave ends with one pair of integer atomics (a pair per wave and row took 4 ms on twelve megapixels)
__global__ __launch_bounds__(256) void k_minmax(const uint8_t* __restrict__ img, int w, int h, int stride, unsigned* __restrict__ mm) {
  unsigned lo = 255u, hi = 0u;
  for (int y = blockIdx.x; y < h; y += gridDim.x)
    for (int x = threadIdx.x; x < w; x += 256) {
      const unsigned v = img[(size_t)y * stride + x];
      lo = min(lo, v); hi = max(hi, v);
    }
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) { lo = min(lo, (unsigned)__shfl_xor((int)lo, d)); hi = max(hi, (unsigned)__shfl_xor((int)hi, d)); }
  if ((threadIdx.x & 63) == 0) { atomicMin(&mm[0], lo); atomicMax(&mm[1], hi); }
}

__global__ __launch_bounds__(256) void k_stretch(const uint8_t* __restrict__ img, int w, int stride, float fmin, float frange, float* __restrict__ out) {
  const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
  if (x >= w) return;
  out[(size_t)y * w + x] = ((float)img[(size_t)y * stride + x] - fmin) / frange * 255.0f;
}

// One row per blockIdx.y, 256 output pixels per workgroup: the 256 + 2 W source pixels (clamped at the borders) in LDS.
__global__ __launch_bounds__(256) void k_blur_rows(const float* __restrict__ src, float* __restrict__ dst, int w, const float* __restrict__ taps, int W) {
  __shared__ float tile[256 + 2 * SIFT_MAX_RADIUS];
  const int x0 = blockIdx.x * 256, y = blockIdx.y;
  const float* row = src + (size_t)y * w;
  for (int i = threadIdx.x; i < 256 + 2 * W; i += 256) tile[i] = row[min(max(x0 - W + i, 0), w - 1)];
  __syncthreads();
  const int x = x0 + threadIdx.x;
  if (x >= w) return;
  float acc = 0.f;
  for (int i = 0; i <= 2 * W; i++) acc = acc + taps[i] * tile[threadIdx.x + i];
  dst[(size_t)y * w + x] = acc;
}

// A tile of 32 x 32 output pixels per workgroup of 32 x 8 threads (four rows each): its 32 + 2 W source rows in LDS.
__global__ __launch_bounds__(256) void k_blur_cols(const float* __restrict__ src, float* __restrict__ dst, int w, int h, const float* __restrict__ taps, int W) {
  __shared__ float tile[32 + 2 * SIFT_MAX_RADIUS][32];
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  const int x0 = blockIdx.x * 32, y0 = blockIdx.y * 32;
  const int xs = min(x0 + tx, w - 1);
  for (int r = ty; r < 32 + 2 * W; r += 8) tile[r][tx] = src[(size_t)min(max(y0 - W + r, 0), h - 1) * w + xs];
  __syncthreads();
  const int x = x0 + tx;
  if (x >= w) return;
#pragma unroll
  for (int j = 0; j < 4; j++) {
    const int oy = ty + 8 * j, y = y0 + oy;
    if (y >= h) continue;
    float acc = 0.f;
    for (int i = 0; i <= 2 * W; i++) acc = acc + taps[i] * tile[oy + i][tx];
    dst[(size_t)y * w + x] = acc;
  }
}

__global__ __launch_bounds__(256) void k_decimate(const float* __restrict__ src, int sw, float* __restrict__ dst, int dw) {
  const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
  if (x >= dw) return;
  dst[(size_t)y * dw + x] = src[(size_t)(2 * y) * sw + 2 * x];
}

__device__ static inline float grad_angle(float gx, float gy) {
  const float ax = fabsf(gx), ay = fabsf(gy);
  const float mx = fmaxf(ax, ay), mn = fminf(ax, ay);
  if (mx == 0.f) return 0.f;
  const float t = mn / mx, q = t * t;
  float r = t * (0.99997726f + q * (-0.33262347f + q * (0.19354346f + q * (-0.11643287f + q * (0.05265332f + q * -0.01172120f)))));
  if (ay > ax) r = 1.57079637f - r;
  if (gx < 0.f) r = 3.14159274f - r;
  if (gy < 0.f) r = SIFT_PI2 - r;
  if (r >= SIFT_PI2) r = r - SIFT_PI2;
  return r;
}

__global__ __launch_bounds__(256) void k_gradient(const float* __restrict__ I, int w, int h, float* __restrict__ mod, float* __restrict__ ang) {
  const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
  if (x >= w) return;
  const float* row = I + (size_t)y * w;
  float gx, gy;
  if (x == 0) gx = row[1] - row[0];
  else if (x == w - 1) gx = row[w - 1] - row[w - 2];
  else gx = 0.5f * (row[x + 1] - row[x - 1]);
  if (y == 0) gy = I[(size_t)w + x] - I[x];
  else if (y == h - 1) gy = I[(size_t)(h - 1) * w + x] - I[(size_t)(h - 2) * w + x];
  else gy = 0.5f * (I[(size_t)(y + 1) * w + x] - I[(size_t)(y - 1) * w + x]);
  mod[(size_t)y * w + x] = sqrtf(gx * gx + gy * gy);
  ang[(size_t)y * w + x] = grad_angle(gx, gy);
}

// lane 0: s_n = sqrtf(sum of s_h[b]^2, b ascending) + EPS
__device__ static inline void ordered_norm(const float* s_h, float* s_n) {
  float s = 0.f;
  for (int b = 0; b < 128; b++) s = s + s_h[b] * s_h[b];
  *s_n = sqrtf(s) + SIFT_EPS;
}

__global__ __launch_bounds__(128) void k_describe(Levels L, const SiftFrame* __restrict__ frames, const float* __restrict__ T, int quantize,
                                                   float* __restrict__ rows, float* __restrict__ kp) {
  __shared__ float s_T[SIFT_TABLE];
  __shared__ float r_base[128], r_rx[128], r_ry[128], r_rt[128];
  __shared__ int r_code[128];   // (bx + 3) | (by + 3) << 4 | bt << 8
  __shared__ int s_cnt[2];
  __shared__ float s_h[128];
  __shared__ float s_n;
  const int f = blockIdx.x, lane = threadIdx.x, wave = lane >> 6, wl = lane & 63;
  const SiftFrame F = frames[f];
  float* row = rows + (size_t)f * 128;
  if (lane == 0) { kp[2 * (size_t)f] = F.x; kp[2 * (size_t)f + 1] = F.y; }
  const int w = L.w[F.o], h = L.h[F.o];
  const float sc = (float)(1 << F.o);
  const float xp = F.x / sc, yp = F.y / sc, sp = F.sigma / sc;
  const float xf = xp + 0.5f, yf = yp + 0.5f;
  if (!(xf > -1.0f && xf < (float)w && yf > -1.0f && yf < (float)(h - 1))) {   // the same for every lane
    row[lane] = 0.f;
    return;
  }
  for (int i = lane; i < SIFT_TABLE; i += 128) s_T[i] = T[i];
  const int xi = (int)xf, yi = (int)yf;
  const float SBP = 3.0f * sp + SIFT_EPS;
  const float Wf = floorf(1.41421356f * SBP * 2.5f + 0.5f);
  const int W = Wf < 32768.0f ? (int)Wf : 32768;
  const int dy0 = max(-W, 1 - yi), dy1 = min(W, h - yi - 2), dx0 = max(-W, 1 - xi), dx1 = min(W, w - xi - 2);
  const int nxw = dx1 - dx0 + 1, nyw = dy1 - dy0 + 1;
  const int total = (nxw > 0 && nyw > 0) ? nxw * nyw : 0;   // at most 16384^2
  const size_t plane = (size_t)w * h;
  const float* mod = L.base[F.o] + (size_t)(L.S + 3 + 2 * F.is) * plane;
  const float* ang = mod + plane;
  const int t = lane & 7, cx = ((lane >> 3) & 3) - 2, cy = (lane >> 5) - 2;   // this lane's bin
  float acc = 0.f;
  __syncthreads();
  for (int p0 = 0; p0 < total; p0 += 128) {
    const int p = p0 + lane;
    bool valid = false;
    float base = 0.f, rx = 0.f, ry = 0.f, rt = 0.f;
    int code = 0;
    if (p < total) {
      const int px = xi + dx0 + p % nxw, py = yi + dy0 + p / nxw;
      const size_t at = (size_t)py * w + px;
      const float dx = (float)px - xp, dy = (float)py - yp;
      const float nx = (F.ct * dx + F.st * dy) / SBP, ny = ((-F.st) * dx + F.ct * dy) / SBP;
      const float u = ((nx * nx + ny * ny) * 0.125f) * 10.24f;
      const float bx = floorf(nx - 0.5f), by = floorf(ny - 0.5f);
      if (u < 256.0f && bx >= -3.0f && bx <= 1.0f && by >= -3.0f && by <= 1.0f) {
        valid = true;
        float th = ang[at] - F.thr;
        if (th < 0.f) th = th + SIFT_PI2;
        if (th >= SIFT_PI2) th = th - SIFT_PI2;
        const float nt = (8.0f * th) / SIFT_PI2;
        const float bt = floorf(nt);
        const int i = (int)u;
        const float fr = u - (float)i;
        const float win = s_T[i] + fr * (s_T[i + 1] - s_T[i]);
        base = win * mod[at];
        rx = nx - (bx + 0.5f); ry = ny - (by + 0.5f); rt = nt - bt;
        code = ((int)bx + 3) | (((int)by + 3) << 4) | ((int)bt << 8);
      }
    }
    const unsigned long long mask = __ballot(valid);
    if (wl == 0) s_cnt[wave] = __popcll(mask);
    __syncthreads();
    const int c0 = s_cnt[0], cnt = c0 + s_cnt[1];
    if (valid) {
      const int q = (wave ? c0 : 0) + __popcll(mask & ((1ull << wl) - 1ull));
      r_base[q] = base; r_rx[q] = rx; r_ry[q] = ry; r_rt[q] = rt; r_code[q] = code;
    }
    __syncthreads();
    for (int q = 0; q < cnt; q++) {
      const int c = r_code[q];
      const int dbx = cx - ((c & 15) - 3), dby = cy - (((c >> 4) & 15) - 3), dbt = (t - (c >> 8)) & 7;
      if ((unsigned)dbx < 2u && (unsigned)dby < 2u && dbt < 2) {
        const float vx = r_rx[q], vy = r_ry[q], vt = r_rt[q];
        const float wx = dbx ? fabsf(vx) : fabsf(1.0f - vx);
        const float wy = dby ? fabsf(vy) : fabsf(1.0f - vy);
        const float wt = dbt ? fabsf(vt) : fabsf(1.0f - vt);
        acc = acc + ((r_base[q] * wx) * wy) * wt;
      }
    }
    __syncthreads();
  }
  s_h[lane] = acc;
  __syncthreads();
  if (lane == 0) ordered_norm(s_h, &s_n);
  __syncthreads();
  float v = acc / s_n;
  v = fminf(v, 0.2f);
  s_h[lane] = v;
  __syncthreads();
  if (lane == 0) ordered_norm(s_h, &s_n);
  __syncthreads();
  v = v / s_n;
  const int col = ((8 - t) & 7) + 8 * (cx + 2) + 32 * (3 - (cy + 2));   // transpose_descriptor
  v = 512.0f * v;
  if (quantize) v = fminf((float)(int)v, 255.0f);
  row[col] = v;
}

}  // namespace sift

#define SF_TRY(e) HIP_TRY(ctx, (e))
// an allocation that fails is the refusal MSFM_E_NOMEM, and leaves no sticky error behind
#define SF_ALLOC(e)                                                                                              \
  do {                                                                                                           \
    if ((e) != hipSuccess) {                                                                                     \
      (void)hipGetLastError();                                                                                   \
      return msfm_set_error(ctx, MSFM_E_NOMEM, "%s: the levels of %d x %d pixels do not fit", who, width, height); \
    }                                                                                                            \
  } while (0)

MSFM_API int msfm_scalespace_create(msfm_ctx* ctx, const uint8_t* gray, int width, int height, int stride, int n_octaves, int n_levels,
                                    msfm_scalespace** out) {
  using namespace sift;
  const char* who = "msfm_scalespace_create";
  if (!ctx) return MSFM_E_INVAL;
  if (!out) return msfm_set_error(ctx, MSFM_E_INVAL, "%s: null argument", who);
  *out = nullptr;
  const std::string bad = sift_check_create(gray, width, height, stride, n_octaves, n_levels);
  if (!bad.empty()) return msfm_set_error(ctx, MSFM_E_INVAL, "%s: %s", who, bad.c_str());
  const int O = n_octaves, S = n_levels;
  // host data: the taps of the S + 3 blurs (the same in every octave) and the window table
  std::vector<float> taps;
  std::vector<int> tap_off(S + 3), tap_W(S + 3);
  for (int s = -1; s <= S + 1; s++) {
    const std::vector<float> g = sift_taps(sift_level_blur(S, s));
    tap_off[s + 1] = (int)taps.size();
    tap_W[s + 1] = (int)(g.size() / 2);
    if (tap_W[s + 1] > SIFT_MAX_RADIUS) return msfm_set_error(ctx, MSFM_E_INVAL, "%s: a blur radius of %d exceeds %d", who, tap_W[s + 1], SIFT_MAX_RADIUS);
    taps.insert(taps.end(), g.begin(), g.end());
  }
  std::unique_ptr<msfm_scalespace> P(new msfm_scalespace());
  P->ctx = ctx; P->w = width; P->h = height; P->O = O; P->S = S;
  for (int o = 0; o < O; o++) { P->ow[o] = width >> o; P->oh[o] = height >> o; }
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  DevBuf<uint8_t> d_img;
  DevBuf<unsigned> d_mm;
  DevBuf<float> d_taps, d_a, d_b;
  DevScope sc(ctx);
  const dim3 g0(cdiv(width, 256), height);
  SF_ALLOC(sc.up(d_img, gray, (size_t)(height - 1) * stride + width));
  SF_ALLOC(d_mm.alloc(2));
  SF_TRY(hipMemsetAsync(d_mm.p, 0xFF, sizeof(unsigned), st));
  SF_TRY(hipMemsetAsync(d_mm.p + 1, 0, sizeof(unsigned), st));
  {
    KTimer t(ctx, "sift_stretch");
    hipLaunchKernelGGL(k_minmax, dim3(std::min(height, 1024)), dim3(256), 0, st, d_img.p, width, height, stride, d_mm.p);
  }
  SF_TRY(hipGetLastError());
  unsigned mm[2] = {0, 0};
  SF_TRY(sc.down(mm, d_mm.p, 2));
  SF_TRY(hipStreamSynchronize(st));   // the range decides whether there is anything to build
  if (mm[1] <= mm[0]) return msfm_set_error(ctx, MSFM_E_INVAL, "%s: a constant image (every pixel is %u)", who, mm[0]);
  SF_ALLOC(sc.up(d_taps, taps));
  SF_ALLOC(sc.up(P->table, sift_table()));
  SF_ALLOC(d_a.alloc((size_t)width * height));
  SF_ALLOC(d_b.alloc((size_t)width * height));
  for (int o = 0; o < O; o++) SF_ALLOC(P->oct[o].alloc((size_t)(3 * S + 3) * P->npx(o)));
  {
    KTimer t(ctx, "sift_stretch");
    hipLaunchKernelGGL(k_stretch, g0, dim3(256), 0, st, d_img.p, width, stride, (float)mm[0], (float)(mm[1] - mm[0]), d_a.p);
  }
  for (int o = 0; o < O; o++) {
    const int w = P->ow[o], h = P->oh[o];
    const dim3 gr(cdiv(w, 256), h), gc(cdiv(w, 32), cdiv(h, 32));
    float* const base = P->oct[o].p;
    const size_t npx = P->npx(o);
    if (o > 0) {
      KTimer t(ctx, "sift_decimate");
      hipLaunchKernelGGL(k_decimate, gr, dim3(256), 0, st, P->level(o - 1, S - 1), P->ow[o - 1], base, w);
    }
    for (int s = (o == 0 ? -1 : 0); s <= S + 1; s++) {
      const float* src = (o == 0 && s == -1) ? d_a.p : base + (size_t)s * npx;   // level s - 1
      const float* g = d_taps.p + tap_off[s + 1];
      {
        KTimer t(ctx, "sift_blur_rows");
        hipLaunchKernelGGL(k_blur_rows, gr, dim3(256), 0, st, src, d_b.p, w, g, tap_W[s + 1]);
      }
      {
        KTimer t(ctx, "sift_blur_cols");
        hipLaunchKernelGGL(k_blur_cols, gc, dim3(256), 0, st, d_b.p, base + (size_t)(s + 1) * npx, w, h, g, tap_W[s + 1]);
      }
    }
    KTimer t(ctx, "sift_gradient");
    t.count = S;
    for (int s = 0; s < S; s++)
      hipLaunchKernelGGL(k_gradient, gr, dim3(256), 0, st, P->level(o, s), w, h, base + (size_t)(S + 3 + 2 * s) * npx, base + (size_t)(S + 4 + 2 * s) * npx);
  }
  SF_TRY(hipGetLastError());
  SF_TRY(sc.finish());
  P->h2d_bytes = sc.h2d;
  ctx->children++;
  *out = P.release();
  return MSFM_OK;
}

MSFM_API int msfm_scalespace_size(const msfm_scalespace* P, int octave, int* w, int* h, int64_t* h2d_bytes) {
  if (!P) return MSFM_E_INVAL;
  if (octave < 0 || octave >= P->O) return msfm_set_error(P->ctx, MSFM_E_INVAL, "msfm_scalespace_size: octave %d outside [0, %d)", octave, P->O);
  if (w) *w = P->ow[octave];
  if (h) *h = P->oh[octave];
  if (h2d_bytes) *h2d_bytes = P->h2d_bytes;
  return MSFM_OK;
}

MSFM_API int msfm_scalespace_fetch(const msfm_scalespace* P, int octave, int level, int kind, float* out) {
  const char* who = "msfm_scalespace_fetch";
  if (!P) return MSFM_E_INVAL;
  msfm_ctx* ctx = P->ctx;
  if (!out) return msfm_set_error(ctx, MSFM_E_INVAL, "%s: null argument", who);
  if (octave < 0 || octave >= P->O) return msfm_set_error(ctx, MSFM_E_INVAL, "%s: octave %d outside [0, %d)", who, octave, P->O);
  if (kind < 0 || kind > 2) return msfm_set_error(ctx, MSFM_E_INVAL, "%s: kind %d outside [0, 2]", who, kind);
  if (kind == 0 ? (level < -1 || level > P->S + 1) : (level < 0 || level > P->S - 1))
    return msfm_set_error(ctx, MSFM_E_INVAL, "%s: level %d outside the range of kind %d", who, level, kind);
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  DevScope sc(ctx);
  SF_TRY(sc.down(out, kind == 0 ? P->level(octave, level) : P->grad(octave, level, kind - 1), P->npx(octave)));
  SF_TRY(sc.finish());
  return MSFM_OK;
}

MSFM_API void msfm_scalespace_destroy(msfm_scalespace* P) {
  if (!P) return;
  msfm_ctx* ctx = P->ctx;
  (void)hipSetDevice(ctx->device);
  (void)hipStreamSynchronize(ctx->stream);   // blocks go back to the pool only behind the work that may still read them
  delete P;
  msfm_ctx_child_released(ctx);
}

MSFM_API int msfm_descset_describe(msfm_descset* set, int image, const msfm_scalespace* P, const float* frames, int n, int quantize,
                                   int64_t* h2d_bytes) {
  using namespace sift;
  const char* who = "msfm_descset_describe";
  if (!set) return MSFM_E_INVAL;
  DescView V;
  descset_view(set, &V);
  msfm_ctx* ctx = V.ctx;
  if (!P) return msfm_set_error(ctx, MSFM_E_INVAL, "%s: null argument", who);
  if (P->ctx != ctx) return msfm_set_error(ctx, MSFM_E_INVAL, "%s: the scale space belongs to another context", who);
  if (image < 0 || image >= V.n_images) return msfm_set_error(ctx, MSFM_E_INVAL, "%s: image %d outside the set of %d", who, image, V.n_images);
  std::vector<SiftFrame> rec;
  const std::string bad = sift_frames(frames, n, P->O, P->S, &rec);
  if (!bad.empty()) return msfm_set_error(ctx, MSFM_E_INVAL, "%s: %s", who, bad.c_str());
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  Levels L;
  for (int o = 0; o < SIFT_MAX_OCTAVES; o++) { L.base[o] = P->oct[o].p; L.w[o] = P->ow[o]; L.h[o] = P->oh[o]; }
  L.S = P->S;
  DevBuf<SiftFrame> d_rec;
  DevScope sc(ctx);
  MSFM_TRY(descset_put_dev(set, image, n, true, "descset_prep", [&](float* d_rows, float* d_kp, hipStream_t st) {
    const hipError_t e = sc.up(d_rec, rec);
    if (e != hipSuccess) return e;
    KTimer t(ctx, "sift_describe");
    hipLaunchKernelGGL(k_describe, dim3(n), dim3(128), 0, st, L, d_rec.p, P->table.p, quantize ? 1 : 0, d_rows, d_kp);
    return hipGetLastError();
  }));
  sc.dismiss();   // behind the core's wait for the flags
  if (h2d_bytes) *h2d_bytes = sc.h2d;
  return MSFM_OK;
}
