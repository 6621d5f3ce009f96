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
// msfm_scalespace_detect    the detecting arm (nikeys < 0: vl_sift_detect, vl_sift_calc_keypoint_orientations,
//                           feature_extractor_vl_sift.cpp:130-136, :171-173).  k_extrema: three DoG levels of a 256 x 8 tile and
//                           their halo in LDS, each value one subtraction of two resident levels, one launch per octave for
//                           its S levels, a wave's 64 verdicts one mask word.  k_count_words, k_scan_blocks, k_emit_cells: the
//                           ordered compaction of the set bits, a candidate's position a prefix sum.  Wait 1 (the count sizes the
//                           buffers).  k_refine: one lane per candidate.  Wait 2: the host counts the rejections, keeps the
//                           accepted in order and makes sigmaw (pow).  k_orient: one wave per keypoint, lane = bin, k_describe's
//                           record walk.  Wait 3: the angles; the frames are made on the host (pow again).
// msfm_descset_extract      detect_frames, then describe_frames: the code msfm_descset_describe runs.
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

// ---- the detector ----

#define SIFT_EX_ROWS 8   // rows of a k_extrema tile; its width is the workgroup's 256 lanes

struct Octaves {   // what the detector's kernels need of a scale space, and where an octave's extremum masks lie
  const float* base[SIFT_MAX_OCTAVES];
  int w[SIFT_MAX_OCTAVES], h[SIFT_MAX_OCTAVES], xw[SIFT_MAX_OCTAVES];   // xw: mask words per row, cdiv(w, 64)
  int word0[SIFT_MAX_OCTAVES + 1];                                      // first word of the octave's [S][h][xw] masks
  int O, S;
};

// One workgroup: the pixels x0 .. x0 + 255, y0 .. y0 + 7 of DoG level s = blockIdx.z of octave o.  The three DoG levels s - 1, s,
// s + 1 of the tile and a halo of one pixel (clamped at the borders; a clamped value is never compared) go to LDS, each value one
// subtraction of two resident levels.  Lane tx tests its column row by row; a wave's 64 verdicts are one mask word.
__global__ __launch_bounds__(256) void k_extrema(Octaves L, int o, float thr, unsigned long long* __restrict__ words) {
  __shared__ float D[3][SIFT_EX_ROWS + 2][258];
  const int w = L.w[o], h = L.h[o], xw = L.xw[o], s = blockIdx.z;
  const int x0 = blockIdx.x * 256, y0 = blockIdx.y * SIFT_EX_ROWS, tx = threadIdx.x;
  const size_t npx = (size_t)w * h;
  const float* G = L.base[o];
  for (int i = tx; i < 3 * (SIFT_EX_ROWS + 2) * 258; i += 256) {
    const int l = i / ((SIFT_EX_ROWS + 2) * 258), r = i % ((SIFT_EX_ROWS + 2) * 258);
    const int ry = r / 258, cx = r % 258;
    const int gx = min(max(x0 - 1 + cx, 0), w - 1), gy = min(max(y0 - 1 + ry, 0), h - 1);
    const size_t p = (size_t)gy * w + gx;
    (&D[0][0][0])[i] = G[(size_t)(s + l + 1) * npx + p] - G[(size_t)(s + l) * npx + p];   // D(s - 1 + l) = G(s + l) - G(s - 1 + l); level t lies at t + 1
  }
  __syncthreads();
  const int x = x0 + tx;
  unsigned long long* out = words + L.word0[o] + ((size_t)s * h) * xw + (x0 >> 6) + (tx >> 6);
  for (int r = 0; r < SIFT_EX_ROWS; r++) {
    const int y = y0 + r;
    if (y >= h) break;   // the same for every lane
    bool ext = false;
    if (x >= 1 && x <= w - 2 && y >= 1 && y <= h - 2) {
      const float v = D[1][r + 1][tx + 1];
      bool mx = v >= thr, mn = v <= -thr;
#pragma unroll
      for (int k = 0; k < 3; k++)
#pragma unroll
        for (int j = 0; j < 3; j++)
#pragma unroll
          for (int i = 0; i < 3; i++)
            if (k != 1 || j != 1 || i != 1) {
              const float n = D[k][r + j][tx + i];
              mx = mx && v > n;
              mn = mn && v < n;
            }
      ext = mx || mn;
    }
    const unsigned long long mask = __ballot(ext);
    if ((tx & 63) == 0 && x0 + (tx & ~63) < w) out[(size_t)y * xw] = mask;
  }
}

// The ordered compaction of the mask words' set bits: k_count_words (set bits per block of 1024 words), k_scan_blocks (one
// workgroup: the exclusive sums of the blocks and the total), k_emit_cells (the cell of every set bit at its position).
__device__ static inline int block_exclusive(int v, int* s_scan, int* total) {   // 256 lanes; s_scan [256]
  const int t = threadIdx.x;
  s_scan[t] = v;
  __syncthreads();
  for (int d = 1; d < 256; d <<= 1) {
    const int a = t >= d ? s_scan[t - d] : 0;
    __syncthreads();
    s_scan[t] += a;
    __syncthreads();
  }
  const int incl = s_scan[t];
  *total = s_scan[255];
  __syncthreads();
  return incl - v;
}

__device__ static inline int four_words(const unsigned long long* __restrict__ words, int nwords, int first, unsigned long long* m) {
  int c = 0;
#pragma unroll
  for (int i = 0; i < 4; i++) {
    m[i] = first + i < nwords ? words[first + i] : 0ull;
    c += __popcll(m[i]);
  }
  return c;
}

__global__ __launch_bounds__(256) void k_count_words(const unsigned long long* __restrict__ words, int nwords, int* __restrict__ bsum) {
  __shared__ int s_scan[256];
  unsigned long long m[4];
  int total;
  (void)block_exclusive(four_words(words, nwords, (blockIdx.x * 256 + threadIdx.x) * 4, m), s_scan, &total);
  if (threadIdx.x == 0) bsum[blockIdx.x] = total;
}

// bsum [nb] -> its exclusive sums in place, and total[0]
__global__ __launch_bounds__(256) void k_scan_blocks(int* __restrict__ bsum, int nb, int* __restrict__ total) {
  __shared__ int s_scan[256];
  int carry = 0;
  for (int b0 = 0; b0 < nb; b0 += 256) {
    const int b = b0 + threadIdx.x;
    int chunk;
    const int ex = block_exclusive(b < nb ? bsum[b] : 0, s_scan, &chunk);
    if (b < nb) bsum[b] = carry + ex;
    carry += chunk;
  }
  if (threadIdx.x == 0) total[0] = carry;
}

// cells [n_cand]: x | y << 16 | s << 32 | o << 40 of every set bit, in the order of the words and of the bits in them
__global__ __launch_bounds__(256) void k_emit_cells(Octaves L, const unsigned long long* __restrict__ words, int nwords, const int* __restrict__ boff,
                                                     int n_cand, unsigned long long* __restrict__ cells) {
  __shared__ int s_scan[256];
  unsigned long long m[4];
  const int first = (blockIdx.x * 256 + threadIdx.x) * 4;
  int total;
  int pos = boff[blockIdx.x] + block_exclusive(four_words(words, nwords, first, m), s_scan, &total);
#pragma unroll
  for (int i = 0; i < 4; i++) {
    unsigned long long bits = m[i];
    if (!bits) continue;
    const int wi = first + i;
    int o = 0;
    while (o + 1 < L.O && wi >= L.word0[o + 1]) o++;
    const int rem = wi - L.word0[o], xw = L.xw[o], h = L.h[o];
    const unsigned long long hi = ((unsigned long long)((rem / xw) % h) << 16) | ((unsigned long long)(rem / (xw * h)) << 32) | ((unsigned long long)o << 40);
    const int xb = (rem % xw) * 64;
    while (bits) {   // at most 64 rounds
      const int bit = __ffsll((long long)bits) - 1;
      bits &= bits - 1;
      if (pos < n_cand) cells[pos] = hi | (unsigned long long)(xb + bit);
      pos++;
    }
  }
}

// One lane per candidate: the refinement of include/msfm.h, every D value one subtraction of two resident levels.
__global__ __launch_bounds__(256) void k_refine(Octaves L, const unsigned long long* __restrict__ cells, int n_cand, float peak, float bound,
                                                SiftRawKp* __restrict__ raw) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= n_cand) return;
  const unsigned long long cell = cells[c];
  const int o = min((int)(cell >> 40) & 255, L.O - 1), w = L.w[o], h = L.h[o];
  const int s = min((int)(cell >> 32) & 255, L.S - 1), x_first = min(max((int)(cell & 0xFFFF), 1), w - 2), y_first = min(max((int)(cell >> 16) & 0xFFFF, 1), h - 2);
  const size_t npx = (size_t)w * h;
  const float* G = L.base[o] + (size_t)(s + 1) * npx;   // level s
  int x = x_first, y = y_first;
  float Dx = 0.f, Dy = 0.f, Ds = 0.f, Dxx = 0.f, Dyy = 0.f, Dxy = 0.f, v0 = 0.f, b[3] = {0.f, 0.f, 0.f};
  int mvx = 0, mvy = 0;
  for (int pass = 0; pass < 5; pass++) {
    x += mvx; y += mvy;
    const size_t p = (size_t)y * w + x;
#define AT(i, j, k) (G[(ptrdiff_t)((k) + 1) * (ptrdiff_t)npx + (ptrdiff_t)p + (j) * w + (i)] - G[(ptrdiff_t)(k) * (ptrdiff_t)npx + (ptrdiff_t)p + (j) * w + (i)])
    v0 = AT(0, 0, 0);
    const float xp = AT(1, 0, 0), xm = AT(-1, 0, 0), yp = AT(0, 1, 0), ym = AT(0, -1, 0), sp = AT(0, 0, 1), sm = AT(0, 0, -1);
    Dx = 0.5f * (xp - xm); Dy = 0.5f * (yp - ym); Ds = 0.5f * (sp - sm);
    Dxx = (xp + xm) - 2.0f * v0; Dyy = (yp + ym) - 2.0f * v0;
    const float Dss = (sp + sm) - 2.0f * v0;
    Dxy = 0.25f * (((AT(1, 1, 0) + AT(-1, -1, 0)) - AT(-1, 1, 0)) - AT(1, -1, 0));
    const float Dxs = 0.25f * (((AT(1, 0, 1) + AT(-1, 0, -1)) - AT(-1, 0, 1)) - AT(1, 0, -1));
    const float Dys = 0.25f * (((AT(0, 1, 1) + AT(0, -1, -1)) - AT(0, -1, 1)) - AT(0, 1, -1));
#undef AT
    float A[3][3] = {{Dxx, Dxy, Dxs}, {Dxy, Dyy, Dys}, {Dxs, Dys, Dss}};
    b[0] = -Dx; b[1] = -Dy; b[2] = -Ds;
    bool singular = false;
#pragma unroll
    for (int j = 0; j < 3; j++) {
      if (singular) continue;
      int pi = j;
      float pa = fabsf(A[j][j]);
#pragma unroll
      for (int i = j + 1; i < 3; i++)
        if (fabsf(A[i][j]) > pa) { pa = fabsf(A[i][j]); pi = i; }
      if (!(pa > 0.f)) { singular = true; continue; }
#pragma unroll
      for (int i = j + 1; i < 3; i++)
        if (pi == i) {
#pragma unroll
          for (int jj = j; jj < 3; jj++) { const float t = A[i][jj]; A[i][jj] = A[j][jj]; A[j][jj] = t; }
          const float t = b[i]; b[i] = b[j]; b[j] = t;
        }
      const float pv = A[j][j];
#pragma unroll
      for (int jj = j; jj < 3; jj++) A[j][jj] = A[j][jj] / pv;
      b[j] = b[j] / pv;
#pragma unroll
      for (int ii = j + 1; ii < 3; ii++) {
        const float f = A[ii][j];
#pragma unroll
        for (int jj = j; jj < 3; jj++) A[ii][jj] = A[ii][jj] - f * A[j][jj];
        b[ii] = b[ii] - f * b[j];
      }
    }
    if (singular) { b[0] = 0.f; b[1] = 0.f; b[2] = 0.f; }
    else {
      b[1] = b[1] - b[2] * A[1][2];
      b[0] = b[0] - b[2] * A[0][2];
      b[0] = b[0] - b[1] * A[0][1];
    }
    mvx = (b[0] > 0.6f && x < w - 2 ? 1 : 0) + (b[0] < -0.6f && x > 1 ? -1 : 0);
    mvy = (b[1] > 0.6f && y < h - 2 ? 1 : 0) + (b[1] < -0.6f && y > 1 ? -1 : 0);
    if (mvx == 0 && mvy == 0) break;
  }
  const float val = v0 + 0.5f * ((Dx * b[0] + Dy * b[1]) + Ds * b[2]);
  const float score = ((Dxx + Dyy) * (Dxx + Dyy)) / (Dxx * Dyy - Dxy * Dxy);
  const float xn = (float)x + b[0], yn = (float)y + b[1], sn = (float)s + b[2];
  int status = 0;
  if (!(fabsf(val) > peak)) status = 1;
  else if (!(score < bound)) status = 2;
  else if (!(score >= 0.f)) status = 3;
  else if (!(fabsf(b[0]) < 1.5f && fabsf(b[1]) < 1.5f && fabsf(b[2]) < 1.5f)) status = 4;
  else if (!(xn >= 0.f && xn <= (float)(w - 1) && yn >= 0.f && yn <= (float)(h - 1) && sn >= -1.0f && sn <= (float)(L.S + 1))) status = 5;
  SiftRawKp r;
  r.o = o; r.ix = x; r.iy = y; r.is = s; r.xn = xn; r.yn = yn; r.sn = sn;
  r.flags = status | ((x != x_first || y != y_first) ? SIFT_KP_MOVED : 0) | ((mvx != 0 || mvy != 0) ? SIFT_KP_UNCONVERGED : 0);
  raw[c] = r;
}

// One wave (a workgroup of 64 lanes) per keypoint, lane = orientation bin.  The window's pixels are taken 64 at a time in raster
// order; every lane makes one pixel's record (win * mod, the bin, the remainder), the kept ones are packed in order into LDS by a
// ballot, and the lanes 0 .. 35 walk them in order and add what touches their bin, as k_describe does.
__global__ __launch_bounds__(64) void k_orient(Octaves L, const SiftOrientIn* __restrict__ in, const float* __restrict__ T, int* __restrict__ nang,
                                               float* __restrict__ theta) {
  __shared__ float s_T[SIFT_TABLE];
  __shared__ float r_v[64], r_rb[64];
  __shared__ int r_ib[64];
  __shared__ float s_h[SIFT_ORI_BINS];
  const int k = blockIdx.x, lane = threadIdx.x;
  const SiftOrientIn K = in[k];
  const int o = min(max(K.o, 0), L.O - 1), is = min(max(K.is, 0), L.S - 1), w = L.w[o], h = L.h[o];
  for (int i = lane; i < SIFT_TABLE; i += 64) s_T[i] = T[i];
  const size_t plane = (size_t)w * h;
  const float* mod = L.base[o] + (size_t)(L.S + 3 + 2 * is) * plane;
  const float* ang = mod + plane;
  const float xn = K.xn, yn = K.yn, sw = K.sigmaw;
  const int xi = min(max((int)(xn + 0.5f), 0), w - 1), yi = min(max((int)(yn + 0.5f), 0), h - 1);
  const float Wf = floorf(3.0f * sw);
  const int W = Wf >= 0.f ? (Wf < 1024.0f ? (int)Wf : 1024) : 0;   // 57 at most for a sigmaw the host made
  const float r2max = (float)(W * W) + 0.6f, den = (2.0f * sw) * sw;
  const int dy0 = max(-W, 1 - yi), dy1 = min(W, h - yi - 2), dx0 = max(-W, 1 - xi), dx1 = min(W, w - xi - 2);
  const int nxw = dx1 - dx0 + 1, nyw = dy1 - dy0 + 1;
  const int total = (nxw > 0 && nyw > 0) ? nxw * nyw : 0;   // at most 2049^2
  float acc = 0.f;
  __syncthreads();
  for (int p0 = 0; p0 < total; p0 += 64) {
    const int p = p0 + lane;
    bool valid = false;
    float v = 0.f, rb = 0.f;
    int ib = 0;
    if (p < total) {
      const int px = xi + dx0 + p % nxw, py = yi + dy0 + p / nxw;
      const size_t at = (size_t)py * w + px;
      const float dx = (float)px - xn, dy = (float)py - yn;
      const float r2 = dx * dx + dy * dy;
      const float u = (r2 / den) * 10.24f;
      if (r2 < r2max && u < 256.0f) {
        valid = true;
        const int i = (int)u;
        const float fr = u - (float)i;
        const float win = s_T[i] + fr * (s_T[i + 1] - s_T[i]);
        v = win * mod[at];
        const float fb = (36.0f * ang[at]) / SIFT_PI2;
        const float bf = floorf(fb - 0.5f);
        rb = fb - (bf + 0.5f);
        ib = (min(max((int)bf, -1), SIFT_ORI_BINS) + SIFT_ORI_BINS) % SIFT_ORI_BINS;
      }
    }
    const unsigned long long mask = __ballot(valid);
    const int cnt = __popcll(mask);
    if (valid) {
      const int q = __popcll(mask & ((1ull << lane) - 1ull));
      r_v[q] = v; r_rb[q] = rb; r_ib[q] = ib;
    }
    __syncthreads();
    for (int q = 0; q < cnt; q++) {
      const int d = lane - r_ib[q];
      if (d == 0) acc = acc + (1.0f - r_rb[q]) * r_v[q];
      else if (d == 1 || d == 1 - SIFT_ORI_BINS) acc = acc + r_rb[q] * r_v[q];
    }
    __syncthreads();
  }
  const int bin = min(lane, SIFT_ORI_BINS - 1), bm = (bin + SIFT_ORI_BINS - 1) % SIFT_ORI_BINS, bp = (bin + 1) % SIFT_ORI_BINS;
  if (lane < SIFT_ORI_BINS) s_h[lane] = acc;
  __syncthreads();
  for (int it = 0; it < 6; it++) {
    const float nv = ((s_h[bm] + s_h[bin]) + s_h[bp]) / 3.0f;
    __syncthreads();
    if (lane < SIFT_ORI_BINS) s_h[lane] = nv;
    __syncthreads();
  }
  const float h0 = s_h[bin], hm = s_h[bm], hp = s_h[bp];
  float m = h0;
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) m = fmaxf(m, __shfl_xor(m, d));
  const bool peak = lane < SIFT_ORI_BINS && h0 > 0.8f * m && h0 > hm && h0 > hp;
  const unsigned long long pm = __ballot(peak);
  const int rank = __popcll(pm & ((1ull << lane) - 1ull)), np = min(__popcll(pm), SIFT_MAX_ANGLES);
  if (peak && rank < SIFT_MAX_ANGLES) {
    const float di = (-0.5f * (hp - hm)) / ((hp + hm) - 2.0f * h0);
    theta[(size_t)SIFT_MAX_ANGLES * k + rank] = (SIFT_PI2 * (((float)lane + di) + 0.5f)) / 36.0f;
  }
  if (lane >= np && lane < SIFT_MAX_ANGLES) theta[(size_t)SIFT_MAX_ANGLES * k + lane] = 0.f;
  if (lane == 0) nang[k] = np;
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
  Child<msfm_scalespace> P = child_new<msfm_scalespace>(ctx);
  P->w = width; P->h = height; P->O = O; P->S = S;
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

MSFM_API void msfm_scalespace_destroy(msfm_scalespace* P) { msfm_child_destroy(P); }

// what describe and extract refuse before anything else: -> the set's context through *out
static int check_set_and_space(const char* who, const msfm_descset* set, int image, const msfm_scalespace* P, msfm_ctx** out) {
  DescView V;
  descset_view(set, &V);
  msfm_ctx* ctx = V.ctx;
  *out = ctx;
  if (!P) return msfm_set_error(ctx, MSFM_E_INVAL, "%s: null argument", who);
  if (P->ctx != ctx) return msfm_set_error(ctx, MSFM_E_INVAL, "%s: the scale space belongs to another context", who);
  if (image < 0 || image >= V.n_images) return msfm_set_error(ctx, MSFM_E_INVAL, "%s: image %d outside the set of %d", who, image, V.n_images);
  return MSFM_OK;
}

// frames [n][4] -> the image's rows and keypoints (the arguments are checked but for the frames); two host waits (descset_put_dev's)
static int describe_frames(const char* who, msfm_descset* set, int image, const msfm_scalespace* P, const float* frames, int n, int quantize,
                           int64_t* h2d_bytes) {
  using namespace sift;
  msfm_ctx* ctx = P->ctx;
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

MSFM_API int msfm_descset_describe(msfm_descset* set, int image, const msfm_scalespace* P, const float* frames, int n, int quantize,
                                   int64_t* h2d_bytes) {
  const char* who = "msfm_descset_describe";
  if (!set) return MSFM_E_INVAL;
  msfm_ctx* ctx = nullptr;
  MSFM_TRY(check_set_and_space(who, set, image, P, &ctx));
  return describe_frames(who, set, image, P, frames, n, quantize, h2d_bytes);
}

// The detection of include/msfm.h: every frame of the scale space in order into *frames ([n_found][4]) and the counters into st.
// Three host waits: the candidate count sizes the candidate buffers; the raw keypoints come back for the host step (rejections
// counted, accepted ones compacted in order, sigmaw made); the angles come back for the frames.
static int detect_frames(const char* who, const msfm_scalespace* P, float peak_thresh, float edge_thresh, std::vector<float>* frames, int64_t* st) {
  using namespace sift;
  msfm_ctx* ctx = P->ctx;
  const int width = P->w, height = P->h;   // (SF_ALLOC's text)
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  hipStream_t stream = ctx->stream;
  Octaves L;
  L.O = P->O; L.S = P->S;
  long nwords = 0;
  for (int o = 0; o < SIFT_MAX_OCTAVES; o++) {
    L.base[o] = P->oct[o].p; L.w[o] = P->ow[o]; L.h[o] = P->oh[o]; L.xw[o] = cdiv(P->ow[o], 64);
    L.word0[o] = (int)nwords;
    if (o < P->O) nwords += (long)P->S * L.h[o] * L.xw[o];   // at most 8 * 16384 * 256 * 4 / 3
  }
  L.word0[SIFT_MAX_OCTAVES] = (int)nwords;
  const int nb = cdiv(nwords, 1024);
  DevBuf<unsigned long long> d_words, d_cells;
  DevBuf<int> d_bsum, d_total, d_nang;
  DevBuf<SiftRawKp> d_raw;
  DevBuf<SiftOrientIn> d_in;
  DevBuf<float> d_theta;
  // The host arrays of the call are kept per thread between calls (and so outlive the scope's wait): a download into freshly
  // mapped host memory took 13 ms for the 2.3 MB of a photograph's raw keypoints, 0.05 ms into memory that a download had
  // written before.
  struct HostArrays {
    std::vector<SiftRawKp> raw;
    std::vector<int> kept, nang;
    std::vector<SiftOrientIn> in;
    std::vector<float> theta;
  };
  static thread_local HostArrays host;
  std::vector<SiftRawKp>& raw = host.raw;
  std::vector<int>&kept = host.kept, &nang = host.nang;
  std::vector<SiftOrientIn>& in = host.in;
  std::vector<float>& theta = host.theta;
  kept.clear();
  in.clear();
  DevScope sc(ctx);
  int64_t d2h = 0;
  SF_ALLOC(d_words.alloc((size_t)nwords));
  SF_ALLOC(d_bsum.alloc(nb));
  SF_ALLOC(d_total.alloc(1));
  {
    KTimer t(ctx, "sift_extrema");
    t.count = P->O;
    for (int o = 0; o < P->O; o++)
      hipLaunchKernelGGL(k_extrema, dim3(cdiv(L.w[o], 256), cdiv(L.h[o], SIFT_EX_ROWS), P->S), dim3(256), 0, stream, L, o, 0.8f * peak_thresh, d_words.p);
  }
  {
    KTimer t(ctx, "sift_compact");
    t.count = 2;
    hipLaunchKernelGGL(k_count_words, dim3(nb), dim3(256), 0, stream, d_words.p, (int)nwords, d_bsum.p);
    hipLaunchKernelGGL(k_scan_blocks, dim3(1), dim3(256), 0, stream, d_bsum.p, nb, d_total.p);
  }
  SF_TRY(hipGetLastError());
  int n_cand = 0;
  SF_TRY(sc.down(&n_cand, d_total.p, 1));
  SF_TRY(hipStreamSynchronize(stream));   // wait 1: the count sizes the candidate buffers
  d2h += sizeof(int);
  st[SIFT_ST_WAITS]++;
  raw.resize((size_t)n_cand);
  if (n_cand > 0) {
    SF_ALLOC(d_cells.alloc((size_t)n_cand));
    SF_ALLOC(d_raw.alloc((size_t)n_cand));
    {
      KTimer t(ctx, "sift_compact");
      hipLaunchKernelGGL(k_emit_cells, dim3(nb), dim3(256), 0, stream, L, d_words.p, (int)nwords, d_bsum.p, n_cand, d_cells.p);
    }
    {
      KTimer t(ctx, "sift_refine");
      hipLaunchKernelGGL(k_refine, dim3(cdiv(n_cand, 256)), dim3(256), 0, stream, L, d_cells.p, n_cand, peak_thresh, sift_edge_bound(edge_thresh), d_raw.p);
    }
    SF_TRY(hipGetLastError());
    SF_TRY(sc.down(raw.data(), d_raw.p, raw.size()));
    SF_TRY(hipStreamSynchronize(stream));   // wait 2: the host step
    d2h += (int64_t)(raw.size() * sizeof(SiftRawKp));
    st[SIFT_ST_WAITS]++;
  }
  sift_collect(raw, P->S, st, &kept, &in);
  const size_t n_kp = kept.size();
  nang.resize(n_kp);
  theta.resize(SIFT_MAX_ANGLES * n_kp);
  if (n_kp > 0) {
    SF_ALLOC(sc.up(d_in, in));
    SF_ALLOC(d_nang.alloc(n_kp));
    SF_ALLOC(d_theta.alloc(SIFT_MAX_ANGLES * n_kp));
    {
      KTimer t(ctx, "sift_orient");
      hipLaunchKernelGGL(k_orient, dim3((unsigned)n_kp), dim3(64), 0, stream, L, d_in.p, P->table.p, d_nang.p, d_theta.p);
    }
    SF_TRY(hipGetLastError());
    SF_TRY(sc.down(nang.data(), d_nang.p, n_kp));
    SF_TRY(sc.down(theta.data(), d_theta.p, theta.size()));
    d2h += (int64_t)(n_kp * sizeof(int) + theta.size() * sizeof(float));
  }
  SF_TRY(sc.finish());   // wait 3: the angles
  st[SIFT_ST_WAITS]++;
  sift_make_frames(raw, kept, nang.data(), theta.data(), P->S, st, frames);
  st[SIFT_ST_H2D] += sc.h2d;
  st[SIFT_ST_D2H] += d2h;
  return MSFM_OK;
}

MSFM_API int msfm_scalespace_detect(const msfm_scalespace* P, float peak_thresh, float edge_thresh, int max_frames, float* frames_out, int* n_out,
                                    int64_t* stats) {
  const char* who = "msfm_scalespace_detect";
  if (!P) return MSFM_E_INVAL;
  msfm_ctx* ctx = P->ctx;
  if (!frames_out || !n_out) return msfm_set_error(ctx, MSFM_E_INVAL, "%s: null argument", who);
  const std::string bad = sift_check_detect(peak_thresh, edge_thresh, max_frames);
  if (!bad.empty()) return msfm_set_error(ctx, MSFM_E_INVAL, "%s: %s", who, bad.c_str());
  int64_t st[SIFT_DETECT_STATS] = {};
  std::vector<float> frames;
  MSFM_TRY(detect_frames(who, P, peak_thresh, edge_thresh, &frames, st));
  const int n = (int)std::min<int64_t>(st[SIFT_ST_FOUND], max_frames);
  std::copy(frames.begin(), frames.begin() + 4 * (size_t)n, frames_out);
  *n_out = n;
  if (stats) std::copy(st, st + SIFT_DETECT_STATS, stats);
  return MSFM_OK;
}

MSFM_API int msfm_descset_extract(msfm_descset* set, int image, const msfm_scalespace* P, float peak_thresh, float edge_thresh, int max_frames,
                                  int quantize, int64_t* stats) {
  const char* who = "msfm_descset_extract";
  if (!set) return MSFM_E_INVAL;
  msfm_ctx* ctx = nullptr;
  MSFM_TRY(check_set_and_space(who, set, image, P, &ctx));
  const std::string bad = sift_check_detect(peak_thresh, edge_thresh, max_frames);
  if (!bad.empty()) return msfm_set_error(ctx, MSFM_E_INVAL, "%s: %s", who, bad.c_str());
  int64_t st[SIFT_DETECT_STATS] = {};
  std::vector<float> frames;
  MSFM_TRY(detect_frames(who, P, peak_thresh, edge_thresh, &frames, st));
  const int n = (int)std::min<int64_t>(st[SIFT_ST_FOUND], max_frames);
  int64_t h2d = 0;
  frames.resize(std::max<size_t>(frames.size(), 4));   // (n = 0 still hands a pointer over)
  MSFM_TRY(describe_frames(who, set, image, P, frames.data(), n, quantize, &h2d));
  st[SIFT_ST_WAITS] += 2;
  st[SIFT_ST_H2D] += h2d;
  if (stats) std::copy(st, st + SIFT_DETECT_STATS, stats);
  return MSFM_OK;
}
