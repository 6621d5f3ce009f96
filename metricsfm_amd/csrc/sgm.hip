// Dense stereo on the device: the semi-global matching of DenseReconstruction::SGMDense (SfM/src/dense_reconstruction.cc:113-190,
// libSGM under SfM/src/dense/cudasgm) by the definitions of include/msfm.h, "Dense stereo".  Integer arithmetic but for one
// binary32 product; tests/sgm_ref.cpp restates it sequentially and every plane here equals it byte for byte.
//
// msfm_sgm_execute   the pair into pinned staging (packed), one copy to the device, then on the context's stream, without a wait:
//   k_census         one lane per pixel and image, the 31 comparisons, 0 on the border
//   k_path_h         paths 0, 1.  A lane group of D / 8 lanes owns one row and one direction and walks x; a lane keeps 8 consecutive
//                    disparities' costs and, as a shift register across the group, the 8 right-census words they meet, so a step
//                    loads one new word.  The census words come in chunks of eight steps, the next chunk in flight.
//   k_path_vd        paths 2, 3 (vertical) and 4 .. 7 (oblique).  A lane group owns one column, or one diagonal by the column it has
//                    at the first row of the walk, and walks y; the groups of a workgroup are adjacent in x, and the D + groups - 1
//                    right-census words of the step are staged in LDS once, double buffered, one barrier per step.
//   k_wta            one workgroup per row walks it in tiles of 64 pixels: the eight volumes summed with 16-byte loads into a ring
//                    of T + D pixel columns of uint16 in LDS; the left winner of the tile's pixels and the right winner of the 64
//                    pixels whose last candidate column has just arrived, four lanes per pixel, top-2 by min / max.
//   k_median         3 x 3 median of both raw planes;  k_check  the consistency rule into the uint8 plane.
// Every path kernel writes a lane's 8 cost bytes as one store and a group's D bytes as one line.
// msfm_sgm_execute_rectified   the same seven launches (sgm_execute_dev) on the rectified planes of a msfm_rectifier (rectify.hip),
//                    where its kernel wrote them: no copy, no wait.
#include <memory>

#include "common.h"
#include "sgm_args.h"

struct msfm_sgm {
  msfm_ctx* ctx = nullptr;
  int w = 0, h = 0, D = 0, P1 = 0, P2 = 0;
  float uniqueness = 0;
  bool executed = false;
  DevBuf<uint8_t> img;         // [2][h][w]: left, right
  DevBuf<uint32_t> census;     // [2][h][w]
  DevBuf<uint8_t> vol[8];      // [h][w][D] each
  DevBuf<uint16_t> planes;     // [4][h][w]: raw left, raw right, median left, median right
  DevBuf<uint8_t> fin;         // [h][w]
  StageSlots stage;            // pinned staging of the packed pair
  size_t npx() const { return (size_t)w * h; }
  int64_t device_bytes() const { return (int64_t)(npx() * (2 + 8 + 8 * (size_t)D + 8 + 1)); }
};

namespace sgm {

struct Vols { uint8_t* p[8]; };

__global__ __launch_bounds__(256) void k_census(const uint8_t* __restrict__ img, int w, int h, uint32_t* __restrict__ out) {
  const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
  if (x >= w) return;
  const size_t plane = (size_t)blockIdx.z * w * h;
  const uint8_t* I = img + plane;
  uint32_t f = 0;
  if (x >= 4 && x < w - 4 && y >= 3 && y < h - 3) {
#pragma unroll
    for (int dy = -3; dy <= 0; dy++)
#pragma unroll
      for (int dx = -4; dx <= 4; dx++)
        if (dy < 0 || dx < 0) f = (f << 1) | (uint32_t)(I[(size_t)(y + dy) * w + x + dx] > I[(size_t)(y - dy) * w + x - dx]);
  }
  out[plane + (size_t)y * w + x] = f;
}

#define SGM_BIG (1 << 20)

// One step of the recurrence for the lane group of G lanes this lane is lane k of: L (the costs of q = p - r, 8 disparities from
// 8 k on) becomes the costs of p from its matching costs C; first: q is outside the image.  Every lane of the group calls it.
// -> the 8 new bytes, lowest disparity in the lowest byte.
template <int G>
__device__ __forceinline__ uint2 path_step(int (&L)[8], const int (&C)[8], bool first, int k, int P1, int P2) {
  int m = min(min(min(L[0], L[1]), min(L[2], L[3])), min(min(L[4], L[5]), min(L[6], L[7])));
#pragma unroll
  for (int s = 1; s < G; s <<= 1) m = min(m, __shfl_xor(m, s));   // (a xor below G stays inside the aligned group)
  int below = __shfl_up(L[7], 1, G), above = __shfl_down(L[0], 1, G);
  if (k == 0) below = SGM_BIG;        // disparity -1
  if (k == G - 1) above = SGM_BIG;    // disparity D
  int N[8];
#pragma unroll
  for (int j = 0; j < 8; j++) {
    const int b = j > 0 ? L[j - 1] : below, c = j < 7 ? L[j + 1] : above;
    const int best = min(min(L[j], min(b, c) + P1) - m, P2);
    N[j] = C[j] + (first ? 0 : best);
  }
#pragma unroll
  for (int j = 0; j < 8; j++) L[j] = N[j];
  return make_uint2((uint32_t)N[0] | ((uint32_t)N[1] << 8) | ((uint32_t)N[2] << 16) | ((uint32_t)N[3] << 24),
                    (uint32_t)N[4] | ((uint32_t)N[5] << 8) | ((uint32_t)N[6] << 16) | ((uint32_t)N[7] << 24));
}

// The walk of one row in direction DIR (+1: path 0 from x = 0 up, -1: path 1 from x = w - 1 down) by one lane group.
// R[j] is the right-census word of x - 8 k - j, 0 in front of the row.
template <int D, int DIR>
__device__ __forceinline__ void walk_row(const uint32_t* __restrict__ cl, const uint32_t* __restrict__ cr, int w, int k, int P1, int P2,
                                         uint8_t* __restrict__ out) {
  constexpr int G = D / SGM_LANE_DISP;
  int L[8];
  uint32_t R[8];
#pragma unroll
  for (int j = 0; j < 8; j++) {
    L[j] = 0;
    R[j] = 0;
    if (DIR < 0) {   // the words of the virtual column x = w; the one of lane 0, j = 0 leaves with the first shift
      const int i = w - 8 * k - j;
      if (i >= 0 && i < w) R[j] = cr[i];
    }
  }
  // a[i], b[i]: the left word of step i of a chunk of eight, and the right word that enters the register in it (DIR > 0: at
  // x into lane 0; DIR < 0: at x - (D - 1) into the last lane)
  uint32_t a[8], b[8], an[8], bn[8];
  auto load = [&](int x0, uint32_t (&pa)[8], uint32_t (&pb)[8]) {
#pragma unroll
    for (int i = 0; i < 8; i++) {
      const int x = x0 + DIR * i, xin = DIR > 0 ? x : x - (D - 1);
      pa[i] = (x >= 0 && x < w) ? cl[x] : 0u;
      pb[i] = (xin >= 0 && xin < w) ? cr[xin] : 0u;
    }
  };
  const int start = DIR > 0 ? 0 : w - 1;
  load(start, a, b);
  for (int s0 = 0; s0 < w; s0 += 8) {
    load(start + DIR * (s0 + 8), an, bn);
#pragma unroll
    for (int i = 0; i < 8; i++) {
      if (s0 + i < w) {   // (the same in every lane of the wave)
        const int x = start + DIR * (s0 + i);
        if (DIR > 0) {
          uint32_t in = (uint32_t)__shfl_up((int)R[7], 1, G);
          if (k == 0) in = b[i];
#pragma unroll
          for (int j = 7; j > 0; j--) R[j] = R[j - 1];
          R[0] = in;
        } else {
          uint32_t in = (uint32_t)__shfl_down((int)R[0], 1, G);
          if (k == G - 1) in = b[i];
#pragma unroll
          for (int j = 0; j < 7; j++) R[j] = R[j + 1];
          R[7] = in;
        }
        int C[8];
#pragma unroll
        for (int j = 0; j < 8; j++) C[j] = __popc(a[i] ^ R[j]);
        const uint2 v = path_step<G>(L, C, s0 + i == 0, k, P1, P2);
        *reinterpret_cast<uint2*>(out + (size_t)x * D + 8 * k) = v;
      }
    }
#pragma unroll
    for (int i = 0; i < 8; i++) { a[i] = an[i]; b[i] = bn[i]; }
  }
}

// paths 0 and 1: blockIdx.y is the path, a lane group is one row
template <int D>
__global__ __launch_bounds__(SGM_PATH_THREADS) void k_path_h(const uint32_t* __restrict__ cl, const uint32_t* __restrict__ cr, int w, int h, int P1,
                                                             int P2, Vols vols) {
  constexpr int G = D / SGM_LANE_DISP, NG = SGM_PATH_THREADS / G;
  const int k = threadIdx.x % G, y = blockIdx.x * NG + threadIdx.x / G;
  if (y >= h) return;   // (whole groups leave: no barrier in this kernel, and a shuffle reads inside its group)
  const size_t row = (size_t)y * w;
  if (blockIdx.y == 0) walk_row<D, 1>(cl + row, cr + row, w, k, P1, P2, vols.p[0] + row * D);
  else walk_row<D, -1>(cl + row, cr + row, w, k, P1, P2, vols.p[1] + row * D);
}

// paths 2 .. 7: blockIdx.y + path0 is the path, (dx, dy) its direction.  Step t of the walk is the row y = t (dy > 0) or h - 1 - t;
// the group with first-row column x0 is at x = x0 + dx t.  A workgroup's NG groups are adjacent in x0, so at a step they need the
// right-census words xb - (D - 1) .. xb + NG - 1 of one row (xb: the first group's x) and NG left words.
template <int D>
__global__ __launch_bounds__(SGM_PATH_THREADS) void k_path_vd(const uint32_t* __restrict__ cl, const uint32_t* __restrict__ cr, int w, int h, int P1,
                                                              int P2, int path0, Vols vols) {
  constexpr int G = D / SGM_LANE_DISP, NG = SGM_PATH_THREADS / G, SEG = D + NG - 1;
  constexpr int PAD = 32 / G;   // a lane's words lie 8 apart, a group's 32-word runs are shifted by PAD banks against each other
  static_assert(SEG + NG <= SGM_PATH_THREADS, "one staged word per lane");
  __shared__ uint32_t seg[2][SEG + PAD * (SEG / 32 + 1)];
  __shared__ uint32_t lft[2][NG];
  const int path = path0 + blockIdx.y;
  const int dx = path < 4 ? 0 : ((path == 4 || path == 7) ? 1 : -1), dy = (path == 2 || path == 4 || path == 5) ? 1 : -1;
  const int tid = threadIdx.x, g = tid / G, k = tid % G;
  const int xa = (dx > 0 ? -(h - 1) : 0) + blockIdx.x * NG;   // x0 of the workgroup's first group
  // the steps at which any group of the workgroup is inside the image
  int t_lo = 0, t_hi = h - 1;
  if (dx > 0) { t_lo = max(0, -(xa + NG - 1)); t_hi = min(h - 1, w - 1 - xa); }
  if (dx < 0) { t_lo = max(0, xa - w + 1); t_hi = min(h - 1, xa + NG - 1); }
  if (dx == 0 && xa >= w) return;
  if (t_lo > t_hi) return;
  uint8_t* const vol = vols.p[path];
  auto fetch = [&](int t) -> uint32_t {   // this lane's word of step t's staging
    const int y = dy > 0 ? t : h - 1 - t, xb = xa + dx * t;
    if (tid < SEG) {
      const int i = xb - (D - 1) + tid;
      return (i >= 0 && i < w) ? cr[(size_t)y * w + i] : 0u;
    }
    if (tid < SEG + NG) {
      const int i = xb + tid - SEG;
      return (i >= 0 && i < w) ? cl[(size_t)y * w + i] : 0u;
    }
    return 0u;
  };
  auto put = [&](int buf, uint32_t v) {
    if (tid < SEG) seg[buf][tid + PAD * (tid >> 5)] = v;
    else if (tid < SEG + NG) lft[buf][tid - SEG] = v;
  };
  put(0, fetch(t_lo));
  __syncthreads();
  int L[8];
#pragma unroll
  for (int j = 0; j < 8; j++) L[j] = 0;
  const int x0 = xa + g;
  for (int t = t_lo; t <= t_hi; t++) {
    const int cur = (t - t_lo) & 1;
    uint32_t next = 0;
    if (t < t_hi) next = fetch(t + 1);
    const int x = x0 + dx * t, y = dy > 0 ? t : h - 1 - t;
    const bool inside = x >= 0 && x < w;
    const bool first = t == 0 || x - dx < 0 || x - dx >= w;
    const uint32_t lw = lft[cur][g];
    int C[8];
#pragma unroll
    for (int j = 0; j < 8; j++) {
      const int i = g + (D - 1) - 8 * k - j;   // the word of x - d, d = 8 k + j, in the segment
      C[j] = __popc(lw ^ seg[cur][i + PAD * (i >> 5)]);
    }
    int Lk[8];
#pragma unroll
    for (int j = 0; j < 8; j++) Lk[j] = L[j];
    const uint2 v = path_step<G>(Lk, C, first, k, P1, P2);
    if (inside) {   // a group outside the image keeps its state untouched and writes nothing
#pragma unroll
      for (int j = 0; j < 8; j++) L[j] = Lk[j];
      *reinterpret_cast<uint2*>(vol + ((size_t)y * w + x) * D + 8 * k) = v;
    }
    put(cur ^ 1, next);
    __syncthreads();
  }
}

__device__ __forceinline__ void merge_top2(uint32_t& k0, uint32_t& k1, uint32_t o0, uint32_t o1) {
  const uint32_t hi = max(k0, o0);
  k0 = min(k0, o0);
  k1 = min(hi, min(k1, o1));
}

// One workgroup per row.  ring: the sums S(x, d) of the last T + D pixel columns, column x in slot x mod (T + D), D + 8 uint16 a slot.
template <int D>
__global__ __launch_bounds__(256) void k_wta(Vols vols, int w, float uniqueness, uint16_t* __restrict__ raw_left, uint16_t* __restrict__ raw_right) {
  constexpr int T = SGM_WTA_TILE, RP = T + D, STRIDE = D + 8, CH = D / 16, Q = D / 4;
  __shared__ __attribute__((aligned(16))) uint16_t ring[RP * STRIDE];
  const int y = blockIdx.x, tid = threadIdx.x;
  const size_t row = (size_t)y * w;
  const int tiles = (w - 1 + D + T - 1) / T;   // until the right winner of pixel w - 1 has been made
  for (int n = 0; n < tiles; n++) {
    const int xt = n * T;
    // the tile's sums: a lane takes 16 disparities of one pixel from each volume
    for (int c = tid; c < T * CH; c += 256) {
      const int x = xt + c / CH, d0 = 16 * (c % CH);
      if (x < w) {
        uint32_t even[4] = {0, 0, 0, 0}, odd[4] = {0, 0, 0, 0};   // two 16-bit sums a word: bytes 0, 2 and bytes 1, 3
#pragma unroll
        for (int r = 0; r < 8; r++) {
          const uint4 v = *reinterpret_cast<const uint4*>(vols.p[r] + (row + x) * D + d0);
          const uint32_t q[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
          for (int i = 0; i < 4; i++) { even[i] += q[i] & 0x00ff00ffu; odd[i] += (q[i] >> 8) & 0x00ff00ffu; }
        }
        uint32_t o[8];
#pragma unroll
        for (int i = 0; i < 4; i++) {
          o[2 * i] = (even[i] & 0xffffu) | (odd[i] << 16);
          o[2 * i + 1] = (even[i] >> 16) | (odd[i] & 0xffff0000u);
        }
        uint4* dst = reinterpret_cast<uint4*>(&ring[(x % RP) * STRIDE + d0]);
        dst[0] = make_uint4(o[0], o[1], o[2], o[3]);
        dst[1] = make_uint4(o[4], o[5], o[6], o[7]);
      }
    }
    __syncthreads();
    const int q = tid & 3;
    {   // left winner of the tile's pixels: four lanes a pixel, a quarter of the disparities each
      const int x = xt + (tid >> 2);
      uint32_t k0 = 0xffffffffu, k1 = 0xffffffffu;
      const uint16_t* s = &ring[(x % RP) * STRIDE + q * Q];
#pragma unroll
      for (int i = 0; i < Q; i += 8) {
        const uint4 v = *reinterpret_cast<const uint4*>(s + i);
        const uint32_t u[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int j = 0; j < 4; j++) {
          sgm_two_smallest(((u[j] & 0xffffu) << 16) | (uint32_t)(q * Q + i + 2 * j), k0, k1);
          sgm_two_smallest((u[j] & 0xffff0000u) | (uint32_t)(q * Q + i + 2 * j + 1), k0, k1);
        }
      }
#pragma unroll
      for (int sft = 1; sft < 4; sft <<= 1) merge_top2(k0, k1, (uint32_t)__shfl_xor((int)k0, sft), (uint32_t)__shfl_xor((int)k1, sft));
      if (q == 0 && x < w) raw_left[row + x] = sgm_decide(k0, k1, uniqueness);
    }
    {   // right winner of the pixels p whose last candidate column p + D - 1 lies in this tile (or behind the row's end)
      const int p = xt - D + 1 + (tid >> 2);
      uint32_t k0 = 0xffffffffu, k1 = 0xffffffffu;
      if (p >= 0 && p < w) {
        const int dmax = min(D - 1, w - 1 - p);
        for (int d = q * Q; d < (q + 1) * Q && d <= dmax; d++)
          sgm_two_smallest(((uint32_t)ring[((p + d) % RP) * STRIDE + d] << 16) | (uint32_t)d, k0, k1);
      }
#pragma unroll
      for (int sft = 1; sft < 4; sft <<= 1) merge_top2(k0, k1, (uint32_t)__shfl_xor((int)k0, sft), (uint32_t)__shfl_xor((int)k1, sft));
      if (q == 0 && p >= 0 && p < w) raw_right[row + p] = sgm_decide(k0, k1, uniqueness);
    }
    __syncthreads();   // the next tile's sums replace columns this step has read
  }
}

// blockIdx.z: 0 the left plane, 1 the right one; in [2][h][w] -> out [2][h][w]
__global__ __launch_bounds__(256) void k_median(const uint16_t* __restrict__ in, int w, int h, uint16_t* __restrict__ out) {
  const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
  if (x >= w) return;
  const size_t plane = (size_t)blockIdx.z * w * h;
  int v = 0;
  if (x >= 1 && x <= w - 2 && y >= 1 && y <= h - 2) {
    int p[9];
#pragma unroll
    for (int j = 0; j < 3; j++)
#pragma unroll
      for (int i = 0; i < 3; i++) p[3 * j + i] = in[plane + (size_t)(y + j - 1) * w + x + i - 1];
    v = sgm_median9(p);
  }
  out[plane + (size_t)y * w + x] = (uint16_t)v;
}

__global__ __launch_bounds__(256) void k_check(const uint8_t* __restrict__ left, const uint16_t* __restrict__ med_left,
                                               const uint16_t* __restrict__ med_right, int w, int h, uint8_t* __restrict__ out) {
  const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
  if (x >= w) return;
  const size_t i = (size_t)y * w + x;
  int d = med_left[i];
  if (x < 16 * (w / 16) && y < 16 * (h / 16)) {
    const int k = x - d;
    bool bad = left[i] == 0 || d <= 0;
    if (k >= 0 && k < w) {
      const int gap = (int)med_right[(size_t)y * w + k] - d;
      bad = bad || gap > 1 || gap < -1;
    }
    if (bad) d = 0;
  }
  out[i] = (uint8_t)d;
}

}  // namespace sgm

#define SG_TRY(e) HIP_TRY(ctx, (e))
// an allocation that fails is the refusal MSFM_E_NOMEM, and leaves no sticky error behind
#define SG_ALLOC(e)                                                                                                                \
  do {                                                                                                                             \
    if ((e) != hipSuccess) {                                                                                                       \
      (void)hipGetLastError();                                                                                                     \
      return msfm_set_error(ctx, MSFM_E_NOMEM, "%s: the planes of %d x %d pixels at %d disparities (%.1f GB) do not fit", who, width, \
                            height, disp_size, (double)P->device_bytes() * 1e-9);                                                  \
    }                                                                                                                              \
  } while (0)

MSFM_API int msfm_sgm_create(msfm_ctx* ctx, int width, int height, int disp_size, int p1, int p2, float uniqueness, msfm_sgm** out) {
  const char* who = "msfm_sgm_create";
  if (!ctx) return MSFM_E_INVAL;
  if (!out) return msfm_set_error(ctx, MSFM_E_INVAL, "%s: null argument", who);
  *out = nullptr;
  const std::string bad = sgm_check_create(width, height, disp_size, p1, p2, uniqueness);
  if (!bad.empty()) return msfm_set_error(ctx, MSFM_E_INVAL, "%s: %s", who, bad.c_str());
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  Child<msfm_sgm> P = child_new<msfm_sgm>(ctx);
  P->w = width; P->h = height; P->D = disp_size; P->P1 = p1; P->P2 = p2; P->uniqueness = uniqueness;
  const size_t npx = P->npx();
  for (int r = 0; r < 8; r++) SG_ALLOC(P->vol[r].alloc(npx * disp_size));
  SG_ALLOC(P->img.alloc(2 * npx));
  SG_ALLOC(P->census.alloc(2 * npx));
  SG_ALLOC(P->planes.alloc(4 * npx));
  SG_ALLOC(P->fin.alloc(npx));
  SG_ALLOC(P->stage.create(2 * npx));
  *out = P.release();
  return MSFM_OK;
}

// The chain on a pair that is on the device: img [2][h][w] packed, left then right, of the object's size.  Seven launches on the
// context's stream, no wait, no copy.  k_census and k_check are the two readers of img.
static int sgm_execute_dev(msfm_sgm* P, const uint8_t* img) {
  using namespace sgm;
  msfm_ctx* ctx = P->ctx;
  const int w = P->w, h = P->h, D = P->D;
  hipStream_t st = ctx->stream;
  const size_t npx = P->npx();
  const uint32_t* cl = P->census.p;
  const uint32_t* cr = P->census.p + npx;
  Vols vols;
  for (int r = 0; r < 8; r++) vols.p[r] = P->vol[r].p;
  const dim3 px(cdiv(w, 256), h);
  const int G = D / SGM_LANE_DISP, NG = SGM_PATH_THREADS / G;
  {
    KTimer t(ctx, "sgm_census");
    hipLaunchKernelGGL(k_census, dim3(px.x, px.y, 2), dim3(256), 0, st, img, w, h, P->census.p);
  }
  {
    KTimer t(ctx, "sgm_path_h");
    const dim3 g(cdiv(h, NG), 2);
    if (D == 128) hipLaunchKernelGGL(k_path_h<128>, g, dim3(SGM_PATH_THREADS), 0, st, cl, cr, w, h, P->P1, P->P2, vols);
    else hipLaunchKernelGGL(k_path_h<64>, g, dim3(SGM_PATH_THREADS), 0, st, cl, cr, w, h, P->P1, P->P2, vols);
  }
  {
    KTimer t(ctx, "sgm_path_v");
    const dim3 g(cdiv(w, NG), 2);
    if (D == 128) hipLaunchKernelGGL(k_path_vd<128>, g, dim3(SGM_PATH_THREADS), 0, st, cl, cr, w, h, P->P1, P->P2, 2, vols);
    else hipLaunchKernelGGL(k_path_vd<64>, g, dim3(SGM_PATH_THREADS), 0, st, cl, cr, w, h, P->P1, P->P2, 2, vols);
  }
  {
    KTimer t(ctx, "sgm_path_d");
    const dim3 g(cdiv(w + h - 1, NG), 4);
    if (D == 128) hipLaunchKernelGGL(k_path_vd<128>, g, dim3(SGM_PATH_THREADS), 0, st, cl, cr, w, h, P->P1, P->P2, 4, vols);
    else hipLaunchKernelGGL(k_path_vd<64>, g, dim3(SGM_PATH_THREADS), 0, st, cl, cr, w, h, P->P1, P->P2, 4, vols);
  }
  uint16_t* const raw = P->planes.p;
  uint16_t* const med = P->planes.p + 2 * npx;
  {
    KTimer t(ctx, "sgm_wta");
    if (D == 128) hipLaunchKernelGGL(k_wta<128>, dim3(h), dim3(256), 0, st, vols, w, P->uniqueness, raw, raw + npx);
    else hipLaunchKernelGGL(k_wta<64>, dim3(h), dim3(256), 0, st, vols, w, P->uniqueness, raw, raw + npx);
  }
  {
    KTimer t(ctx, "sgm_median");
    hipLaunchKernelGGL(k_median, dim3(px.x, px.y, 2), dim3(256), 0, st, raw, w, h, med);
  }
  {
    KTimer t(ctx, "sgm_check");
    hipLaunchKernelGGL(k_check, px, dim3(256), 0, st, img, med, med + npx, w, h, P->fin.p);
  }
  SG_TRY(hipGetLastError());
  P->executed = true;
  return MSFM_OK;
}
#define SGM_CHAIN_LAUNCHES 7

MSFM_API int msfm_sgm_execute(msfm_sgm* P, const uint8_t* left, int left_stride, const uint8_t* right, int right_stride, int64_t* stats) {
  const char* who = "msfm_sgm_execute";
  if (!P) return MSFM_E_INVAL;
  msfm_ctx* ctx = P->ctx;
  const int w = P->w, h = P->h;
  const std::string bad = sgm_check_execute(left, left_stride, right, right_stride, w);
  if (!bad.empty()) return msfm_set_error(ctx, MSFM_E_INVAL, "%s: %s", who, bad.c_str());
  SG_TRY(hipSetDevice(ctx->device));
  int64_t waits = 0;
  const size_t npx = P->npx();
  uint8_t* stage = nullptr;
  SG_TRY(P->stage.take(&stage, &waits));
  for (int y = 0; y < h; y++) {
    memcpy(stage + (size_t)y * w, left + (size_t)y * left_stride, (size_t)w);
    memcpy(stage + npx + (size_t)y * w, right + (size_t)y * right_stride, (size_t)w);
  }
  SG_TRY(P->stage.send(P->img.p, 2 * npx, ctx->stream));
  MSFM_TRY(sgm_execute_dev(P, P->img.p));
  if (stats) {
    stats[SGM_ST_WAITS] = waits;
    stats[SGM_ST_H2D] = (int64_t)(2 * npx);
    stats[SGM_ST_LAUNCHES] = SGM_CHAIN_LAUNCHES;
  }
  return MSFM_OK;
}

MSFM_API int msfm_sgm_execute_rectified(msfm_sgm* P, const msfm_rectifier* rect, int64_t* stats) {
  const char* who = "msfm_sgm_execute_rectified";
  if (!P) return MSFM_E_INVAL;
  msfm_ctx* ctx = P->ctx;
  if (!rect) return msfm_set_error(ctx, MSFM_E_INVAL, "%s: null argument", who);
  msfm_ctx* rctx = nullptr;
  int rw = 0, rh = 0;
  const uint8_t* planes = rectifier_planes(rect, &rctx, &rw, &rh);
  if (rctx != ctx) return msfm_set_error(ctx, MSFM_E_INVAL, "%s: the rectifier belongs to another context", who);
  if (rw != P->w || rh != P->h) return msfm_set_error(ctx, MSFM_E_INVAL, "%s: a rectifier of %d x %d for an object of %d x %d", who, rw, rh, P->w, P->h);
  if (!planes) return msfm_set_error(ctx, MSFM_E_INVAL, "%s: the rectifier has not rectified anything yet", who);
  SG_TRY(hipSetDevice(ctx->device));
  MSFM_TRY(sgm_execute_dev(P, planes));
  if (stats) {
    stats[SGM_ST_WAITS] = 0;
    stats[SGM_ST_H2D] = 0;
    stats[SGM_ST_LAUNCHES] = SGM_CHAIN_LAUNCHES;
  }
  return MSFM_OK;
}

MSFM_API int msfm_sgm_fetch(const msfm_sgm* P, int kind, int index, void* out) {
  const char* who = "msfm_sgm_fetch";
  if (!P) return MSFM_E_INVAL;
  msfm_ctx* ctx = P->ctx;
  if (!out) return msfm_set_error(ctx, MSFM_E_INVAL, "%s: null argument", who);
  const int item = sgm_fetch_item(kind, P->D);
  if (!item) return msfm_set_error(ctx, MSFM_E_INVAL, "%s: kind %d outside [0, %d)", who, kind, SGM_FETCH_KINDS);
  if (index < 0 || index >= (kind == 2 ? 8 : 1)) return msfm_set_error(ctx, MSFM_E_INVAL, "%s: index %d outside the range of kind %d", who, index, kind);
  if (!P->executed) return msfm_set_error(ctx, MSFM_E_INVAL, "%s: nothing has been executed yet", who);
  const size_t npx = P->npx();
  const void* src = nullptr;
  switch (kind) {
    case 0: case 1: src = P->census.p + (size_t)kind * npx; break;
    case 2: src = P->vol[index].p; break;
    case 7: src = P->fin.p; break;
    default: src = P->planes.p + (size_t)(kind - 3) * npx; break;
  }
  SG_TRY(hipSetDevice(ctx->device));
  SG_TRY(hipMemcpyAsync(out, src, npx * (size_t)item, hipMemcpyDeviceToHost, ctx->stream));
  SG_TRY(hipStreamSynchronize(ctx->stream));
  return MSFM_OK;
}

MSFM_API int msfm_sgm_depth(const msfm_sgm* P, double baseline, double focal, uint8_t* depth_out) {
  const char* who = "msfm_sgm_depth";
  if (!P) return MSFM_E_INVAL;
  msfm_ctx* ctx = P->ctx;
  if (!depth_out) return msfm_set_error(ctx, MSFM_E_INVAL, "%s: null argument", who);
  if (!std::isfinite(baseline) || !std::isfinite(focal)) return msfm_set_error(ctx, MSFM_E_INVAL, "%s: baseline or focal is not finite", who);
  if (!P->executed) return msfm_set_error(ctx, MSFM_E_INVAL, "%s: nothing has been executed yet", who);
  // the final plane comes to the host anyway: the 128-entry table is applied to it here, in place
  uint8_t table[128];
  sgm_depth_table(baseline, focal, table);
  const size_t npx = P->npx();
  SG_TRY(hipSetDevice(ctx->device));
  SG_TRY(hipMemcpyAsync(depth_out, P->fin.p, npx, hipMemcpyDeviceToHost, ctx->stream));
  SG_TRY(hipStreamSynchronize(ctx->stream));
  for (size_t i = 0; i < npx; i++) depth_out[i] = table[depth_out[i] & 127];
  return MSFM_OK;
}

MSFM_API int msfm_sgm_size(const msfm_sgm* P, int* width, int* height, int* disp_size, int64_t* device_bytes) {
  if (!P) return MSFM_E_INVAL;
  if (width) *width = P->w;
  if (height) *height = P->h;
  if (disp_size) *disp_size = P->D;
  if (device_bytes) *device_bytes = P->device_bytes();
  return MSFM_OK;
}

MSFM_API void msfm_sgm_destroy(msfm_sgm* P) { msfm_child_destroy(P); }
