// Stereo rectification on the device: DenseReconstruction::EpipolarRectification (SfM/src/dense_reconstruction.cc:299-331) by the
// definitions of include/msfm.h, "Stereo rectification".  The geometry (cv::stereoRectify restated) is a few hundred binary64
// operations on the host, rectify_args.h; maps (cv::initUndistortRectifyMap) and warp (cv::remap, INTER_LINEAR, as its 5-bit
// fixed-point integers) are one kernel.  tests/rectify_ref.cpp restates all three sequentially and every plane here equals it byte
// for byte.
//
// msfm_rectifier_rectify   geometry and parameter block on the host; the block and the packed pair into pinned staging, one copy
//                          to the device; then on the context's stream, without a wait:
//   k_remap                one lane per output pixel, blockIdx.z the camera: the map in unfused binary64 straight from (column,
//                          row) - no pixel depends on its neighbour -, four source bytes gathered from global memory (a pair's
//                          planes are a few megabytes and stay in L2), the integer blend, one byte stored; with MAPS also the two
//                          map values.  Bytes are stored because a packed row of odd width starts unaligned; a wave's 64 of them
//                          are one 64-byte line, and the launch moves 4 w h bytes beside the 16 w h D of the chain behind it.
// msfm_sgm_execute_rectified (sgm.hip) reads the rectified planes where k_remap wrote them.
#include "common.h"
#include "rectify_args.h"

struct msfm_rectifier {
  msfm_ctx* ctx = nullptr;
  int w = 0, h = 0;
  bool rectified = false, maps = false;   // maps: the last rectify wrote the map planes
  DevBuf<uint8_t> src;    // the parameter block (RECT_PARAM_BYTES), then [2][h][w]: left, right as they came
  DevBuf<uint8_t> dst;    // [2][h][w]: left, right rectified
  DevBuf<float> map;      // [4][h][w]: mapx, mapy of left, then of right
  StageSlots stage;       // pinned staging of src
  size_t npx() const { return (size_t)w * h; }
  int64_t device_bytes() const { return (int64_t)(RECT_PARAM_BYTES + npx() * (2 + 2 + 4 * sizeof(float))); }
};

const uint8_t* rectifier_planes(const msfm_rectifier* R, msfm_ctx** ctx, int* width, int* height) {
  *ctx = R->ctx;
  *width = R->w;
  *height = R->h;
  return R->rectified ? R->dst.p : nullptr;
}

namespace rectify {

// (rectify_args.h has switched contraction off for this file: the map is products and sums rounded one by one, and the division is
// the correctly rounded one, so the host's restatement gets the same bits)
template <bool MAPS>
__global__ __launch_bounds__(256) void k_remap(const RectParams* __restrict__ par, const uint8_t* __restrict__ src, int w, int h,
                                               uint8_t* __restrict__ dst, float* __restrict__ map) {
  const int j = blockIdx.x * 256 + threadIdx.x, i = blockIdx.y, cam = blockIdx.z;
  if (j >= w) return;
  const RectCamera& c = par->cam[cam];   // (uniform: scalar loads)
  const double x = (double)j, y = (double)i;
  const double X = (c.iR[0] * x + c.iR[1] * y) + c.iR[2];
  const double Y = (c.iR[3] * x + c.iR[4] * y) + c.iR[5];
  const double W = (c.iR[6] * x + c.iR[7] * y) + c.iR[8];
  const double wi = 1.0 / W;
  const float mapx = (float)(c.fx * (X * wi) + c.cx), mapy = (float)(c.fy * (Y * wi) + c.cy);
  const size_t npx = (size_t)w * h, at = (size_t)i * w + j;
  if (MAPS) {
    map[(size_t)(2 * cam) * npx + at] = mapx;
    map[(size_t)(2 * cam + 1) * npx + at] = mapy;
  }
  const float px = mapx * 32.0f, py = mapy * 32.0f;
  uint8_t v = 0;
  // (a NaN fails the comparison; below 2^30 the rounded value and the tap beside it are ints, and every tap is checked in rect_blend)
  if (fabsf(px) < 0x1p30f && fabsf(py) < 0x1p30f) v = rect_blend(src + (size_t)cam * npx, w, h, __float2int_rn(px), __float2int_rn(py));
  dst[(size_t)cam * npx + at] = v;
}

}  // namespace rectify

#define RC_TRY(e) HIP_TRY(ctx, (e))
#define RC_ALLOC(e)                                                                                                                \
  do {                                                                                                                             \
    if ((e) != hipSuccess) {                                                                                                       \
      (void)hipGetLastError();                                                                                                     \
      return msfm_set_error(ctx, MSFM_E_NOMEM, "%s: the planes of %d x %d pixels (%.1f MB) do not fit", who, width, height,        \
                            (double)P->device_bytes() * 1e-6);                                                                     \
    }                                                                                                                              \
  } while (0)

MSFM_API int msfm_stereo_rectify(const double* K1, const double* R1, const double* t1, const double* K2, const double* R2, const double* t2,
                                 int width, int height, double* R1_out, double* R2_out, double* P1_out, double* P2_out, double* Q_out,
                                 int* idx_out) {
  RectGeometry g;
  if (!rect_geometry(K1, R1, t1, K2, R2, t2, width, height, g).empty()) return MSFM_E_INVAL;
  if (R1_out) memcpy(R1_out, g.R1, sizeof g.R1);
  if (R2_out) memcpy(R2_out, g.R2, sizeof g.R2);
  if (P1_out) memcpy(P1_out, g.P1, sizeof g.P1);
  if (P2_out) memcpy(P2_out, g.P2, sizeof g.P2);
  if (Q_out) memcpy(Q_out, g.Q, sizeof g.Q);
  if (idx_out) *idx_out = g.idx;
  return MSFM_OK;
}

MSFM_API int msfm_rectifier_create(msfm_ctx* ctx, int width, int height, msfm_rectifier** out) {
  const char* who = "msfm_rectifier_create";
  if (!ctx) return MSFM_E_INVAL;
  if (!out) return msfm_set_error(ctx, MSFM_E_INVAL, "%s: null argument", who);
  *out = nullptr;
  const std::string bad = rect_check_size(width, height);
  if (!bad.empty()) return msfm_set_error(ctx, MSFM_E_INVAL, "%s: %s", who, bad.c_str());
  RC_TRY(hipSetDevice(ctx->device));
  Child<msfm_rectifier> P = child_new<msfm_rectifier>(ctx);
  P->w = width; P->h = height;
  const size_t npx = P->npx();
  RC_ALLOC(P->src.alloc(RECT_PARAM_BYTES + 2 * npx));
  RC_ALLOC(P->dst.alloc(2 * npx));
  RC_ALLOC(P->map.alloc(4 * npx));
  RC_ALLOC(P->stage.create(RECT_PARAM_BYTES + 2 * npx));
  *out = P.release();
  return MSFM_OK;
}

MSFM_API int msfm_rectifier_rectify(msfm_rectifier* P, const uint8_t* left, int left_stride, const uint8_t* right, int right_stride,
                                    const double* K1, const double* R1, const double* t1, const double* K2, const double* R2,
                                    const double* t2, int keep_maps, double* R1_out, double* R2_out, double* P1_out, double* P2_out,
                                    int64_t* stats) {
  using namespace rectify;
  const char* who = "msfm_rectifier_rectify";
  if (!P) return MSFM_E_INVAL;
  msfm_ctx* ctx = P->ctx;
  const int w = P->w, h = P->h;
  std::string bad = rect_check_pair(left, left_stride, right, right_stride, w);
  if (!bad.empty()) return msfm_set_error(ctx, MSFM_E_INVAL, "%s: %s", who, bad.c_str());
  RectGeometry g;
  bad = rect_geometry(K1, R1, t1, K2, R2, t2, w, h, g);
  if (!bad.empty()) return msfm_set_error(ctx, MSFM_E_INVAL, "%s: %s", who, bad.c_str());
  RC_TRY(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  int64_t waits = 0;
  const size_t npx = P->npx(), bytes = RECT_PARAM_BYTES + 2 * npx;
  uint8_t* stage = nullptr;
  RC_TRY(P->stage.take(&stage, &waits));
  RectParams par;
  rect_params(g, K1, K2, par);
  memcpy(stage, &par, sizeof par);
  uint8_t* const pair = stage + RECT_PARAM_BYTES;
  for (int y = 0; y < h; y++) {
    memcpy(pair + (size_t)y * w, left + (size_t)y * left_stride, (size_t)w);
    memcpy(pair + npx + (size_t)y * w, right + (size_t)y * right_stride, (size_t)w);
  }
  RC_TRY(P->stage.send(P->src.p, bytes, st));
  {
    KTimer t(ctx, "rectify_remap");
    const dim3 grid(cdiv(w, 256), h, 2);
    const RectParams* dpar = reinterpret_cast<const RectParams*>(P->src.p);   // (a pool block: aligned far beyond 8 bytes)
    const uint8_t* dsrc = P->src.p + RECT_PARAM_BYTES;
    if (keep_maps) hipLaunchKernelGGL(k_remap<true>, grid, dim3(256), 0, st, dpar, dsrc, w, h, P->dst.p, P->map.p);
    else hipLaunchKernelGGL(k_remap<false>, grid, dim3(256), 0, st, dpar, dsrc, w, h, P->dst.p, P->map.p);
  }
  RC_TRY(hipGetLastError());
  P->rectified = true;
  P->maps = keep_maps != 0;
  if (R1_out) memcpy(R1_out, g.R1, sizeof g.R1);
  if (R2_out) memcpy(R2_out, g.R2, sizeof g.R2);
  if (P1_out) memcpy(P1_out, g.P1, sizeof g.P1);
  if (P2_out) memcpy(P2_out, g.P2, sizeof g.P2);
  if (stats) {
    stats[RECT_ST_WAITS] = waits;
    stats[RECT_ST_H2D] = (int64_t)bytes;
    stats[RECT_ST_LAUNCHES] = 1;
  }
  return MSFM_OK;
}

MSFM_API int msfm_rectifier_fetch(const msfm_rectifier* P, int kind, void* out) {
  const char* who = "msfm_rectifier_fetch";
  if (!P) return MSFM_E_INVAL;
  msfm_ctx* ctx = P->ctx;
  if (!out) return msfm_set_error(ctx, MSFM_E_INVAL, "%s: null argument", who);
  const int item = rect_fetch_item(kind);
  if (!item) return msfm_set_error(ctx, MSFM_E_INVAL, "%s: kind %d outside [0, %d)", who, kind, RECT_FETCH_KINDS);
  if (!P->rectified) return msfm_set_error(ctx, MSFM_E_INVAL, "%s: nothing has been rectified yet", who);
  if (kind >= 2 && !P->maps) return msfm_set_error(ctx, MSFM_E_INVAL, "%s: the last rectify kept no maps", who);
  const size_t npx = P->npx();
  const void* src = kind < 2 ? (const void*)(P->dst.p + (size_t)kind * npx) : (const void*)(P->map.p + (size_t)(kind - 2) * npx);
  RC_TRY(hipSetDevice(ctx->device));
  RC_TRY(hipMemcpyAsync(out, src, npx * (size_t)item, hipMemcpyDeviceToHost, ctx->stream));
  RC_TRY(hipStreamSynchronize(ctx->stream));
  return MSFM_OK;
}

MSFM_API int msfm_rectifier_size(const msfm_rectifier* P, int* width, int* height, int64_t* device_bytes) {
  if (!P) return MSFM_E_INVAL;
  if (width) *width = P->w;
  if (height) *height = P->h;
  if (device_bytes) *device_bytes = P->device_bytes();
  return MSFM_OK;
}

MSFM_API void msfm_rectifier_destroy(msfm_rectifier* P) { msfm_child_destroy(P); }
