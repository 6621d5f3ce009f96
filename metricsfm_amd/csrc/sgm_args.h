// What sgm.hip does without a device: the argument checks, the launch constants the tests derive their shapes from, and the three
// small rules that host and device share word for word (the winner's decision, the median of nine, the depth table).  Plain C++.
// A check returns an empty string or the refusal's text.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <string>

#if defined(__HIPCC__)
#define SGM_HD __host__ __device__
#else
#define SGM_HD
#endif

#define SGM_MAX_SIDE 16384
#define SGM_MAX_P2 224          // 31 + P2 must fit a byte
#define SGM_LANE_DISP 8         // consecutive disparities a lane holds in the path kernels: a lane group is D / 8 lanes
#define SGM_PATH_THREADS 256    // lanes per workgroup of the path kernels: 256 / (D / 8) lane groups, 16 at D = 128, 32 at D = 64
#define SGM_WTA_TILE 64         // pixels a workgroup of the winner kernel sums per step of its walk along a row
#define SGM_STATS 3             // = MSFM_SGM_STATS
#define SGM_ST_WAITS 0
#define SGM_ST_H2D 1
#define SGM_ST_LAUNCHES 2
#define SGM_FETCH_KINDS 8

static inline std::string sgm_fmt(const char* fmt, long a = 0, long b = 0, long c = 0) {
  char buf[256];
  snprintf(buf, sizeof buf, fmt, a, b, c);
  return buf;
}

static inline std::string sgm_check_create(int width, int height, int disp_size, int p1, int p2, float uniqueness) {
  if (disp_size != 64 && disp_size != 128) return sgm_fmt("disp_size = %ld is neither 64 nor 128", disp_size);
  if (width < disp_size || width > SGM_MAX_SIDE) return sgm_fmt("width = %ld outside [disp_size = %ld, %ld]", width, disp_size, SGM_MAX_SIDE);
  if (height < 1 || height > SGM_MAX_SIDE) return sgm_fmt("height = %ld outside [1, %ld]", height, SGM_MAX_SIDE);
  if (p1 < 0 || p2 < 0) return sgm_fmt("P1 = %ld, P2 = %ld: a negative penalty", p1, p2);
  if (p2 > SGM_MAX_P2) return sgm_fmt("P2 = %ld above %ld: a path cost would not fit a byte", p2, SGM_MAX_P2);
  if (p1 > p2) return sgm_fmt("P1 = %ld above P2 = %ld", p1, p2);
  if (!(uniqueness >= 0.0f && uniqueness <= 1.0f)) return "uniqueness is not a number of [0, 1]";   // (a NaN fails the comparison)
  return "";
}

static inline std::string sgm_check_execute(const void* left, int left_stride, const void* right, int right_stride, int width) {
  if (!left || !right) return "null argument";
  if (left_stride < width || right_stride < width) return sgm_fmt("stride = %ld below width = %ld", left_stride < width ? left_stride : right_stride, width);
  return "";
}

// the plane a fetch kind names: bytes per pixel (kind 2 counts disp_size of them), 0 for a kind outside the range
static inline int sgm_fetch_item(int kind, int disp_size) {
  if (kind == 0 || kind == 1) return 4;
  if (kind == 2) return disp_size;
  if (kind >= 3 && kind <= 6) return 2;
  return kind == 7 ? 1 : 0;
}

// Keeps the two smallest of the keys it has seen (all keys of a pixel differ: they carry their disparity).
SGM_HD static inline void sgm_two_smallest(uint32_t key, uint32_t& k0, uint32_t& k1) {
  const uint32_t hi = key > k0 ? key : k0;
  k0 = key < k0 ? key : k0;
  k1 = hi < k1 ? hi : k1;
}

// The winner's rule on the two smallest keys (cost << 16 | disparity).
SGM_HD static inline uint16_t sgm_decide(uint32_t k0, uint32_t k1, float uniqueness) {
  const int c0 = (int)(k0 >> 16), d0 = (int)(k0 & 0xffffu), c1 = (int)(k1 >> 16), d1 = (int)(k1 & 0xffffu);
  if ((float)c1 * uniqueness >= (float)c0) return (uint16_t)d0;
  const int gap = d1 > d0 ? d1 - d0 : d0 - d1;
  return gap <= 1 ? (uint16_t)d0 : (uint16_t)0;
}

// The median of nine by the 19 exchanges of the classic network; p is left partly sorted.
SGM_HD static inline int sgm_median9(int (&p)[9]) {
#define SGM_SORT2(a, b) { const int lo_ = p[a] < p[b] ? p[a] : p[b]; p[b] = p[a] < p[b] ? p[b] : p[a]; p[a] = lo_; }
  SGM_SORT2(1, 2) SGM_SORT2(4, 5) SGM_SORT2(7, 8) SGM_SORT2(0, 1) SGM_SORT2(3, 4) SGM_SORT2(6, 7) SGM_SORT2(1, 2) SGM_SORT2(4, 5) SGM_SORT2(7, 8)
  SGM_SORT2(0, 3) SGM_SORT2(5, 8) SGM_SORT2(4, 7) SGM_SORT2(3, 6) SGM_SORT2(1, 4) SGM_SORT2(2, 5) SGM_SORT2(4, 7) SGM_SORT2(4, 2) SGM_SORT2(6, 4)
  SGM_SORT2(4, 2)
#undef SGM_SORT2
  return p[4];
}

// depth of every disparity 0 .. 127 (dense_reconstruction.cc:160-181): binary64, truncated, 0 outside [0, 255] and for disparity 0
static inline void sgm_depth_table(double baseline, double focal, uint8_t table[128]) {
  table[0] = 0;
  for (int d = 1; d < 128; d++) {
    const double t = ((200.0 * baseline) * focal) / (double)d;
    table[d] = (t > 255 || t < 0) ? 0 : (uint8_t)t;
  }
}
