// Runs of equal keys in a sorted array, on the device: group heads by flag, an exclusive scan (prim_scan_excl), a scatter of the heads.
// pairsel.hip (the groups of an image's words, the bins of the inverted file) and words.hip (the bags of words) include it;
// the kernels are static, so each unit carries its own copy.
#pragma once
#include "prim_device.h"

namespace runs {

typedef unsigned long long u64;

// flag[e] = 1 where (key >> shift) differs from its predecessor's, e < cnt; flag[cnt] = 0 closes the scan
static __global__ __launch_bounds__(256) void k_heads(int cnt, const u64* __restrict__ key, int shift, int* __restrict__ flag) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e > cnt) return;
  flag[e] = (e < cnt && (e == 0 || (key[e] >> shift) != (key[e - 1] >> shift))) ? 1 : 0;
}

// start[g] = first element of run g; start[G] = cnt, G = pos[cnt]
static __global__ __launch_bounds__(256) void k_put_heads(int cnt, const int* __restrict__ flag, const int* __restrict__ pos, int* __restrict__ start) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e > cnt) return;
  if (e == cnt) start[pos[cnt]] = cnt;
  else if (flag[e]) start[pos[e]] = e;
}

// map_off[i] = entries of images below i, tab_img [T] ascending
static __global__ __launch_bounds__(256) void k_map_off(int n, int T, const int* __restrict__ tab_img, int* __restrict__ map_off) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i > n) return;
  int lo = 0, hi = T;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (tab_img[mid] < i) lo = mid + 1; else hi = mid;
  }
  map_off[i] = lo;
}

}  // namespace runs
