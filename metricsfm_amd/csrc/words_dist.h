// The vocabulary tree's distance on the device, stated once: the descent (words.hip) and the training (voctrain.hip) evaluate the
// same eight partial sums in the same order, so a trained tree's centres and the descent through them agree on every comparison.
// Eight lanes share a feature; lane j holds its elements j, j + 8, ... (f[0..15]) and reads a node's run j of the relayed layout
// [node][8][16] with four 16-byte loads.
#pragma once
#include "common.h"

// s + (a - b)^2 in three roundings
__device__ static inline float sq_step(float s, float a, float b) {
#pragma clang fp contract(off)
  const float d = a - b;
  const float q = d * d;
  return s + q;
}

__device__ static inline float add8(float s) {   // the sum over a group of eight lanes: ((s0+s1)+(s2+s3))+((s4+s5)+(s6+s7)), in all of them
  s = s + __shfl_xor(s, 1, 8);
  s = s + __shfl_xor(s, 2, 8);
  s = s + __shfl_xor(s, 4, 8);
  return s;
}

// lane j's partial sum of |f - node|^2: the node's run j, 16 steps in ascending element order
__device__ static inline float part16(const float* f, const float* run) {
  const float4* p = reinterpret_cast<const float4*>(run);
  const float4 a = p[0], b = p[1], c = p[2], d = p[3];
  float s = 0.f;
  s = sq_step(s, f[0], a.x); s = sq_step(s, f[1], a.y); s = sq_step(s, f[2], a.z); s = sq_step(s, f[3], a.w);
  s = sq_step(s, f[4], b.x); s = sq_step(s, f[5], b.y); s = sq_step(s, f[6], b.z); s = sq_step(s, f[7], b.w);
  s = sq_step(s, f[8], c.x); s = sq_step(s, f[9], c.y); s = sq_step(s, f[10], c.z); s = sq_step(s, f[11], c.w);
  s = sq_step(s, f[12], d.x); s = sq_step(s, f[13], d.y); s = sq_step(s, f[14], d.z); s = sq_step(s, f[15], d.w);
  return s;
}

// position of element i of a descriptor in the relayed layout: run i % 8, slot i / 8
__host__ __device__ static inline int relay_pos(int i) { return (i & 7) * 16 + (i >> 3); }
