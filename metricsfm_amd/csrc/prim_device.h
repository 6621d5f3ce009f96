// rocPRIM behind one scratch type (PrimTmp, common.h): the library's scans and radix sorts, each a size query, PrimTmp::fit and
// the call.  No other file of the library names rocPRIM.
#pragma once
#include "common.h"   // (first: rocPRIM's headers expect <cstring>)

#include <rocprim/rocprim.hpp>

// call(temporary, bytes) is one rocPRIM call with everything but its first two arguments bound: the size query, fit, the call
template <class Call>
static inline hipError_t prim_run(PrimTmp& tmp, Call&& call) {
  size_t bytes = 0;
  hipError_t e = call((void*)nullptr, bytes);
  if (e == hipSuccess) e = tmp.fit(bytes);
  return e != hipSuccess ? e : call((void*)tmp.cur.p, bytes);
}

// out[i] = in[0] + .. + in[i - 1]; in == out is allowed
template <typename T>
static inline hipError_t prim_scan_excl(PrimTmp& tmp, const T* in, T* out, size_t n, hipStream_t s) {
  if (n == 0) return hipSuccess;
  return prim_run(tmp, [&](void* t, size_t& b) { return rocprim::exclusive_scan(t, b, in, out, T(0), n, rocprim::plus<T>(), s); });
}
// out[i] = in[0] + .. + in[i]
template <typename T>
static inline hipError_t prim_scan_incl(PrimTmp& tmp, const T* in, T* out, size_t n, hipStream_t s) {
  if (n == 0) return hipSuccess;
  return prim_run(tmp, [&](void* t, size_t& b) { return rocprim::inclusive_scan(t, b, in, out, n, rocprim::plus<T>(), s); });
}

// Ascending radix sorts on bits [begin_bit, end_bit) of the key; stable: equal keys keep the order of the input.
template <typename K, typename V>
static inline hipError_t prim_sort_pairs(PrimTmp& tmp, const K* kin, K* kout, const V* vin, V* vout, size_t n, unsigned begin_bit, unsigned end_bit,
                                         hipStream_t s) {
  if (n == 0) return hipSuccess;
  return prim_run(tmp, [&](void* t, size_t& b) { return rocprim::radix_sort_pairs(t, b, kin, kout, vin, vout, n, begin_bit, end_bit, s); });
}
template <typename K>
static inline hipError_t prim_sort_keys(PrimTmp& tmp, const K* kin, K* kout, size_t n, unsigned begin_bit, unsigned end_bit, hipStream_t s) {
  if (n == 0) return hipSuccess;
  return prim_run(tmp, [&](void* t, size_t& b) { return rocprim::radix_sort_keys(t, b, kin, kout, n, begin_bit, end_bit, s); });
}

// The same inside each of `segments` segments [begin_offsets[i], end_offsets[i]) of the n elements (offsets on the device).
template <typename K>
static inline hipError_t prim_seg_sort_keys(PrimTmp& tmp, const K* kin, K* kout, unsigned n, unsigned segments, const int* begin_offsets,
                                            const int* end_offsets, unsigned begin_bit, unsigned end_bit, hipStream_t s) {
  if (n == 0) return hipSuccess;
  return prim_run(tmp, [&](void* t, size_t& b) {
    return rocprim::segmented_radix_sort_keys(t, b, kin, kout, n, segments, begin_offsets, end_offsets, begin_bit, end_bit, s);
  });
}
template <typename K, typename V>
static inline hipError_t prim_seg_sort_pairs(PrimTmp& tmp, const K* kin, K* kout, const V* vin, V* vout, unsigned n, unsigned segments,
                                             const int* begin_offsets, const int* end_offsets, unsigned begin_bit, unsigned end_bit, hipStream_t s) {
  if (n == 0) return hipSuccess;
  return prim_run(tmp, [&](void* t, size_t& b) {
    return rocprim::segmented_radix_sort_pairs(t, b, kin, kout, vin, vout, n, segments, begin_offsets, end_offsets, begin_bit, end_bit, s);
  });
}
