// The argument checks of msfm_descset_voctree_train (metricsfm_amd/csrc/voctrain_args.h, the code the library refuses with), its
// shifts and its draw.  Needs neither the library nor a device; tests/test_voctrain_abi.py builds it with the host sanitizers.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../metricsfm_amd/csrc/voctrain_args.h"

static int fail(const char* what) {
  std::printf("voctrain_host_check FAILED: %s\n", what);
  return 1;
}

static uint32_t bits(float v) {
  uint32_t b;
  std::memcpy(&b, &v, sizeof b);
  return b & 0x7fffffffu;
}

int main() {
  voctrain_options o;
  voctrain_defaults(&o);
  if (o.k != 10 || o.levels != 6 || o.max_iters != 11 || o.image_step != 1 || o.seed != 0) return fail("the defaults");
  if (!voctrain_check_options(&o).empty()) return fail("the defaults are refused");
  if (voctrain_check_options(nullptr).empty()) return fail("a null options pointer accepted");
  struct { int voctrain_options::*field; int bad[2]; int good[2]; } cases[] = {
      {&voctrain_options::k, {1, 65}, {2, 64}},
      {&voctrain_options::levels, {0, 33}, {1, 32}},
      {&voctrain_options::max_iters, {0, -3}, {1, 1000}},
      {&voctrain_options::image_step, {0, -1}, {1, 1 << 30}},
  };
  for (const auto& c : cases) {
    for (int v : c.bad) {
      voctrain_options p = o;
      p.*(c.field) = v;
      if (voctrain_check_options(&p).empty()) return fail("an option out of range accepted");
    }
    for (int v : c.good) {
      voctrain_options p = o;
      p.*(c.field) = v;
      if (!voctrain_check_options(&p).empty()) return fail("an option at its limit refused");
    }
  }

  // the sample: every image_step-th image with all its features
  std::vector<int> images, off;
  const std::vector<int> count = {0, 1, 301, 333, 512, 700, 31};
  if (!voctrain_sample(7, count.data(), 1, &images, &off).empty() || images.size() != 7 || off.back() != 1878 || off[3] != 302)
    return fail("the sample of step 1");
  if (!voctrain_sample(7, count.data(), 2, &images, &off).empty() || images != std::vector<int>({0, 2, 4, 6}) || off.back() != 844)
    return fail("the sample of step 2");
  if (voctrain_sample(7, count.data(), 100, &images, &off).empty()) return fail("a sample without features accepted");
  if (voctrain_sample(0, count.data(), 1, &images, &off).empty()) return fail("no image accepted");
  const std::vector<int> big = {1 << 22, 5, 1 << 22, 7, 1};
  if (!voctrain_sample(3, big.data(), 2, &images, &off).empty() || off.back() != (1 << 23)) return fail("2^23 features refused");
  if (voctrain_sample(5, big.data(), 2, &images, &off).empty()) return fail("2^23 + 1 features accepted");
  if (voctrain_sample(5, big.data(), 1, &images, &off).empty()) return fail("2^23 + 13 features accepted");
  const std::vector<int> huge(3, 0x7fffffff);
  if (voctrain_sample(3, huge.data(), 1, &images, &off).empty()) return fail("a sum past 2^31 accepted");
  const std::vector<int> neg = {4, -1};
  if (voctrain_sample(2, neg.data(), 1, &images, &off).empty()) return fail("a negative count accepted");

  // the shifts: 512 maxabs^2 < 2^(40 - weight_shift), maxabs 2^sum_shift < 2^39
  int ws = 0, ss = 0;
  for (float v : {0.0f, 1e-30f, 0.0004f, 0.51f, 1.0f, 1.5f, 255.0f, 256.0f, 512.0f, 2560.0f, 2895.9998f}) {
    if (!voctrain_shifts(bits(v), &ws, &ss).empty()) return fail("a legal magnitude refused");
    if (!(512.0 * (double)v * (double)v < std::ldexp(1.0, 40 - ws))) return fail("the weight shift is too large");
    if (!((double)v * std::ldexp(1.0, ss) < std::ldexp(1.0, 39))) return fail("the sum shift is too large");
    if (v >= 1e-30f && !((double)v * std::ldexp(1.0, ss) >= std::ldexp(1.0, 38))) return fail("the sum shift wastes a bit");
  }
  if (!voctrain_shifts(bits(255.0f), &ws, &ss).empty() || ws != 15 || ss != 31) return fail("the shifts of 8-bit descriptors");
  if (voctrain_shifts(bits(2896.0f), &ws, &ss).empty() || voctrain_shifts(bits(-2896.0f), &ws, &ss).empty() ||
      voctrain_shifts(bits(1e30f), &ws, &ss).empty())
    return fail("a value of 2896 or more accepted");
  if (voctrain_shifts(bits(INFINITY), &ws, &ss).empty() || voctrain_shifts(bits(NAN), &ws, &ss).empty()) return fail("a non-finite value accepted");

  // the draw: a pure function of its four arguments, each of which matters; first values pinned against the Python restatement
  if (voctrain_draw(0, 0, 0, 0) != voctrain_draw(0, 0, 0, 0)) return fail("the draw is not a function");
  const uint64_t d0 = voctrain_draw(7, 3, 11, 2);
  if (d0 == voctrain_draw(8, 3, 11, 2) || d0 == voctrain_draw(7, 4, 11, 2) || d0 == voctrain_draw(7, 3, 12, 2) || d0 == voctrain_draw(7, 3, 11, 3))
    return fail("an argument of the draw does not matter");
  std::printf("voctrain_host_check ok draw %llu %llu\n", (unsigned long long)voctrain_draw(0, 0, 0, 0), (unsigned long long)d0);
  return 0;
}
