// What sift.hip does without a device: the argument checks and the numbers that need the C library's exp, pow, log2, fmod, sin or
// cos (include/msfm.h, "host data").  Plain C++, binary64, rounded to binary32 once; the kernels and the restatements of tests/
// take them as data.  A check returns an empty string or the refusal's text.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#define SIFT_MAX_SIDE 16384
#define SIFT_MAX_OCTAVES 8
#define SIFT_MAX_LEVELS 8
#define SIFT_MAX_FRAMES 65535
#define SIFT_MAX_RADIUS 64      // of a blur (45 at n_levels = 1, 9 at n_levels = 5): the LDS tiles of the blur kernels are sized by it
#define SIFT_TABLE 257          // entries of the window table

struct SiftFrame {   // one frame as the descriptor kernel reads it: the caller's four values and the host's five
  float x, y, sigma, thr, st, ct;
  int o, is;
};

static inline std::string sift_fmt(const char* fmt, long a = 0, long b = 0, long c = 0) {
  char buf[256];
  snprintf(buf, sizeof buf, fmt, a, b, c);
  return buf;
}

static inline std::string sift_check_create(const uint8_t* gray, int width, int height, int stride, int n_octaves, int n_levels) {
  if (!gray) return "null argument";
  if (width < 2 || width > SIFT_MAX_SIDE || height < 2 || height > SIFT_MAX_SIDE)
    return sift_fmt("%ld x %ld pixels: a side outside [2, %ld]", width, height, SIFT_MAX_SIDE);
  if (stride < width) return sift_fmt("stride = %ld below width = %ld", stride, width);
  if (n_octaves < 1 || n_octaves > SIFT_MAX_OCTAVES) return sift_fmt("n_octaves = %ld outside [1, %ld]", n_octaves, SIFT_MAX_OCTAVES);
  if (n_levels < 1 || n_levels > SIFT_MAX_LEVELS) return sift_fmt("n_levels = %ld outside [1, %ld]", n_levels, SIFT_MAX_LEVELS);
  if ((std::min(width, height) >> (n_octaves - 1)) < 2) return sift_fmt("octave %ld of %ld x %ld pixels has a side below 2", n_octaves - 1, width, height);
  return "";
}

static inline double sift_sigma0(int S) { return 1.6 * std::pow(2.0, 1.0 / S); }

// the blur that makes level s (-1 .. S + 1) from the level before it
static inline double sift_level_blur(int S, int s) {
  const double k = std::pow(2.0, 1.0 / S), sigma0 = 1.6 * k;
  if (s < 0) {
    const double sa = sigma0 * std::pow(k, -1.0);
    return std::sqrt(sa * sa - 0.25);
  }
  const double dsigma0 = sigma0 * std::sqrt(1 - 1 / (k * k));
  return dsigma0 * std::pow(k, (double)s);
}

static inline std::vector<float> sift_taps(double sd) {
  const int W = std::max((int)std::ceil(4 * sd), 1);
  std::vector<double> g(2 * W + 1);
  double sum = 0;
  for (int i = 0; i <= 2 * W; i++) {
    g[i] = std::exp(-0.5 * ((double)(i - W) * (double)(i - W)) / (sd * sd));
    sum += g[i];
  }
  std::vector<float> out(2 * W + 1);
  for (int i = 0; i <= 2 * W; i++) out[i] = (float)(g[i] / sum);
  return out;
}

static inline std::vector<float> sift_table() {
  std::vector<float> T(SIFT_TABLE);
  for (int i = 0; i < SIFT_TABLE; i++) T[i] = (float)std::exp(-i * 25.0 / 256.0);
  return T;
}

// frames [n][4] -> the records of the kernel; the refusal names the first bad frame
static inline std::string sift_frames(const float* frames, int n, int O, int S, std::vector<SiftFrame>* out) {
  if (n < 0 || n > SIFT_MAX_FRAMES) return sift_fmt("n = %ld frames outside [0, %ld]", n, SIFT_MAX_FRAMES);
  if (!frames) return "null argument";
  for (int f = 0; f < n; f++) {
    for (int c = 0; c < 4; c++)
      if (!std::isfinite(frames[4 * f + c])) return sift_fmt("frame %ld: value %ld is not finite", f, c);
    if (!(frames[4 * f + 2] > 0.f)) return sift_fmt("frame %ld: sigma is not positive", f);
  }
  out->resize(n);
  const double sigma0 = sift_sigma0(S), two_pi = 6.283185307179586;
  for (int f = 0; f < n; f++) {
    SiftFrame& r = (*out)[f];
    r.x = frames[4 * f]; r.y = frames[4 * f + 1]; r.sigma = frames[4 * f + 2];
    const double sigma = r.sigma, theta = frames[4 * f + 3];
    const double phi = std::log2((sigma + 1.1920928955078125e-07) / sigma0);
    double o = std::floor(phi - (-1 + 0.5) / S);
    o = std::min(std::max(o, 0.0), (double)(O - 1));
    double is = std::floor(S * (phi - o) + 0.5);
    is = std::min(std::max(is, 0.0), (double)(S - 1));
    r.o = (int)o; r.is = (int)is;
    double thr = std::fmod(theta, two_pi);
    if (thr < 0) thr += two_pi;
    r.thr = (float)thr; r.st = (float)std::sin(theta); r.ct = (float)std::cos(theta);
  }
  return "";
}
