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

// ---- the detector (include/msfm.h, "Detecting SIFT keypoints") ----
#define SIFT_ORI_BINS 36
#define SIFT_MAX_ANGLES 4
#define SIFT_DETECT_STATS 18
enum {   // indices of msfm_scalespace_detect's stats
  SIFT_ST_CAND = 0, SIFT_ST_REJ_PEAK, SIFT_ST_REJ_EDGE, SIFT_ST_REJ_NEG, SIFT_ST_REJ_OFFSET, SIFT_ST_REJ_BOUNDS, SIFT_ST_KEYPOINTS, SIFT_ST_FOUND,
  SIFT_ST_ANGLES0, SIFT_ST_MOVED = SIFT_ST_ANGLES0 + SIFT_MAX_ANGLES + 1, SIFT_ST_UNCONVERGED, SIFT_ST_WAITS, SIFT_ST_H2D, SIFT_ST_D2H
};
enum { SIFT_KP_STATUS = 15, SIFT_KP_MOVED = 16, SIFT_KP_UNCONVERGED = 32 };   // SiftRawKp.flags: the rejecting rule (0: accepted) and two bits

struct SiftRawKp {   // what the refinement leaves per candidate
  int o, ix, iy, is;
  float xn, yn, sn;
  int flags;
};

struct SiftOrientIn {   // what the orientation kernel reads per keypoint: the raw keypoint's place and the host's sigmaw
  int o, is;
  float xn, yn, sigmaw;
};

static inline std::string sift_check_detect(float peak_thresh, float edge_thresh, int max_frames) {
  if (!std::isfinite(peak_thresh) || peak_thresh < 0.f) return "peak_thresh is negative or not finite";
  if (!std::isfinite(edge_thresh) || edge_thresh < 0.f) return "edge_thresh is negative or not finite";
  if (max_frames < 0 || max_frames > SIFT_MAX_FRAMES) return sift_fmt("max_frames = %ld outside [0, %ld]", max_frames, SIFT_MAX_FRAMES);
  return "";
}

static inline float sift_edge_bound(float edge_thresh) {
  const double e = (double)edge_thresh;
  return (float)((e + 1) * (e + 1) / e);
}

static inline float sift_sigmaw(int S, float sn) { return (float)(1.5 * sift_sigma0(S) * std::pow(2.0, (double)sn / S)); }

static inline float sift_frame_sigma(int S, int o, float sn) { return (float)(1.6 * std::pow(2.0, 1.0 / S) * std::pow(2.0, o + (double)sn / S)); }

// raw keypoints [n] (the refinement's, every candidate in order) -> the counters of the rejections and the accepted ones in order
static inline void sift_collect(const std::vector<SiftRawKp>& raw, int S, int64_t* st, std::vector<int>* kept, std::vector<SiftOrientIn>* in) {
  st[SIFT_ST_CAND] = (int64_t)raw.size();
  for (size_t c = 0; c < raw.size(); c++) {
    const SiftRawKp& r = raw[c];
    const int status = r.flags & SIFT_KP_STATUS;
    if (status) { st[SIFT_ST_REJ_PEAK + status - 1]++; continue; }
    st[SIFT_ST_KEYPOINTS]++;
    if (r.flags & SIFT_KP_MOVED) st[SIFT_ST_MOVED]++;
    if (r.flags & SIFT_KP_UNCONVERGED) st[SIFT_ST_UNCONVERGED]++;
    kept->push_back((int)c);
    in->push_back(SiftOrientIn{r.o, r.is, r.xn, r.yn, sift_sigmaw(S, r.sn)});
  }
}

// the frames [n_found][4] of the kept raw keypoints and their angles, in order; n_found is also counted into st
static inline void sift_make_frames(const std::vector<SiftRawKp>& raw, const std::vector<int>& kept, const int* nang, const float* theta, int S,
                                    int64_t* st, std::vector<float>* frames) {
  for (size_t k = 0; k < kept.size(); k++) {
    const SiftRawKp& r = raw[kept[k]];
    const int na = std::min(std::max(nang[k], 0), SIFT_MAX_ANGLES);
    st[SIFT_ST_ANGLES0 + na]++;
    st[SIFT_ST_FOUND] += na;
    const float sc = (float)(1 << r.o), sigma = sift_frame_sigma(S, r.o, r.sn);
    for (int a = 0; a < na; a++) {
      const float f[4] = {r.xn * sc, r.yn * sc, sigma, theta[SIFT_MAX_ANGLES * k + a]};
      frames->insert(frames->end(), f, f + 4);
    }
  }
}
