// The sequential restatement of "Describing given SIFT frames" in include/msfm.h: stretch, Gaussian scale space, gradients and the
// descriptor of given frames, one pixel and one frame after the other on one thread.  Built with -ffp-contract=off, so every
// binary32 operation is rounded on its own.  The numbers that need exp, pow, log2, fmod, sin or cos - the taps, the window table
// and per frame (thr, st, ct, o, is) - are INPUTS: no libm call of this program decides a bit (sqrtf is correctly rounded).
//
//   sift_ref in.bin out.bin
// in : int32 w, h, O, S, n_frames; uint8 image [h][w]; S + 3 tap sets (int32 count, float taps), levels -1 .. S + 1;
//      float T[257]; n_frames records (float x, y, sigma, thr, st, ct; int32 o, is)
// out: per octave S + 3 levels [h_o][w_o], then per level 0 .. S - 1 modulus and angle; then rows [n][128] with quantize = 0 and
//      rows [n][128] with quantize = 1.  stdout: "sift_ref ok, <seconds scale space>, <seconds descriptors>"
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

static const float EPS = 1.19209290e-07f;
static const float PI2 = 6.28318548f;

struct Frame {
  float x, y, sigma, thr, st, ct;
  int32_t o, is;
};

struct Plane {
  int w = 0, h = 0;
  std::vector<float> v;
  float at(int x, int y) const { return v[(size_t)y * w + x]; }
};

static int clampi(int a, int lo, int hi) { return a < lo ? lo : (a > hi ? hi : a); }

static Plane blur(const Plane& src, const std::vector<float>& g) {
  const int W = (int)g.size() / 2, w = src.w, h = src.h;
  Plane rows = src, out = src;
  for (int y = 0; y < h; y++)
    for (int x = 0; x < w; x++) {
      float acc = 0.f;
      for (int i = 0; i <= 2 * W; i++) acc = acc + g[i] * src.at(clampi(x + i - W, 0, w - 1), y);
      rows.v[(size_t)y * w + x] = acc;
    }
  for (int y = 0; y < h; y++)
    for (int x = 0; x < w; x++) {
      float acc = 0.f;
      for (int i = 0; i <= 2 * W; i++) acc = acc + g[i] * rows.at(x, clampi(y + i - W, 0, h - 1));
      out.v[(size_t)y * w + x] = acc;
    }
  return out;
}

static float angle_of(float gx, float gy) {
  const float ax = std::fabs(gx), ay = std::fabs(gy);
  const float mx = ax > ay ? ax : ay, mn = ax > ay ? ay : ax;
  if (mx == 0.f) return 0.f;
  const float t = mn / mx, q = t * t;
  float r = -0.01172120f;
  r = 0.05265332f + q * r;
  r = -0.11643287f + q * r;
  r = 0.19354346f + q * r;
  r = -0.33262347f + q * r;
  r = 0.99997726f + q * r;
  r = t * r;
  if (ay > ax) r = 1.57079637f - r;
  if (gx < 0.f) r = 3.14159274f - r;
  if (gy < 0.f) r = PI2 - r;
  if (r >= PI2) r = r - PI2;
  return r;
}

static void gradient(const Plane& I, Plane* mod, Plane* ang) {
  const int w = I.w, h = I.h;
  *mod = I; *ang = I;
  for (int y = 0; y < h; y++)
    for (int x = 0; x < w; x++) {
      const float gx = x == 0 ? I.at(1, y) - I.at(0, y) : x == w - 1 ? I.at(w - 1, y) - I.at(w - 2, y) : 0.5f * (I.at(x + 1, y) - I.at(x - 1, y));
      const float gy = y == 0 ? I.at(x, 1) - I.at(x, 0) : y == h - 1 ? I.at(x, h - 1) - I.at(x, h - 2) : 0.5f * (I.at(x, y + 1) - I.at(x, y - 1));
      mod->v[(size_t)y * w + x] = sqrtf(gx * gx + gy * gy);
      ang->v[(size_t)y * w + x] = angle_of(gx, gy);
    }
}

static float norm_of(const float* h) {
  float s = 0.f;
  for (int b = 0; b < 128; b++) s = s + h[b] * h[b];
  return sqrtf(s) + EPS;
}

// the row of one frame on its level's gradient planes; out [128]
static void describe(const Frame& F, const Plane& mod, const Plane& ang, const float* T, int quantize, float* out) {
  const int w = mod.w, h = mod.h;
  for (int b = 0; b < 128; b++) out[b] = 0.f;
  const float sc = (float)(1 << F.o);
  const float xp = F.x / sc, yp = F.y / sc, sp = F.sigma / sc;
  const float xf = xp + 0.5f, yf = yp + 0.5f;
  if (!(xf > -1.0f && xf < (float)w && yf > -1.0f && yf < (float)(h - 1))) return;
  const int xi = (int)xf, yi = (int)yf;
  const float SBP = 3.0f * sp + EPS;
  const float Wf = std::floor(1.41421356f * SBP * 2.5f + 0.5f);
  const int W = Wf < 32768.0f ? (int)Wf : 32768;
  float hist[128];
  for (int b = 0; b < 128; b++) hist[b] = 0.f;
  const int dy0 = -W > 1 - yi ? -W : 1 - yi, dy1 = W < h - yi - 2 ? W : h - yi - 2;
  const int dx0 = -W > 1 - xi ? -W : 1 - xi, dx1 = W < w - xi - 2 ? W : w - xi - 2;
  for (int dyi = dy0; dyi <= dy1; dyi++)
    for (int dxi = dx0; dxi <= dx1; dxi++) {
      const int px = xi + dxi, py = yi + dyi;
      const float dx = (float)px - xp, dy = (float)py - yp;
      const float nx = (F.ct * dx + F.st * dy) / SBP;
      const float ny = ((-F.st) * dx + F.ct * dy) / SBP;
      float th = ang.at(px, py) - F.thr;
      if (th < 0.f) th = th + PI2;
      if (th >= PI2) th = th - PI2;
      const float nt = (8.0f * th) / PI2;
      const float u = ((nx * nx + ny * ny) * 0.125f) * 10.24f;
      if (!(u < 256.0f)) continue;
      const int i = (int)u;
      const float fr = u - (float)i;
      const float win = T[i] + fr * (T[i + 1] - T[i]);
      const float fbx = std::floor(nx - 0.5f), fby = std::floor(ny - 0.5f), fbt = std::floor(nt);
      if (!(fbx >= -3.0f && fbx <= 1.0f && fby >= -3.0f && fby <= 1.0f)) continue;
      const int bx = (int)fbx, by = (int)fby, bt = (int)fbt;
      const float rx = nx - (fbx + 0.5f), ry = ny - (fby + 0.5f), rt = nt - fbt;
      const float wx[2] = {std::fabs(1.0f - rx), std::fabs(rx)}, wy[2] = {std::fabs(1.0f - ry), std::fabs(ry)},
                  wt[2] = {std::fabs(1.0f - rt), std::fabs(rt)};
      const float base = win * mod.at(px, py);
      for (int dby = 0; dby < 2; dby++)
        for (int dbx = 0; dbx < 2; dbx++)
          for (int dbt = 0; dbt < 2; dbt++) {
            const int cx = bx + dbx, cy = by + dby;
            if (cx < -2 || cx > 1 || cy < -2 || cy > 1) continue;
            const int bin = ((bt + dbt) % 8) + 8 * (cx + 2) + 32 * (cy + 2);
            hist[bin] = hist[bin] + ((base * wx[dbx]) * wy[dby]) * wt[dbt];
          }
    }
  float n = norm_of(hist);
  for (int b = 0; b < 128; b++) {
    hist[b] = hist[b] / n;
    if (hist[b] > 0.2f) hist[b] = 0.2f;
  }
  n = norm_of(hist);
  for (int b = 0; b < 128; b++) {
    const int t = b % 8, i = (b / 8) % 4, j = b / 32;
    float v = 512.0f * (hist[b] / n);
    if (quantize) {
      v = (float)(int)v;
      if (v > 255.0f) v = 255.0f;
    }
    out[((8 - t) % 8) + 8 * i + 32 * (3 - j)] = v;
  }
}

template <class X>
static void get(FILE* f, X* p, size_t n) {
  if (n && fread(p, sizeof(X), n, f) != n) { fprintf(stderr, "sift_ref: short input\n"); exit(2); }
}

int main(int argc, char** argv) {
  if (argc != 3) { fprintf(stderr, "usage: sift_ref in.bin out.bin\n"); return 2; }
  FILE* fi = fopen(argv[1], "rb");
  if (!fi) { perror(argv[1]); return 2; }
  int32_t hd[5];
  get(fi, hd, 5);
  const int w = hd[0], h = hd[1], O = hd[2], S = hd[3], n = hd[4];
  std::vector<uint8_t> img((size_t)w * h);
  get(fi, img.data(), img.size());
  std::vector<std::vector<float>> taps(S + 3);
  for (auto& g : taps) {
    int32_t c = 0;
    get(fi, &c, 1);
    g.resize(c);
    get(fi, g.data(), g.size());
  }
  std::vector<float> T(257);
  get(fi, T.data(), T.size());
  std::vector<Frame> frames(n);
  get(fi, frames.data(), frames.size());
  fclose(fi);

  const auto t0 = std::chrono::steady_clock::now();
  int lo = 255, hi = 0;
  for (uint8_t v : img) { lo = v < lo ? v : lo; hi = v > hi ? v : hi; }
  const float fmin = (float)lo, frange = (float)(hi - lo);
  Plane first;
  first.w = w; first.h = h; first.v.resize(img.size());
  for (size_t p = 0; p < img.size(); p++) first.v[p] = ((float)img[p] - fmin) / frange * 255.0f;
  std::vector<std::vector<Plane>> gss(O), mod(O), ang(O);   // gss[o][s + 1]
  for (int o = 0; o < O; o++) {
    gss[o].resize(S + 3); mod[o].resize(S); ang[o].resize(S);
    if (o == 0) gss[0][0] = blur(first, taps[0]);
    else {
      const Plane& up = gss[o - 1][S];   // level S - 1
      Plane& d = gss[o][0];
      d.w = up.w >> 1; d.h = up.h >> 1; d.v.resize((size_t)d.w * d.h);
      for (int y = 0; y < d.h; y++)
        for (int x = 0; x < d.w; x++) d.v[(size_t)y * d.w + x] = up.at(2 * x, 2 * y);
    }
    for (int s = 0; s <= S + 1; s++) gss[o][s + 1] = blur(gss[o][s], taps[s + 1]);
    for (int s = 0; s < S; s++) gradient(gss[o][s + 1], &mod[o][s], &ang[o][s]);
  }
  const auto t1 = std::chrono::steady_clock::now();
  std::vector<float> rows[2];
  for (int qz = 0; qz < 2; qz++) {
    rows[qz].resize((size_t)n * 128);
    for (int f = 0; f < n; f++) describe(frames[f], mod[frames[f].o][frames[f].is], ang[frames[f].o][frames[f].is], T.data(), qz, &rows[qz][(size_t)f * 128]);
  }
  const auto t2 = std::chrono::steady_clock::now();

  FILE* fo = fopen(argv[2], "wb");
  if (!fo) { perror(argv[2]); return 2; }
  for (int o = 0; o < O; o++) {
    for (const Plane& p : gss[o]) fwrite(p.v.data(), sizeof(float), p.v.size(), fo);
    for (int s = 0; s < S; s++) {
      fwrite(mod[o][s].v.data(), sizeof(float), mod[o][s].v.size(), fo);
      fwrite(ang[o][s].v.data(), sizeof(float), ang[o][s].v.size(), fo);
    }
  }
  for (int qz = 0; qz < 2; qz++) fwrite(rows[qz].data(), sizeof(float), rows[qz].size(), fo);
  if (fclose(fo) != 0) { perror(argv[2]); return 2; }
  printf("sift_ref ok, %.6f s scale space, %.6f s descriptors (both quantize forms)\n", std::chrono::duration<double>(t1 - t0).count(),
         std::chrono::duration<double>(t2 - t1).count());
  return 0;
}
