// The sequential restatement of "Detecting SIFT keypoints" in include/msfm.h: DoG extrema, refinement, orientation histogram and
// frames, one cell and one keypoint after the other on one thread, on the Gaussian levels and gradient planes that
// tests/sift_ref.cpp wrote.  Built with -ffp-contract=off, so every binary32 operation is rounded on its own.  The window table is
// an input.  sigmaw, the edge bound and the frames' sigma are host numbers in the library too (metricsfm_amd/csrc/sift_args.h):
// this program makes them with the same C library calls in binary64.
//
//   siftdetect_ref in.bin out.bin
// in : int32 w, h, O, S; float peak_thresh, edge_thresh; float T[257]; per octave S + 3 levels [h_o][w_o], then per level
//      0 .. S - 1 modulus and angle (the planes part of sift_ref's output)
// out: int64 stats[18] (include/msfm.h; bytes each way left 0); int64 n_cand; n_cand cells (int32 o, s, y, x); n_cand raw
//      keypoints (int32 o, ix, iy, is; float xn, yn, sn; int32 flags); n_cand floats, the refinement's val; n_found frames
//      (float x, y, sigma, angle).
//      stdout: "siftdetect_ref ok, <seconds>"
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

static const float PI2 = 6.28318548f;
enum { ST_CAND = 0, ST_REJ = 1, ST_KEYPOINTS = 6, ST_FOUND = 7, ST_ANGLES0 = 8, ST_MOVED = 13, ST_UNCONVERGED = 14, ST_WAITS = 15, N_STATS = 18 };
enum { KP_MOVED = 16, KP_UNCONVERGED = 32 };

struct Raw {
  int32_t o, ix, iy, is;
  float xn, yn, sn;
  int32_t flags;
};

struct Octave {
  int w = 0, h = 0;
  std::vector<std::vector<float>> gss, mod, ang;   // gss[s + 1]
  float D(int x, int y, int s) const {             // s = -1 .. S
    const size_t p = (size_t)y * w + x;
    return gss[s + 2][p] - gss[s + 1][p];
  }
};

template <class X>
static void get(FILE* f, X* p, size_t n) {
  if (n && fread(p, sizeof(X), n, f) != n) { fprintf(stderr, "siftdetect_ref: short input\n"); exit(2); }
}

static bool extremum(const Octave& Q, int x, int y, int s, float thr) {
  const float v = Q.D(x, y, s);
  bool mx = v >= thr, mn = v <= -thr;
  for (int k = -1; k <= 1; k++)
    for (int j = -1; j <= 1; j++)
      for (int i = -1; i <= 1; i++) {
        if (!i && !j && !k) continue;
        const float n = Q.D(x + i, y + j, s + k);
        mx = mx && v > n;
        mn = mn && v < n;
      }
  return mx || mn;
}

static Raw refine(const Octave& Q, int o, int S, int x0, int y0, int s, float peak, float bound, float* val_out) {
  const int w = Q.w, h = Q.h;
  int x = x0, y = y0, mvx = 0, mvy = 0;
  float Dx = 0, Dy = 0, Ds = 0, Dxx = 0, Dyy = 0, Dxy = 0, v0 = 0, b[3] = {0, 0, 0};
  for (int pass = 0; pass < 5; pass++) {
    x += mvx; y += mvy;
    auto d = [&](int i, int j, int k) { return Q.D(x + i, y + j, s + k); };
    v0 = d(0, 0, 0);
    Dx = 0.5f * (d(1, 0, 0) - d(-1, 0, 0)); Dy = 0.5f * (d(0, 1, 0) - d(0, -1, 0)); Ds = 0.5f * (d(0, 0, 1) - d(0, 0, -1));
    Dxx = (d(1, 0, 0) + d(-1, 0, 0)) - 2.0f * v0; Dyy = (d(0, 1, 0) + d(0, -1, 0)) - 2.0f * v0;
    const float Dss = (d(0, 0, 1) + d(0, 0, -1)) - 2.0f * v0;
    Dxy = 0.25f * (((d(1, 1, 0) + d(-1, -1, 0)) - d(-1, 1, 0)) - d(1, -1, 0));
    const float Dxs = 0.25f * (((d(1, 0, 1) + d(-1, 0, -1)) - d(-1, 0, 1)) - d(1, 0, -1));
    const float Dys = 0.25f * (((d(0, 1, 1) + d(0, -1, -1)) - d(0, -1, 1)) - d(0, 1, -1));
    float A[3][3] = {{Dxx, Dxy, Dxs}, {Dxy, Dyy, Dys}, {Dxs, Dys, Dss}};
    b[0] = -Dx; b[1] = -Dy; b[2] = -Ds;
    bool singular = false;
    for (int j = 0; j < 3 && !singular; j++) {
      int pi = j;
      float pa = std::fabs(A[j][j]);
      for (int i = j + 1; i < 3; i++)
        if (std::fabs(A[i][j]) > pa) { pa = std::fabs(A[i][j]); pi = i; }
      if (!(pa > 0.f)) { singular = true; break; }
      for (int jj = j; jj < 3; jj++) { const float t = A[pi][jj]; A[pi][jj] = A[j][jj]; A[j][jj] = t; }
      { const float t = b[pi]; b[pi] = b[j]; b[j] = t; }
      const float pv = A[j][j];
      for (int jj = j; jj < 3; jj++) A[j][jj] = A[j][jj] / pv;
      b[j] = b[j] / pv;
      for (int ii = j + 1; ii < 3; ii++) {
        const float f = A[ii][j];
        for (int jj = j; jj < 3; jj++) A[ii][jj] = A[ii][jj] - f * A[j][jj];
        b[ii] = b[ii] - f * b[j];
      }
    }
    if (singular) b[0] = b[1] = b[2] = 0.f;
    else
      for (int i = 2; i > 0; i--)
        for (int ii = i - 1; ii >= 0; ii--) b[ii] = b[ii] - b[i] * A[ii][i];
    mvx = (b[0] > 0.6f && x < w - 2 ? 1 : 0) + (b[0] < -0.6f && x > 1 ? -1 : 0);
    mvy = (b[1] > 0.6f && y < h - 2 ? 1 : 0) + (b[1] < -0.6f && y > 1 ? -1 : 0);
    if (mvx == 0 && mvy == 0) break;
  }
  const float val = v0 + 0.5f * ((Dx * b[0] + Dy * b[1]) + Ds * b[2]);
  const float score = ((Dxx + Dyy) * (Dxx + Dyy)) / (Dxx * Dyy - Dxy * Dxy);
  *val_out = val;
  Raw r;
  r.o = o; r.ix = x; r.iy = y; r.is = s;
  r.xn = (float)x + b[0]; r.yn = (float)y + b[1]; r.sn = (float)s + b[2];
  int status = 0;
  if (!(std::fabs(val) > peak)) status = 1;
  else if (!(score < bound)) status = 2;
  else if (!(score >= 0.f)) status = 3;
  else if (!(std::fabs(b[0]) < 1.5f && std::fabs(b[1]) < 1.5f && std::fabs(b[2]) < 1.5f)) status = 4;
  else if (!(r.xn >= 0.f && r.xn <= (float)(w - 1) && r.yn >= 0.f && r.yn <= (float)(h - 1) && r.sn >= -1.0f && r.sn <= (float)(S + 1))) status = 5;
  r.flags = status | ((x != x0 || y != y0) ? KP_MOVED : 0) | ((mvx || mvy) ? KP_UNCONVERGED : 0);
  return r;
}

// -> the number of angles; theta [4]
static int orientations(const Octave& Q, const Raw& K, float sigmaw, const float* T, float* theta) {
  const int w = Q.w, h = Q.h;
  const std::vector<float>&mod = Q.mod[K.is], &ang = Q.ang[K.is];
  const int xi = (int)(K.xn + 0.5f), yi = (int)(K.yn + 0.5f), W = (int)std::floor(3.0f * sigmaw);
  const float r2max = (float)(W * W) + 0.6f, den = (2.0f * sigmaw) * sigmaw;
  float hist[36];
  for (float& v : hist) v = 0.f;
  const int dy0 = -W > 1 - yi ? -W : 1 - yi, dy1 = W < h - yi - 2 ? W : h - yi - 2;
  const int dx0 = -W > 1 - xi ? -W : 1 - xi, dx1 = W < w - xi - 2 ? W : w - xi - 2;
  for (int dyi = dy0; dyi <= dy1; dyi++)
    for (int dxi = dx0; dxi <= dx1; dxi++) {
      const int px = xi + dxi, py = yi + dyi;
      const size_t at = (size_t)py * w + px;
      const float dx = (float)px - K.xn, dy = (float)py - K.yn;
      const float r2 = dx * dx + dy * dy;
      if (!(r2 < r2max)) continue;
      const float u = (r2 / den) * 10.24f;
      if (!(u < 256.0f)) continue;
      const int i = (int)u;
      const float f = u - (float)i;
      const float win = T[i] + f * (T[i + 1] - T[i]);
      const float v = win * mod[at];
      const float fb = (36.0f * ang[at]) / PI2;
      const float bf = std::floor(fb - 0.5f);
      const float rb = fb - (bf + 0.5f);
      const int ib = ((int)bf + 36) % 36;
      hist[ib] = hist[ib] + (1.0f - rb) * v;
      hist[(ib + 1) % 36] = hist[(ib + 1) % 36] + rb * v;
    }
  for (int it = 0; it < 6; it++) {
    float old[36];
    for (int i = 0; i < 36; i++) old[i] = hist[i];
    for (int i = 0; i < 36; i++) hist[i] = ((old[(i + 35) % 36] + old[i]) + old[(i + 1) % 36]) / 3.0f;
  }
  float m = hist[0];
  for (int i = 1; i < 36; i++) m = hist[i] > m ? hist[i] : m;
  int n = 0;
  for (int i = 0; i < 36 && n < 4; i++) {
    const float h0 = hist[i], hm = hist[(i + 35) % 36], hp = hist[(i + 1) % 36];
    if (h0 > 0.8f * m && h0 > hm && h0 > hp) {
      const float di = (-0.5f * (hp - hm)) / ((hp + hm) - 2.0f * h0);
      theta[n++] = (PI2 * (((float)i + di) + 0.5f)) / 36.0f;
    }
  }
  return n;
}

int main(int argc, char** argv) {
  if (argc != 3) { fprintf(stderr, "usage: siftdetect_ref in.bin out.bin\n"); return 2; }
  FILE* fi = fopen(argv[1], "rb");
  if (!fi) { perror(argv[1]); return 2; }
  int32_t hd[4];
  float th[2];
  get(fi, hd, 4);
  get(fi, th, 2);
  const int w = hd[0], h = hd[1], O = hd[2], S = hd[3];
  const float peak = th[0], edge = th[1];
  std::vector<float> T(257);
  get(fi, T.data(), T.size());
  std::vector<Octave> oct(O);
  for (int o = 0; o < O; o++) {
    Octave& Q = oct[o];
    Q.w = w >> o; Q.h = h >> o;
    const size_t n = (size_t)Q.w * Q.h;
    Q.gss.assign(S + 3, std::vector<float>(n)); Q.mod.assign(S, std::vector<float>(n)); Q.ang.assign(S, std::vector<float>(n));
    for (auto& p : Q.gss) get(fi, p.data(), n);
    for (int s = 0; s < S; s++) { get(fi, Q.mod[s].data(), n); get(fi, Q.ang[s].data(), n); }
  }
  fclose(fi);

  const auto t0 = std::chrono::steady_clock::now();
  const double e = (double)edge;
  const float bound = (float)((e + 1) * (e + 1) / e), thr = 0.8f * peak;
  const double sigma0 = 1.6 * std::pow(2.0, 1.0 / S);
  int64_t st[N_STATS] = {};
  std::vector<int32_t> cells;
  std::vector<Raw> raw;
  std::vector<float> frames, vals;
  for (int o = 0; o < O; o++)
    for (int s = 0; s < S; s++)
      for (int y = 1; y <= oct[o].h - 2; y++)
        for (int x = 1; x <= oct[o].w - 2; x++) {
          if (!extremum(oct[o], x, y, s, thr)) continue;
          const int32_t c[4] = {o, s, y, x};
          cells.insert(cells.end(), c, c + 4);
          float val = 0.f;
          const Raw r = refine(oct[o], o, S, x, y, s, peak, bound, &val);
          raw.push_back(r);
          vals.push_back(val);
          st[ST_CAND]++;
          if (r.flags & 15) { st[ST_REJ + (r.flags & 15) - 1]++; continue; }
          st[ST_KEYPOINTS]++;
          if (r.flags & KP_MOVED) st[ST_MOVED]++;
          if (r.flags & KP_UNCONVERGED) st[ST_UNCONVERGED]++;
          const float sigmaw = (float)(1.5 * sigma0 * std::pow(2.0, (double)r.sn / S));
          float theta[4];
          const int na = orientations(oct[o], r, sigmaw, T.data(), theta);
          st[ST_ANGLES0 + na]++;
          st[ST_FOUND] += na;
          const float sc = (float)(1 << o), sigma = (float)(1.6 * std::pow(2.0, 1.0 / S) * std::pow(2.0, o + (double)r.sn / S));
          for (int a = 0; a < na; a++) {
            const float f[4] = {r.xn * sc, r.yn * sc, sigma, theta[a]};
            frames.insert(frames.end(), f, f + 4);
          }
        }
  st[ST_WAITS] = 2 + (st[ST_CAND] > 0 ? 1 : 0);   // the library's: count, raw keypoints (when there are candidates), angles
  const auto t1 = std::chrono::steady_clock::now();

  FILE* fo = fopen(argv[2], "wb");
  if (!fo) { perror(argv[2]); return 2; }
  const int64_t n_cand = st[ST_CAND];
  fwrite(st, sizeof(int64_t), N_STATS, fo);
  fwrite(&n_cand, sizeof(int64_t), 1, fo);
  fwrite(cells.data(), sizeof(int32_t), cells.size(), fo);
  fwrite(raw.data(), sizeof(Raw), raw.size(), fo);
  fwrite(vals.data(), sizeof(float), vals.size(), fo);
  fwrite(frames.data(), sizeof(float), frames.size(), fo);
  if (fclose(fo) != 0) { perror(argv[2]); return 2; }
  printf("siftdetect_ref ok, %.6f s\n", std::chrono::duration<double>(t1 - t0).count());
  return 0;
}
