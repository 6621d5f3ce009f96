// The sequential restatement of the dense-stereo definitions of include/msfm.h ("Dense stereo"): census, matching cost, the
// eight path costs, their sum, the left and the right winner with the uniqueness rule, the 3 x 3 median, the consistency check
// and the depth.  One thread, one pixel and one disparity at a time, in the words of the header; nothing here is shared with
// metricsfm_amd/csrc/sgm.hip.
//
//   sgm_ref IN OUT
// IN : int32 w, h, D, P1, P2, mode; float uniqueness; double baseline, focal; uint8 left [h][w], right [h][w]
// OUT: uint32 censusL [h][w], censusR [h][w]; (mode 0 only: uint8 L_r [8][h][w][D]); uint16 rawL, rawR, medL, medR [h][w];
//      uint8 final [h][w]; uint8 depth [h][w]
// Prints "sgm_ref ok, <seconds> s" (the seconds of the computation, without the file traffic).
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

typedef std::vector<uint8_t> Bytes;
typedef std::vector<uint16_t> Plane;

static int W, H, D, P1, P2;

static std::vector<uint32_t> census(const Bytes& I) {
  std::vector<uint32_t> out((size_t)W * H, 0u);
  for (int y = 3; y < H - 3; y++)
    for (int x = 4; x < W - 4; x++) {
      uint32_t f = 0;
      for (int dy = -3; dy <= 0; dy++)
        for (int dx = -4; dx <= (dy < 0 ? 4 : -1); dx++)
          f = (f << 1) | (uint32_t)(I[(size_t)(y + dy) * W + x + dx] > I[(size_t)(y - dy) * W + x - dx]);
      out[(size_t)y * W + x] = f;
    }
  return out;
}

static uint32_t cost(const std::vector<uint32_t>& cl, const std::vector<uint32_t>& cr, int x, int y, int d) {
  const uint32_t r = x - d < 0 ? 0u : cr[(size_t)y * W + x - d];
  return (uint32_t)__builtin_popcount(cl[(size_t)y * W + x] ^ r);
}

static const int DIRS[8][2] = {{1, 0}, {-1, 0}, {0, 1}, {0, -1}, {1, 1}, {-1, 1}, {-1, -1}, {1, -1}};

// L_r of one path into vol [h][w][D]: the pixels in an order in which q = p - r comes before p
static void path(const std::vector<uint32_t>& cl, const std::vector<uint32_t>& cr, int rx, int ry, Bytes& vol) {
  const bool forward = ry > 0 || (ry == 0 && rx > 0);
  const long n = (long)W * H;
  for (long i = 0; i < n; i++) {
    const long p = forward ? i : n - 1 - i;
    const int x = (int)(p % W), y = (int)(p / W), qx = x - rx, qy = y - ry;
    uint8_t* out = &vol[(size_t)p * D];
    if (qx < 0 || qx >= W || qy < 0 || qy >= H) {
      for (int d = 0; d < D; d++) out[d] = (uint8_t)cost(cl, cr, x, y, d);
      continue;
    }
    const uint8_t* prev = &vol[((size_t)qy * W + qx) * D];
    uint32_t m = prev[0];
    for (int e = 1; e < D; e++) m = prev[e] < m ? prev[e] : m;
    for (int d = 0; d < D; d++) {
      uint32_t best = (uint32_t)prev[d] - m;
      if (d - 1 >= 0 && (uint32_t)prev[d - 1] - m + P1 < best) best = (uint32_t)prev[d - 1] - m + P1;
      if (d + 1 < D && (uint32_t)prev[d + 1] - m + P1 < best) best = (uint32_t)prev[d + 1] - m + P1;
      if ((uint32_t)P2 < best) best = (uint32_t)P2;
      out[d] = (uint8_t)(cost(cl, cr, x, y, d) + best);
    }
  }
}

// the rule both winners share: the two smallest keys -> the disparity
static uint16_t decide(uint32_t k0, uint32_t k1, float uniqueness) {
  const int c0 = (int)(k0 >> 16), d0 = (int)(k0 & 0xffff), c1 = (int)(k1 >> 16), d1 = (int)(k1 & 0xffff);
  const float product = (float)c1 * uniqueness;
  if (product >= (float)c0) return (uint16_t)d0;
  if (abs(d1 - d0) <= 1) return (uint16_t)d0;
  return 0;
}

static void two_smallest(uint32_t key, uint32_t& k0, uint32_t& k1) {
  if (key < k0) { k1 = k0; k0 = key; }
  else if (key < k1) k1 = key;
}

static Plane median(const Plane& in) {
  Plane out((size_t)W * H, 0);
  for (int y = 1; y <= H - 2; y++)
    for (int x = 1; x <= W - 2; x++) {
      uint16_t v[9];
      int n = 0;
      for (int j = -1; j <= 1; j++)
        for (int i = -1; i <= 1; i++) v[n++] = in[(size_t)(y + j) * W + x + i];
      for (int a = 1; a < 9; a++)   // insertion sort
        for (int b = a; b > 0 && v[b] < v[b - 1]; b--) { const uint16_t t = v[b]; v[b] = v[b - 1]; v[b - 1] = t; }
      out[(size_t)y * W + x] = v[4];
    }
  return out;
}

template <class T>
static void put(FILE* f, const std::vector<T>& v) {
  if (fwrite(v.data(), sizeof(T), v.size(), f) != v.size()) { fprintf(stderr, "sgm_ref: short write\n"); exit(3); }
}

int main(int argc, char** argv) {
  if (argc != 3) { fprintf(stderr, "usage: sgm_ref IN OUT\n"); return 2; }
  FILE* fi = fopen(argv[1], "rb");
  if (!fi) { fprintf(stderr, "sgm_ref: cannot read %s\n", argv[1]); return 2; }
  int32_t head[6];
  float uniqueness;
  double bf[2];
  if (fread(head, 4, 6, fi) != 6 || fread(&uniqueness, 4, 1, fi) != 1 || fread(bf, 8, 2, fi) != 2) return 2;
  W = head[0]; H = head[1]; D = head[2]; P1 = head[3]; P2 = head[4];
  const int mode = head[5];
  const size_t npx = (size_t)W * H;
  Bytes left(npx), right(npx);
  if (fread(left.data(), 1, npx, fi) != npx || fread(right.data(), 1, npx, fi) != npx) return 2;
  fclose(fi);
  FILE* fo = fopen(argv[2], "wb");
  if (!fo) { fprintf(stderr, "sgm_ref: cannot write %s\n", argv[2]); return 2; }
  double seconds = 0;
  auto t0 = std::chrono::steady_clock::now();
  auto lap = [&]() { seconds += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count(); };

  const std::vector<uint32_t> cl = census(left), cr = census(right);
  lap();
  put(fo, cl); put(fo, cr);
  // the eight paths, one volume at a time, summed as they are made
  Bytes vol(npx * D);
  Plane S(npx * D, 0);
  for (int r = 0; r < 8; r++) {
    t0 = std::chrono::steady_clock::now();
    path(cl, cr, DIRS[r][0], DIRS[r][1], vol);
    for (size_t i = 0; i < npx * D; i++) S[i] = (uint16_t)(S[i] + vol[i]);
    lap();
    if (mode == 0) put(fo, vol);
  }
  t0 = std::chrono::steady_clock::now();
  Plane rawL(npx), rawR(npx);
  for (int y = 0; y < H; y++)
    for (int x = 0; x < W; x++) {
      uint32_t k0 = 0xffffffffu, k1 = 0xffffffffu;
      for (int d = 0; d < D; d++) two_smallest(((uint32_t)S[((size_t)y * W + x) * D + d] << 16) | (uint32_t)d, k0, k1);
      rawL[(size_t)y * W + x] = decide(k0, k1, uniqueness);
      k0 = k1 = 0xffffffffu;
      for (int d = 0; d < D && x + d <= W - 1; d++) two_smallest(((uint32_t)S[((size_t)y * W + x + d) * D + d] << 16) | (uint32_t)d, k0, k1);
      rawR[(size_t)y * W + x] = decide(k0, k1, uniqueness);
    }
  const Plane medL = median(rawL), medR = median(rawR);
  Bytes fin(npx), depth(npx);
  for (int y = 0; y < H; y++)
    for (int x = 0; x < W; x++) {
      int d = medL[(size_t)y * W + x];
      if (x < 16 * (W / 16) && y < 16 * (H / 16)) {
        const int k = x - d;
        bool bad = left[(size_t)y * W + x] == 0 || d <= 0;
        if (k >= 0 && k < W && abs((int)medR[(size_t)y * W + k] - d) > 1) bad = true;
        if (bad) d = 0;
      }
      fin[(size_t)y * W + x] = (uint8_t)d;
    }
  for (size_t i = 0; i < npx; i++) {
    if (fin[i] == 0) { depth[i] = 0; continue; }
    const double t = ((200.0 * bf[0]) * bf[1]) / (double)fin[i];
    depth[i] = (t > 255 || t < 0) ? 0 : (uint8_t)t;
  }
  lap();
  put(fo, rawL); put(fo, rawR); put(fo, medL); put(fo, medR); put(fo, fin); put(fo, depth);
  fclose(fo);
  printf("sgm_ref ok, %.6f s\n", seconds);
  return 0;
}
