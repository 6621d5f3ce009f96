// Sequential restatement of include/msfm.h, "Stereo rectification": geometry, maps and warp of one posed pair, written from the
// header's text and sharing no code with the library.  Build with -ffp-contract=off: every product and sum is rounded on its own.
//   rectify_ref in.bin out.bin
// in:  int32 w, h; binary64 K1[9] R1[9] t1[3] K2[9] R2[9] t2[3]; uint8 left[h][w], right[h][w]
// out: int32 refused (1: nothing else follows), idx; binary64 R1_[9] R2_[9] P1_[12] P2_[12] Q[16] t_rect[3];
//      float mapx_left, mapy_left, mapx_right, mapy_right [h][w]; uint8 left_rectified, right_rectified [h][w]
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

struct V3 { double x, y, z; };
struct M3 { double m[3][3]; };

static double dot3(double a0, double b0, double a1, double b1, double a2, double b2) { return (a0 * b0 + a1 * b1) + a2 * b2; }
static M3 mul(const M3& A, const M3& B) {
  M3 C;
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) C.m[i][j] = dot3(A.m[i][0], B.m[0][j], A.m[i][1], B.m[1][j], A.m[i][2], B.m[2][j]);
  return C;
}
static V3 mul(const M3& A, const V3& v) {
  return {dot3(A.m[0][0], v.x, A.m[0][1], v.y, A.m[0][2], v.z), dot3(A.m[1][0], v.x, A.m[1][1], v.y, A.m[1][2], v.z),
          dot3(A.m[2][0], v.x, A.m[2][1], v.y, A.m[2][2], v.z)};
}
static M3 transpose(const M3& A) {
  M3 T;
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) T.m[i][j] = A.m[j][i];
  return T;
}
static double norm(const V3& v) { return std::sqrt(dot3(v.x, v.x, v.y, v.y, v.z, v.z)); }
static M3 inverse(const M3& A) {
  const double(&a)[3][3] = A.m;
  M3 C;
  C.m[0][0] = a[1][1] * a[2][2] - a[1][2] * a[2][1];
  C.m[0][1] = a[0][2] * a[2][1] - a[0][1] * a[2][2];
  C.m[0][2] = a[0][1] * a[1][2] - a[0][2] * a[1][1];
  C.m[1][0] = a[1][2] * a[2][0] - a[1][0] * a[2][2];
  C.m[1][1] = a[0][0] * a[2][2] - a[0][2] * a[2][0];
  C.m[1][2] = a[0][2] * a[1][0] - a[0][0] * a[1][2];
  C.m[2][0] = a[1][0] * a[2][1] - a[1][1] * a[2][0];
  C.m[2][1] = a[0][1] * a[2][0] - a[0][0] * a[2][1];
  C.m[2][2] = a[0][0] * a[1][1] - a[0][1] * a[1][0];
  const double det = dot3(a[0][0], C.m[0][0], a[0][1], C.m[1][0], a[0][2], C.m[2][0]);
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) C.m[i][j] = C.m[i][j] / det;
  return C;
}
static M3 rodrigues(const V3& v) {
  M3 R = {{{1, 0, 0}, {0, 1, 0}, {0, 0, 1}}};
  const double th = norm(v);
  if (th == 0) return R;
  const double c = std::cos(th), s = std::sin(th), c1 = 1.0 - c;
  const double k[3] = {v.x / th, v.y / th, v.z / th};
  const double skew[3][3] = {{0, -k[2], k[1]}, {k[2], 0, -k[0]}, {-k[1], k[0], 0}};
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) R.m[i][j] = (c * R.m[i][j] + (c1 * k[i]) * k[j]) + s * skew[i][j];
  return R;
}

struct Geometry { M3 R1, R2; double P1[3][4], P2[3][4], Q[4][4]; V3 trect; int idx; };

static bool finite_all(const double* v, int n) {
  for (int i = 0; i < n; i++)
    if (!std::isfinite(v[i])) return false;
  return true;
}

static bool geometry(const M3& K1, const M3& R1, const V3& t1, const M3& K2, const M3& R2, const V3& t2, int w, int h, Geometry& g) {
  if (w < 1 || w > 16384 || h < 1 || h > 16384) return false;
  if (!finite_all(&K1.m[0][0], 9) || !finite_all(&R1.m[0][0], 9) || !finite_all(&t1.x, 3)) return false;
  if (!finite_all(&K2.m[0][0], 9) || !finite_all(&R2.m[0][0], 9) || !finite_all(&t2.x, 3)) return false;
  if (!(K1.m[0][0] > 0) || !(K1.m[1][1] > 0) || !(K2.m[0][0] > 0) || !(K2.m[1][1] > 0)) return false;
  const M3 R21 = mul(R2, inverse(R1));
  const V3 rt = mul(R21, t1);
  const V3 t21 = {-rt.x + t2.x, -rt.y + t2.y, -rt.z + t2.z};
  if (!finite_all(&R21.m[0][0], 9) || !finite_all(&t21.x, 3)) return false;
  double c = (((R21.m[0][0] + R21.m[1][1]) + R21.m[2][2]) - 1.0) * 0.5;
  if (c > 1.0) c = 1.0;
  if (c < -1.0) c = -1.0;
  const double theta = std::acos(c);
  if (M_PI - theta < 1e-6) return false;
  const V3 r = {(R21.m[2][1] - R21.m[1][2]) * 0.5, (R21.m[0][2] - R21.m[2][0]) * 0.5, (R21.m[1][0] - R21.m[0][1]) * 0.5};
  const double s = norm(r);
  V3 om = {0, 0, 0};
  if (s != 0) {
    const double f = theta / s;
    om = {r.x * f, r.y * f, r.z * f};
  }
  const M3 rr = rodrigues({-0.5 * om.x, -0.5 * om.y, -0.5 * om.z});
  const V3 t = mul(rr, t21);
  const double tv[3] = {t.x, t.y, t.z};
  const int idx = std::fabs(tv[0]) > std::fabs(tv[1]) ? 0 : 1;
  const double cidx = tv[idx], nt = norm(t);
  if (!(nt > 0)) return false;
  double uu[3] = {0, 0, 0};
  uu[idx] = cidx > 0 ? 1.0 : -1.0;
  V3 ww = {tv[1] * uu[2] - tv[2] * uu[1], tv[2] * uu[0] - tv[0] * uu[2], tv[0] * uu[1] - tv[1] * uu[0]};
  const double nw = norm(ww);
  if (nw > 0) {
    const double f = std::acos(std::fabs(cidx) / nt) / nw;
    ww = {ww.x * f, ww.y * f, ww.z * f};
  }
  const M3 wR = rodrigues(ww);
  g.R1 = mul(wR, transpose(rr));
  g.R2 = mul(wR, rr);
  g.trect = mul(g.R2, t21);
  const double trv[3] = {g.trect.x, g.trect.y, g.trect.z};
  const int o = idx ^ 1;
  const double fc = K1.m[o][o] < K2.m[o][o] ? K1.m[o][o] : K2.m[o][o];
  double cc[2][2];
  for (int k = 0; k < 2; k++) {
    const M3& K = k ? K2 : K1;
    const M3& R = k ? g.R2 : g.R1;
    double sx = 0, sy = 0;
    const double xs[4] = {0.0, (double)(w - 1), 0.0, (double)(w - 1)}, ys[4] = {0.0, 0.0, (double)(h - 1), (double)(h - 1)};
    for (int q = 0; q < 4; q++) {
      const V3 p = mul(R, V3{(xs[q] - K.m[0][2]) / K.m[0][0], (ys[q] - K.m[1][2]) / K.m[1][1], 1.0});
      sx = sx + (p.x / p.z) * fc;
      sy = sy + (p.y / p.z) * fc;
    }
    cc[k][0] = (w - 1) * 0.5 - sx * 0.25;
    cc[k][1] = (h - 1) * 0.5 - sy * 0.25;
  }
  const double ccx = (cc[0][0] + cc[1][0]) * 0.5, ccy = (cc[0][1] + cc[1][1]) * 0.5;
  const double P[3][4] = {{fc, 0, ccx, 0}, {0, fc, ccy, 0}, {0, 0, 1, 0}};
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 4; j++) g.P1[i][j] = g.P2[i][j] = P[i][j];
  g.P2[idx][3] = trv[idx] * fc;
  const double Q[4][4] = {{1, 0, 0, -ccx}, {0, 1, 0, -ccy}, {0, 0, 0, fc}, {0, 0, -1.0 / trv[idx], 0}};
  for (int i = 0; i < 4; i++)
    for (int j = 0; j < 4; j++) g.Q[i][j] = Q[i][j];
  g.idx = idx;
  return finite_all(&g.R1.m[0][0], 9) && finite_all(&g.R2.m[0][0], 9) && finite_all(&g.P1[0][0], 12) && finite_all(&g.P2[0][0], 12) &&
         finite_all(&g.Q[0][0], 16);
}

static void maps(const double P[3][4], const M3& R, const M3& K, int w, int h, float* mapx, float* mapy) {
  M3 A;
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) A.m[i][j] = P[i][j];
  const M3 iR = inverse(mul(A, R));
  const double fx = K.m[0][0], fy = K.m[1][1], cx = K.m[0][2], cy = K.m[1][2];
  for (int i = 0; i < h; i++)
    for (int j = 0; j < w; j++) {
      const double X = (iR.m[0][0] * j + iR.m[0][1] * i) + iR.m[0][2];
      const double Y = (iR.m[1][0] * j + iR.m[1][1] * i) + iR.m[1][2];
      const double W = (iR.m[2][0] * j + iR.m[2][1] * i) + iR.m[2][2];
      const double wi = 1.0 / W;
      mapx[(size_t)i * w + j] = (float)(fx * (X * wi) + cx);
      mapy[(size_t)i * w + j] = (float)(fy * (Y * wi) + cy);
    }
}

static int tap(const uint8_t* src, int w, int h, int x, int y) { return (x >= 0 && x < w && y >= 0 && y < h) ? src[(size_t)y * w + x] : 0; }

static void warp(const uint8_t* src, int w, int h, const float* mapx, const float* mapy, uint8_t* out) {
  for (size_t n = 0; n < (size_t)w * h; n++) {
    const float px = mapx[n] * 32.0f, py = mapy[n] * 32.0f;
    out[n] = 0;
    if (!std::isfinite(px) || !std::isfinite(py) || std::fabs(px) >= 1073741824.0f || std::fabs(py) >= 1073741824.0f) continue;
    const int sx = (int)std::nearbyintf(px), sy = (int)std::nearbyintf(py);   // (the default rounding mode: half to even)
    const int ix = sx >> 5, iy = sy >> 5, ax = sx & 31, ay = sy & 31;
    const int S = (32 - ax) * (32 - ay) * tap(src, w, h, ix, iy) + ax * (32 - ay) * tap(src, w, h, ix + 1, iy) +
                  (32 - ax) * ay * tap(src, w, h, ix, iy + 1) + ax * ay * tap(src, w, h, ix + 1, iy + 1);
    out[n] = (uint8_t)((S + 512) >> 10);
  }
}

template <class T>
static bool rd(FILE* f, T* p, size_t n) { return fread(p, sizeof(T), n, f) == n; }
template <class T>
static bool wr(FILE* f, const T* p, size_t n) { return fwrite(p, sizeof(T), n, f) == n; }

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* fi = fopen(argv[1], "rb");
  if (!fi) return 2;
  int32_t wh[2];
  M3 K[2], R[2];
  V3 t[2];
  bool ok = rd(fi, wh, 2);
  for (int k = 0; ok && k < 2; k++) ok = rd(fi, &K[k].m[0][0], 9) && rd(fi, &R[k].m[0][0], 9) && rd(fi, &t[k].x, 3);
  const int w = wh[0], h = wh[1];
  if (!ok || w < 0 || h < 0) return 2;
  const size_t npx = (size_t)w * h;
  std::vector<uint8_t> img(2 * npx), out(2 * npx);
  ok = rd(fi, img.data(), 2 * npx);
  fclose(fi);
  if (!ok) return 2;
  FILE* fo = fopen(argv[2], "wb");
  if (!fo) return 2;
  Geometry g;
  const int32_t refused = geometry(K[0], R[0], t[0], K[1], R[1], t[1], w, h, g) ? 0 : 1;
  double seconds = 0;
  ok = wr(fo, &refused, 1);
  if (!refused) {
    const int32_t idx = g.idx;
    ok = ok && wr(fo, &idx, 1) && wr(fo, &g.R1.m[0][0], 9) && wr(fo, &g.R2.m[0][0], 9) && wr(fo, &g.P1[0][0], 12) && wr(fo, &g.P2[0][0], 12) &&
         wr(fo, &g.Q[0][0], 16) && wr(fo, &g.trect.x, 3);
    std::vector<float> map(4 * npx);
    const auto t0 = std::chrono::steady_clock::now();
    maps(g.P1, g.R1, K[0], w, h, map.data(), map.data() + npx);
    maps(g.P2, g.R2, K[1], w, h, map.data() + 2 * npx, map.data() + 3 * npx);
    warp(img.data(), w, h, map.data(), map.data() + npx, out.data());
    warp(img.data() + npx, w, h, map.data() + 2 * npx, map.data() + 3 * npx, out.data() + npx);
    seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    ok = ok && wr(fo, map.data(), 4 * npx) && wr(fo, out.data(), 2 * npx);
  }
  if (fclose(fo) != 0 || !ok) return 3;
  printf("rectify_ref ok, %.6f s maps and warp, refused %d\n", seconds, (int)refused);
  return 0;
}
