// Driver for tests/test_gpu_relposef_host.py: reads pairs (int32 n, int32 sizes[n], then per pair x_ref[N][2], x_cur[N][2] as
// doubles) from argv[1], runs the host mirror's RelativePoseWithoutFocalLengthBatch and, on every pair by itself,
// RelativePoseEstimation::RelativePoseWithoutFocalLength (host/objectsfm.cc; reference relative_pose_estimation.cc:29-83), and
// writes per pair ok, f_ref, f_cur, R[9], t[3] of the batch form, then the same of the single form, to argv[2].  The single
// form starts from f = -1 and a pose of -1s, which it must leave alone when it returns false.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "objectsfm.h"

using namespace objectsfm;

int main(int argc, char** argv) {
  if (argc < 3) return 2;
  FILE* in = std::fopen(argv[1], "rb");
  if (!in) return 2;
  int32_t n = 0;
  if (std::fread(&n, 4, 1, in) != 1) return 2;
  std::vector<int32_t> sizes(n);
  if (n && std::fread(sizes.data(), 4, n, in) != (size_t)n) return 2;
  std::vector<std::vector<Vec2>> pa(n), pb(n);
  for (int p = 0; p < n; p++) {
    pa[p].resize(sizes[p]); pb[p].resize(sizes[p]);
    for (auto& x : pa[p]) { double b[2]; if (std::fread(b, 8, 2, in) != 2) return 2; x.x = b[0]; x.y = b[1]; }
    for (auto& x : pb[p]) { double b[2]; if (std::fread(b, 8, 2, in) != 2) return 2; x.x = b[0]; x.y = b[1]; }
  }
  std::fclose(in);
  std::vector<double> f1, f2;
  std::vector<RTPoseRelative> poses;
  std::vector<uint8_t> ok;
  RelativePoseWithoutFocalLengthBatch(pa, pb, f1, f2, poses, ok);
  FILE* out = std::fopen(argv[2], "wb");
  if (!out) return 2;
  for (int p = 0; p < n; p++) {
    const double good = ok[p];
    std::fwrite(&good, 8, 1, out);
    std::fwrite(&f1[p], 8, 1, out);
    std::fwrite(&f2[p], 8, 1, out);
    std::fwrite(poses[p].R.m, 8, 9, out);
    std::fwrite(poses[p].t.v, 8, 3, out);
  }
  for (int p = 0; p < n; p++) {
    double g1 = -1.0, g2 = -1.0;
    RTPoseRelative pose;
    for (int k = 0; k < 9; k++) pose.R.m[k] = -1.0;
    for (int k = 0; k < 3; k++) pose.t[k] = -1.0;
    const double good = RelativePoseEstimation::RelativePoseWithoutFocalLength(pa[p], pb[p], g1, g2, pose) ? 1.0 : 0.0;
    std::fwrite(&good, 8, 1, out);
    std::fwrite(&g1, 8, 1, out);
    std::fwrite(&g2, 8, 1, out);
    std::fwrite(pose.R.m, 8, 9, out);
    std::fwrite(pose.t.v, 8, 3, out);
  }
  std::fclose(out);
  std::printf("relposef_host_check ok: %d pairs\n", n);
  return 0;
}
