// Driver for tests/test_gpu_epnpf_host.py: reads images (int32 n, int32 sizes[n], then per image f_estimated, X[N][3], x[N][2] as
// doubles) from argv[1], runs the host mirror's AbsolutePoseWithoutFocalLengthBatch (host/objectsfm.cc; reference
// absolute_pose_estimation.cc:28-40) and writes per image f_out, R[9], t[3], avg_error, errors[N] to argv[2].
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
  std::vector<std::vector<Vec3>> pw(n);
  std::vector<std::vector<Vec2>> p2(n);
  std::vector<double> f_est(n);
  for (int p = 0; p < n; p++) {
    if (std::fread(&f_est[p], 8, 1, in) != 1) return 2;
    pw[p].resize(sizes[p]); p2[p].resize(sizes[p]);
    for (auto& X : pw[p]) if (std::fread(X.v, 8, 3, in) != 3) return 2;
    for (auto& x : p2[p]) { double b[2]; if (std::fread(b, 8, 2, in) != 2) return 2; x.x = b[0]; x.y = b[1]; }
  }
  std::fclose(in);
  std::vector<double> f_out, avg;
  std::vector<RTPose> poses;
  std::vector<std::vector<double>> errs;
  AbsolutePoseWithoutFocalLengthBatch(pw, p2, f_est, f_out, poses, errs, avg);
  FILE* out = std::fopen(argv[2], "wb");
  if (!out) return 2;
  for (int p = 0; p < n; p++) {
    std::fwrite(&f_out[p], 8, 1, out);
    std::fwrite(poses[p].R.m, 8, 9, out);
    std::fwrite(poses[p].t.v, 8, 3, out);
    std::fwrite(&avg[p], 8, 1, out);
    std::fwrite(errs[p].data(), 8, errs[p].size(), out);
  }
  std::fclose(out);
  std::printf("epnpf_host_check ok: %d images\n", n);
  return 0;
}
