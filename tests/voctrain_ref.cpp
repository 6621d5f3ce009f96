// msfm_descset_voctree_train (include/msfm.h states the definitions) as a literal scalar loop: node by node, member by member,
// one thread.  Build: g++ -O2 -ffp-contract=off (no intrinsics: every binary32 operation below is one rounding).
//   voctrain_ref <in.bin> <out.bin>
// in.bin : int32 k, levels, max_iters, image_step, n_images; uint64 seed; int32 count[n_images]; float32 rows of all images
// out.bin: int32 n_blocks, k, depth, weight_shift, sum_shift, n_images (sampled); int64 n_features, n_leaves;
//          int32 level_nodes[depth], level_split[depth], level_max_iters[depth], level_capped[depth];
//          uint16 block_n[nb]; float32 node_desc[nb][k][128]; uint32 node_link[nb][k]; float32 node_weight[nb][k];
//          uint16 block_leaf[nb]; uint32 block_parent[nb]
// stdout : "voctrain_ref ok: <features> features, <blocks> blocks, <seconds> s in the training"
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <vector>

static float dist8(const float* f, const float* d) {
  float s[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  for (int i = 0; i < 128; i++) {
    const float x = f[i] - d[i];
    const float q = x * x;
    s[i % 8] = s[i % 8] + q;
  }
  const float a = s[0] + s[1], b = s[2] + s[3], c = s[4] + s[5], e = s[6] + s[7];
  const float ab = a + b, ce = c + e;
  return ab + ce;
}

static uint64_t next(uint64_t& x) {
  x += 0x9E3779B97F4A7C15ull;
  uint64_t z = x;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

static uint64_t draw(uint64_t seed, int level, int ordinal, int j) {
  uint64_t x = seed ^ 0x766F637472616E31ull;
  uint64_t h = next(x);
  x = h ^ (((uint64_t)level << 40) | (uint64_t)ordinal);
  h = next(x);
  x = h ^ (uint64_t)j;
  return next(x);
}

struct Node { std::vector<int> mem; uint32_t parent; };
struct Row { std::vector<float> desc; uint32_t link; float weight; };

int main(int argc, char** argv) {
  if (argc < 3) { std::printf("usage: voctrain_ref <in.bin> <out.bin>\n"); return 1; }
  std::ifstream in(argv[1], std::ios::binary);
  int head[5];
  uint64_t seed = 0;
  in.read((char*)head, sizeof head);
  in.read((char*)&seed, sizeof seed);
  const int k = head[0], levels = head[1], max_iters = head[2], step = head[3], n = head[4];
  std::vector<int> count(n);
  in.read((char*)count.data(), sizeof(int) * n);
  std::vector<float> X;
  int n_sampled = 0;
  for (int i = 0; i < n; i++) {
    std::vector<float> rows((size_t)count[i] * 128);
    in.read((char*)rows.data(), sizeof(float) * rows.size());
    if (i % step == 0) { X.insert(X.end(), rows.begin(), rows.end()); n_sampled++; }
  }
  if (!in) { std::printf("voctrain_ref FAILED: short input\n"); return 1; }
  const int M = (int)(X.size() / 128);
  uint32_t maxbits = 0;
  for (float v : X) {
    uint32_t b;
    std::memcpy(&b, &v, 4);
    b &= 0x7fffffffu;
    if (b > maxbits) maxbits = b;
  }
  float bound = 2896.0f;
  uint32_t bound_bits;
  std::memcpy(&bound_bits, &bound, 4);
  if (M == 0 || M > (1 << 23) || maxbits >= bound_bits || k < 2 || k > 64 || levels < 1 || levels > 32 || max_iters < 1 || step < 1) {
    std::printf("voctrain_ref REFUSED\n");
    return 2;
  }
  const int e = (int)(maxbits >> 23) - 126;
  const int wshift = 40 - (9 + 2 * e), S = 39 - e;
  const double wscale = std::ldexp(1.0, wshift), sscale = std::ldexp(1.0, S), inv = std::ldexp(1.0, -S);

  const auto t0 = std::chrono::steady_clock::now();
  std::vector<std::vector<Row>> blocks;
  std::vector<uint32_t> parents;
  std::vector<int> level_nodes, level_split, level_most, level_capped;
  std::vector<Node> nodes(1);
  nodes[0].parent = 0;
  for (int s = 0; s < M; s++) nodes[0].mem.push_back(s);
  uint32_t word = 0, base = 0;
  for (int level = 0; level < levels && !nodes.empty(); level++) {
    const int nn = (int)nodes.size();
    std::vector<Node> nxt;
    int split = 0, most = 0, capped = 0;
    for (int o = 0; o < nn; o++) {
      const std::vector<int>& mem = nodes[o].mem;
      const int m = (int)mem.size();
      std::vector<Row> blk;
      auto row_of = [&](const float* d) { Row r; r.desc.assign(d, d + 128); r.link = 0x80000000u | word++; r.weight = 1.0f; return r; };
      if (m <= k) {
        for (int i = 0; i < m; i++) blk.push_back(row_of(&X[(size_t)mem[i] * 128]));
      } else {
        // seeding
        std::vector<int> chosen(1, mem[(size_t)(draw(seed, level, o, 0) % (uint64_t)m)]);
        std::vector<float> mind(m);
        for (int j = 1; j < k; j++) {
          const float* c = &X[(size_t)chosen.back() * 128];
          uint64_t W = 0;
          std::vector<uint64_t> w(m);
          for (int i = 0; i < m; i++) {
            const float d = dist8(&X[(size_t)mem[i] * 128], c);
            if (j == 1 || d < mind[i]) mind[i] = d;
            w[i] = (uint64_t)((double)mind[i] * wscale);
            W += w[i];
          }
          if (W == 0) break;
          const uint64_t r = draw(seed, level, o, j) % W;
          uint64_t prefix = 0;
          for (int i = 0; i < m; i++) {
            prefix += w[i];
            if (prefix > r) { chosen.push_back(mem[i]); break; }
          }
        }
        const int N = (int)chosen.size();
        if (N == 1) {
          blk.push_back(row_of(&X[(size_t)chosen[0] * 128]));
        } else {
          std::vector<float> C((size_t)N * 128);
          for (int c = 0; c < N; c++) std::memcpy(&C[(size_t)c * 128], &X[(size_t)chosen[c] * 128], 512);
          std::vector<int> a(m, -1), cnt(N, 0);
          int its = 0;
          bool cap = true;
          for (int it = 1; it <= max_iters; it++) {
            bool same = true;
            for (int i = 0; i < m; i++) {
              float best = 4294967296.0f;
              int best_c = -1;
              for (int c = 0; c < N; c++) {
                const float d = dist8(&X[(size_t)mem[i] * 128], &C[(size_t)c * 128]);
                if (d < best) { best = d; best_c = c; }
              }
              if (best_c != a[i]) { a[i] = best_c; same = false; }
            }
            its = it;
            if (same) { cap = false; break; }   // the centres already are the means of this assignment
            std::vector<int64_t> sum((size_t)N * 128, 0);
            std::fill(cnt.begin(), cnt.end(), 0);
            for (int i = 0; i < m; i++) {
              cnt[a[i]]++;
              for (int d = 0; d < 128; d++) sum[(size_t)a[i] * 128 + d] += (int64_t)((double)X[(size_t)mem[i] * 128 + d] * sscale);
            }
            for (int c = 0; c < N; c++)
              if (cnt[c] > 0)
                for (int d = 0; d < 128; d++) C[(size_t)c * 128 + d] = (float)(((double)sum[(size_t)c * 128 + d] / (double)cnt[c]) * inv);
          }
          split++;
          if (its > most) most = its;
          capped += cap;
          for (int c = 0; c < N; c++) {
            if (cnt[c] == 0) continue;
            if (level == levels - 1 || cnt[c] == 1) { blk.push_back(row_of(&C[(size_t)c * 128])); continue; }
            Row r;
            r.desc.assign(&C[(size_t)c * 128], &C[(size_t)c * 128] + 128);
            r.link = base + (uint32_t)nn + (uint32_t)nxt.size();
            r.weight = 0.0f;
            blk.push_back(r);
            Node child;
            child.parent = base + (uint32_t)o;
            for (int i = 0; i < m; i++) if (a[i] == c) child.mem.push_back(mem[i]);
            nxt.push_back(child);
          }
        }
      }
      blocks.push_back(blk);
      parents.push_back(nodes[o].parent);
    }
    level_nodes.push_back(nn); level_split.push_back(split); level_most.push_back(most); level_capped.push_back(capped);
    base += (uint32_t)nn;
    nodes.swap(nxt);
  }
  const double seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();

  const int nb = (int)blocks.size(), depth = (int)level_nodes.size();
  std::ofstream out(argv[2], std::ios::binary);
  const int h[6] = {nb, k, depth, wshift, S, n_sampled};
  const int64_t h64[2] = {M, (int64_t)word};
  out.write((const char*)h, sizeof h);
  out.write((const char*)h64, sizeof h64);
  for (const auto* v : {&level_nodes, &level_split, &level_most, &level_capped}) out.write((const char*)v->data(), sizeof(int) * depth);
  std::vector<uint16_t> bn(nb), leaf(nb);
  std::vector<float> desc((size_t)nb * k * 128, 0.f), weight((size_t)nb * k, 0.f);
  std::vector<uint32_t> link((size_t)nb * k, 0);
  for (int b = 0; b < nb; b++) {
    bn[b] = (uint16_t)blocks[b].size();
    leaf[b] = 1;
    for (size_t i = 0; i < blocks[b].size(); i++) {
      std::memcpy(&desc[((size_t)b * k + i) * 128], blocks[b][i].desc.data(), 512);
      link[(size_t)b * k + i] = blocks[b][i].link;
      weight[(size_t)b * k + i] = blocks[b][i].weight;
      if (!(blocks[b][i].link & 0x80000000u)) leaf[b] = 0;
    }
  }
  out.write((const char*)bn.data(), 2 * (size_t)nb);
  out.write((const char*)desc.data(), sizeof(float) * desc.size());
  out.write((const char*)link.data(), sizeof(uint32_t) * link.size());
  out.write((const char*)weight.data(), sizeof(float) * weight.size());
  out.write((const char*)leaf.data(), 2 * (size_t)nb);
  out.write((const char*)parents.data(), sizeof(uint32_t) * (size_t)nb);
  std::printf("voctrain_ref ok: %d features, %d blocks, %.6f s in the training\n", M, nb, seconds);
  return 0;
}
