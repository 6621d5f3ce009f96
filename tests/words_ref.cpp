// The vocabulary-tree descent of msfm_descset_words (include/msfm.h states the semantics) as a literal scalar loop, one feature
// at a time, one thread.  Build: g++ -O2 -ffp-contract=off (no intrinsics: every operation below is one binary32 rounding).
//   words_ref <in.bin> <out.bin>
// in.bin : int32 k, n_blocks, n_images, min_features; int32 block_n[n_blocks]; float32 node_desc[n_blocks][k][128];
//          uint32 node_link[n_blocks][k]; float32 node_weight[n_blocks][k]; int32 count[n_images]; float32 rows of all images
// out.bin: int32 n_unassigned, num_words, n_bow; int32 has_words[n_images]; int32 word_id[features]; int32 image_max_id[n_images];
//          int32 bow_off[n_images + 1]; int32 bow_word[n_bow]; float32 bow_weight[n_bow]
// stdout : "words_ref ok: <features> features, <seconds> s in the descent"
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <fstream>
#include <map>
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

int main(int argc, char** argv) {
  if (argc < 3) { std::printf("usage: words_ref <in.bin> <out.bin>\n"); return 1; }
  std::ifstream in(argv[1], std::ios::binary);
  int head[4];
  in.read((char*)head, sizeof head);
  const int k = head[0], nb = head[1], n = head[2], min_features = head[3];
  std::vector<int> block_n(nb), count(n);
  std::vector<float> desc((size_t)nb * k * 128), weight((size_t)nb * k);
  std::vector<uint32_t> link((size_t)nb * k);
  in.read((char*)block_n.data(), sizeof(int) * nb);
  in.read((char*)desc.data(), sizeof(float) * desc.size());
  in.read((char*)link.data(), sizeof(uint32_t) * link.size());
  in.read((char*)weight.data(), sizeof(float) * weight.size());
  in.read((char*)count.data(), sizeof(int) * n);
  size_t total = 0;
  for (int c : count) total += (size_t)c;
  std::vector<float> rows(total * 128);
  in.read((char*)rows.data(), sizeof(float) * rows.size());
  if (!in) { std::printf("words_ref FAILED: short input\n"); return 1; }

  std::vector<int> has(n), word(total, -1), image_max(n, 0), bow_off(n + 1, 0), bow_word;
  std::vector<float> bow_weight;
  int n_un = 0, num_words = 0;
  double seconds = 0;
  size_t base = 0;
  for (int img = 0; img < n; base += (size_t)count[img], img++) {
    has[img] = count[img] > min_features;
    if (has[img]) {
      std::map<uint32_t, float> bag;
      const auto t0 = std::chrono::steady_clock::now();
      for (int f = 0; f < count[img]; f++) {
        const float* row = &rows[(base + f) * 128];
        uint32_t blk = 0;
        for (int level = 0; level < 64; level++) {
          float best = 4294967296.0f;
          int best_i = -1;
          for (int i = 0; i < block_n[blk]; i++) {
            const float d = dist8(row, &desc[((size_t)blk * k + i) * 128]);
            if (d < best) { best = d; best_i = i; }
          }
          if (best_i < 0) break;   // nothing won: no word
          const uint32_t l = link[(size_t)blk * k + best_i];
          if (l & 0x80000000u) {
            const uint32_t id = l & 0x7fffffffu;
            word[base + f] = (int)id;
            bag[id] += weight[(size_t)blk * k + best_i];
            break;
          }
          if (l == 0) break;
          blk = l;
        }
      }
      seconds += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
      for (int f = 0; f < count[img]; f++) {
        const int w = word[base + f];
        if (w < 0) n_un++;
        else if (w > image_max[img]) image_max[img] = w;
      }
      for (const auto& e : bag) { bow_word.push_back((int)e.first); bow_weight.push_back(e.second); }
      if (image_max[img] > num_words) num_words = image_max[img];
    }
    bow_off[img + 1] = (int)bow_word.size();
  }
  std::ofstream out(argv[2], std::ios::binary);
  const int tail[3] = {n_un, num_words, (int)bow_word.size()};
  out.write((const char*)tail, sizeof tail);
  out.write((const char*)has.data(), sizeof(int) * n);
  out.write((const char*)word.data(), sizeof(int) * total);
  out.write((const char*)image_max.data(), sizeof(int) * n);
  out.write((const char*)bow_off.data(), sizeof(int) * (n + 1));
  out.write((const char*)bow_word.data(), sizeof(int) * bow_word.size());
  out.write((const char*)bow_weight.data(), sizeof(float) * bow_weight.size());
  std::printf("words_ref ok: %zu features, %.6f s in the descent\n", total, seconds);
  return 0;
}
