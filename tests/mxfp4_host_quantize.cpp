// Host run of the quantiser arithmetic in aha_amd/csrc/mxfp4.h, block by block as mxfp4_quantize_kernel does it
// (tests/test_weights_fp4_cpu.py compiles this and compares its output with aha_amd/quant.py).
//   argv[1]: int32 N, int32 K, then N * K bf16 patterns        argv[2]: q (N * K / 2 bytes), scale bytes (N * K / 32), W' (N * K bf16)
#include <stdio.h>

#include <vector>

#include "mxfp4.h"

using namespace aha;

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 3;
  int32_t N = 0, K = 0;
  if (fread(&N, 4, 1, f) != 1 || fread(&K, 4, 1, f) != 1 || N < 1 || K < 32 || K % 32) return 4;
  std::vector<uint16_t> w((size_t)N * K), wr((size_t)N * K);
  if (fread(w.data(), 2, w.size(), f) != w.size()) return 5;
  fclose(f);
  std::vector<uint8_t> q(w.size() / 2), s(w.size() / 32);
  for (size_t b = 0; b < s.size(); ++b) {
    uint32_t amax = 0, codes[32];
    for (int j = 0; j < 32; ++j) {
      const uint32_t a = w[b * 32 + j] & 0x7fffu;
      if (a > amax) amax = a;
    }
    const int e = mx4_block_exp(amax);
    s[b] = (uint8_t)(e + 127);
    for (int j = 0; j < 32; ++j) {
      const uint16_t x = w[b * 32 + j];
      const uint32_t idx = mx4_e2m1_index(mx4_scaled_abs(x & 0x7fffu, e));
      codes[j] = ((uint32_t)(x >> 12) & 8u) | idx;
      wr[b * 32 + j] = (uint16_t)((mx_f32_bits(mx4_e2m1_mag(idx) * mx_exp2(e)) >> 16) | (x & 0x8000u));
    }
    for (int j = 0; j < 32; j += 2) q[(b * 32 + j) / 2] = (uint8_t)(codes[j] | (codes[j + 1] << 4));
  }
  f = fopen(argv[2], "wb");
  if (!f) return 6;
  fwrite(q.data(), 1, q.size(), f);
  fwrite(s.data(), 1, s.size(), f);
  fwrite(wr.data(), 2, wr.size(), f);
  fclose(f);
  return 0;
}
