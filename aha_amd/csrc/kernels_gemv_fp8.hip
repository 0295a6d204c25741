// Batch-1 matvec from MXFP8 weights: the single-sequence decode step of a quantised model (kernels.h "MXFP8 weight copies").
//
//   y[n] = sum_k h[k] * (q[n,k] * 2^e[n, k / 32])     q (N,K) E4M3 bytes row-major, e the E8M0 block scales, h (K) bf16, f32 accumulate
//
// gemv_mxfp8_kernel is gemv_kernel (kernels_gemv.hip) with another weight load: per 512-k chunk a lane reads its 8 k as ONE 8-byte
// non-temporal load plus the scale byte of its MX block (four lanes share a block), and v_cvt_scalef32_pk_f32_fp8 turns two bytes into two
// f32 with the scale folded in.  q * 2^e is exact in f32 and is bit for bit what lo_bf / hi_bf give on W' = dequantised W; lane -> k map,
// fma order, wave reduction and the epilogues' rounding points are gemv_body's, so every output bit equals gemv_kernel on W'
// (tests/test_weights_fp8_single_gpu.py), whatever R, U or grid either plan picks.
//
// Scales: one byte load per (row, chunk) and lane, non-temporal like the weights -- as many load instructions again, 1/32 more bytes; the 64
// lanes touch 16 consecutive bytes, one request to the memory pipeline.  The loads are half as wide as the bf16 kernel's, so the plan below
// keeps R * U * NW = 16 of them per buffer where the shape allows (two rows per wave where the bf16 plan takes one).
#include <stdlib.h>

#include "gemv_fp8_body.h"

namespace aha {

namespace {

// What is first used behind the first weight request travels here (kernels_gemv.hip has the reasoning): the 14 leading dwords are q, scales,
// x, norm_w, y, the residual vector, N and K; eps is first used in the prologue and the grid size for a block's second tile.
struct GemvFp8TailArgs {
  float* y_f32;
  float* blk_max;
  uint32_t* blk_idx;
  void* h_out;
  float eps;
  int nblk;
};

template <int R, int U, int EPI, bool FAST, int PRO>
__global__ __launch_bounds__(GEMV_THREADS) void gemv_mxfp8_kernel(const void* q, const uint8_t* scales, const void* x, const void* norm_w, void* y,
                                                                  const void* residual, int N, int K, GemvFp8TailArgs t) {
  extern __shared__ __attribute__((aligned(16))) float xs[];  // K f32 + 8 floats reduction scratch
  GemvFp8Args a;
  a.q = q; a.scales = scales; a.x = x; a.norm_w = norm_w; a.residual = residual; a.y = y;
  a.y_f32 = t.y_f32; a.blk_max = t.blk_max; a.blk_idx = t.blk_idx; a.h_out = t.h_out; a.N = N; a.K = K; a.eps = t.eps;
  gemv_fp8_body<R, U, EPI, FAST, PRO>(a, xs, (int)blockIdx.x, t.nblk);
}

struct GemvFp8Plan { int R, U, grid; };

constexpr int FP8_LOADS = 16;   // 8-byte weight loads per wave and buffer (and as many scale bytes)

// N: output rows (GEMV_SILU_MUL: I).  Rows per wave so that there are at least 512 tiles (two per CU), then as many chunks per item as
// keep R * U * NW = 16 loads, at most 8 and at most the row's chunks (a power of two).
GemvFp8Plan plan_gemv_mxfp8(int N, int K, GemvEpi epi) {
  const int nchunks = (K + 511) / 512;
  const int nw = epi == GEMV_SILU_MUL ? 2 : 1;
  int R = 4;
  while (R > 1 && (N + 4 * R - 1) / (4 * R) < 512) R >>= 1;
  if (nw == 2 && R > 2) R = 2;
  int U = std::min(std::min(FP8_LOADS / (R * nw), 8), nchunks);
  int Up = 1;
  while (Up * 2 <= U) Up *= 2;
  // persistent blocks: 3 per CU on 256 CUs, as plan_gemv (the 16-load instantiations take 160 .. 169 VGPRs: 12 waves per CU, which with
  // two buffers of 16 half-KiB requests each is the bytes in flight of the bf16 kernel's 8-load plans)
  const int gmax = 768;
  const int ntiles = (N + 4 * R - 1) / (4 * R);
  int grid = std::min(ntiles, gmax);
  // whole rounds, as plan_gemv: the largest grid in [gmax / 2, gmax] that divides the tile count, multiples of 8 only
  if (ntiles > gmax) {
    for (int g = gmax; g >= gmax / 2; g -= 8)
      if (ntiles % g == 0) {
        grid = g;
        break;
      }
  }
  return {R, Up, std::max(grid, 1)};
}

// the forms launch_gemv_mxfp8 takes for a shape: FAST = every chunk group full; PRO = the straight-line prologue
void form_of(const GemvFp8Plan& p, int K, bool has_norm, bool* fast, int* pro) {
  *fast = K % (512 * p.U) == 0;
  *pro = *fast && K <= (has_norm ? 4 : 8) * 8 * GEMV_THREADS ? (has_norm ? 2 : 1) : 0;
}

template <int EPI>
void launch_epi(const GemvFp8Args& a, const GemvFp8Plan& p, hipStream_t st) {
  const size_t lds = (size_t)((a.K + 511) / 512) * 512 * 4 + 64;
  dim3 grid(p.grid), block(GEMV_THREADS);
  bool fast;
  int pro;
  form_of(p, a.K, a.norm_w != nullptr, &fast, &pro);
  const GemvFp8TailArgs t{a.y_f32, a.blk_max, a.blk_idx, a.h_out, a.eps, p.grid};
#define GV_(RR, UU, FF, PP) \
  hipLaunchKernelGGL((gemv_mxfp8_kernel<RR, UU, EPI, FF, PP>), grid, block, lds, st, a.q, a.scales, a.x, a.norm_w, a.y, a.residual, a.N, a.K, t)
  // U at the plan's cap (the row has at least 2 * U chunks or exactly U): every form
#define GV_FULL(RR, UU)                                                                 \
  do {                                                                                  \
    if (pro == 2) GV_(RR, UU, true, 2); else if (pro == 1) GV_(RR, UU, true, 1);        \
    else if (fast) GV_(RR, UU, true, 0); else GV_(RR, UU, false, 0);                    \
  } while (0)
  // U below the cap: the row has fewer than 2 * U chunks, so a FAST shape is K = 512 * U <= 2048 and always straight-line
#define GV_SHORT(RR, UU)                                                                \
  do {                                                                                  \
    if (pro == 2) GV_(RR, UU, true, 2); else if (pro == 1) GV_(RR, UU, true, 1);        \
    else GV_(RR, UU, false, 0);                                                         \
  } while (0)
  constexpr int NW = EPI == GEMV_SILU_MUL ? 2 : 1;
  if (p.R == 4) {
    if constexpr (NW == 1) {
      if (p.U >= 4) GV_FULL(4, 4); else if (p.U == 2) GV_SHORT(4, 2); else GV_SHORT(4, 1);
    }
  } else if (p.R == 2) {
    if constexpr (NW == 1) {
      if (p.U >= 8) GV_FULL(2, 8); else if (p.U == 4) GV_SHORT(2, 4); else if (p.U == 2) GV_SHORT(2, 2); else GV_SHORT(2, 1);
    } else {
      if (p.U >= 4) GV_FULL(2, 4); else if (p.U == 2) GV_SHORT(2, 2); else GV_SHORT(2, 1);
    }
  } else {
    if (p.U >= 8) GV_FULL(1, 8); else if (p.U == 4) GV_SHORT(1, 4); else if (p.U == 2) GV_SHORT(1, 2); else GV_SHORT(1, 1);
  }
#undef GV_SHORT
#undef GV_FULL
#undef GV_
}

}  // namespace

// Which matrices the model hands to this kernel: those of at least 2^24 elements whose launch takes the FAST form.  Measured per matrix on
// an MI355X (profiles/weights_fp8_single.md; the rule: FP8's p90 below bf16's p10): every Qwen3-8B decode matrix wins, the smallest being
// o_proj's 4096 x 4096 = 2^24, all of them FAST; of Qwen3-0.6B's only lm_head does -- its layer matrices (2 .. 6 M elements) run 4 .. 6 us
// in either kernel, launch-bound, and down_proj (K = 3072: six chunks in items of four, the general form with its predicated loads) is
// slower.  Nothing between 6.3 M and 16.8 M elements was measured, so the line sits at the smallest measured win; no large general-form
// shape was measured either, and the one measured general-form launch lost, so such a shape stays on bf16.  N: matrix rows (gate+up: 2I).
bool gemv_mxfp8_by_plan(int N, int K, GemvEpi epi) {
  if ((int64_t)N * K < ((int64_t)1 << 24)) return false;
  const GemvFp8Plan p = plan_gemv_mxfp8(epi == GEMV_SILU_MUL ? N / 2 : N, K, epi);
  return K % (512 * p.U) == 0;
}

int gemv_mxfp8_num_tiles(int N, int K) { return plan_gemv_mxfp8(N, K, GEMV_LOGITS).grid; }

void debug_plan_gemv_mxfp8(int N, int K, GemvEpi epi, bool has_norm, int* out5) {
  const GemvFp8Plan p = plan_gemv_mxfp8(N, K, epi);
  bool fast;
  int pro;
  form_of(p, K, has_norm, &fast, &pro);
  out5[0] = p.R; out5[1] = p.U; out5[2] = p.grid; out5[3] = fast ? 1 : 0; out5[4] = pro;
}

void launch_gemv_mxfp8(const GemvArgs& g, const void* q, const uint32_t* scales, GemvEpi epi, hipStream_t st) {
  if (g.N <= 0 || g.K <= 0) return;
  GemvFp8Args a{};
  a.q = q; a.scales = (const uint8_t*)scales; a.x = g.x; a.norm_w = g.norm_w; a.residual = g.residual; a.y = g.y; a.y_f32 = g.y_f32;
  a.blk_max = g.blk_max; a.blk_idx = g.blk_idx; a.h_out = g.h_out; a.N = g.N; a.K = g.K; a.eps = g.eps;
  const GemvFp8Plan p = plan_gemv_mxfp8(a.N, a.K, epi);
  switch (epi) {
    case GEMV_STORE: launch_epi<GEMV_STORE>(a, p, st); break;
    case GEMV_RESIDUAL: launch_epi<GEMV_RESIDUAL>(a, p, st); break;
    case GEMV_SILU_MUL: launch_epi<GEMV_SILU_MUL>(a, p, st); break;
    case GEMV_LOGITS: launch_epi<GEMV_LOGITS>(a, p, st); break;
    default: abort();   // GEMV_PARTIAL_F32: sharded models have no copies
  }
}

}  // namespace aha
