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
#include "gemv_fp8_launch.h"

namespace aha {

namespace {

template <int R, int U, int EPI, bool FAST, int PRO>
__global__ __launch_bounds__(GEMV_THREADS) void gemv_mxfp8_kernel(const void* q, const uint8_t* scales, const void* x, const void* norm_w, void* y,
                                                                  const void* residual, int N, int K, GemvCopyTailArgs t) {
  extern __shared__ __attribute__((aligned(16))) float xs[];  // K f32 + 8 floats reduction scratch
  GemvArgs a{};
  a.W = q; a.scales = scales; a.x = x; a.norm_w = norm_w; a.residual = residual; a.y = y;
  a.y_f32 = t.y_f32; a.blk_max = t.blk_max; a.blk_idx = t.blk_idx; a.h_out = t.h_out; a.N = N; a.K = K; a.eps = t.eps;
  gemv_fp8_body<GemvWFp8, R, U, EPI, FAST, PRO>(a, xs, (int)blockIdx.x, t.nblk);
}

struct Fp8Kernels {
  template <int R, int U, int EPI, bool FAST, int PRO>
  static constexpr auto get() { return &gemv_mxfp8_kernel<R, U, EPI, FAST, PRO>; }
};

constexpr int FP8_LOADS = 16;   // 8-byte weight loads per wave and buffer (and as many scale bytes)

GemvFp8Plan plan_gemv_mxfp8(int N, int K, GemvEpi epi) { return plan_gemv_mx(N, K, epi, FP8_LOADS); }

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

void debug_plan_gemv_mxfp8(int N, int K, GemvEpi epi, bool has_norm, int* out5) { debug_plan_out(plan_gemv_mxfp8(N, K, epi), K, has_norm, out5); }

void launch_gemv_mxfp8(const GemvArgs& g, const void* q, const uint32_t* scales, GemvEpi epi, hipStream_t st) {
  if (g.N <= 0 || g.K <= 0) return;
  launch_mx<Fp8Kernels>(g, q, scales, epi, plan_gemv_mxfp8(g.N, g.K, epi), st);
}

}  // namespace aha
