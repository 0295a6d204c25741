// Batch-1 matvec from MXFP4 weights: the single-sequence decode step of a model with E2M1 copies (kernels.h "MXFP4 weight copies").
//
//   y[n] = sum_k h[k] * (q[n,k] * 2^e[n, k / 32])     q (N,K/2) bytes of two E2M1 codes, e the E8M0 block scales, h (K) bf16, f32 accumulate
//
// gemv_mxfp4_kernel is gemv_mxfp8_kernel (kernels_gemv_fp8.hip) with the other weight form of the one body (gemv_fp8_body.h GemvWFp4): per
// 512-k chunk a lane reads its 8 k as ONE 4-byte non-temporal load -- the bytes mxfp4_quantize_kernel writes, the even k of a byte in bits
// 0..3, no second layout -- plus the scale byte of its MX block, and v_cvt_scalef32_pk_f32_fp4 turns byte 0..3 of the dword (op_sel) into
// two f32 with the scale folded in.  code * 2^e has two significant bits and a magnitude of at least 2^-126 or zero: exact in f32, 0x8 gives
// -0.0, bit for bit what lo_bf / hi_bf give on W'.  Everything else is the body's, so every output bit equals gemv_kernel on W'
// (tests/test_weights_fp4_single_gpu.py), whatever R, U or grid either plan picks.
//
// Plan: the direct form, FP8's with loads half as wide again -- R * U * NW = 16 dword loads and 16 scale bytes per buffer.  Two buffers of
// 32 + 32 would not fit under the 6-bit vmcnt a wave counts its outstanding vector-memory operations in.
#include "gemv_fp8_launch.h"

namespace aha {

namespace {

template <int R, int U, int EPI, bool FAST, int PRO>
__global__ __launch_bounds__(GEMV_THREADS) void gemv_mxfp4_kernel(const void* q, const uint8_t* scales, const void* x, const void* norm_w, void* y,
                                                                  const void* residual, int N, int K, GemvCopyTailArgs t) {
  extern __shared__ __attribute__((aligned(16))) float xs[];  // K f32 + 8 floats reduction scratch
  GemvArgs a{};
  a.W = q; a.scales = scales; a.x = x; a.norm_w = norm_w; a.residual = residual; a.y = y;
  a.y_f32 = t.y_f32; a.blk_max = t.blk_max; a.blk_idx = t.blk_idx; a.h_out = t.h_out; a.N = N; a.K = K; a.eps = t.eps;
  gemv_fp8_body<GemvWFp4, R, U, EPI, FAST, PRO>(a, xs, (int)blockIdx.x, t.nblk);
}

struct Fp4Kernels {
  template <int R, int U, int EPI, bool FAST, int PRO>
  static constexpr auto get() { return &gemv_mxfp4_kernel<R, U, EPI, FAST, PRO>; }
};

constexpr int FP4_LOADS = 16;   // 4-byte weight loads per wave and buffer (and as many scale bytes)

GemvFp8Plan plan_gemv_mxfp4(int N, int K, GemvEpi epi) { return plan_gemv_mx(N, K, epi, FP4_LOADS); }

}  // namespace

// Which matrices the model hands to this kernel: those of at least 2^24 elements whose launch takes the FAST form, the FP8 kernel's line.
// Measured per matrix on an MI355X against the bf16 kernel on W' (profiles/weights_fp4_single.md; the rule: FP4's p90 below bf16's p10):
// every Qwen3-8B decode matrix wins (1.46x o_proj .. 2.75x lm_head), the smallest being o_proj's 4096 x 4096 = 2^24, all of them FAST; of
// Qwen3-0.6B's only lm_head does -- its layer matrices (2 .. 6 M elements) run 3 .. 5 us in either kernel and their distributions overlap,
// and down_proj (K = 3072, the general form) is slower.  Nothing between 6.3 M and 16.8 M elements was measured, so the line sits at the
// smallest measured win; no large general-form shape was measured, so such a shape stays on bf16.  N: matrix rows (gate+up: 2I).
bool gemv_mxfp4_by_plan(int N, int K, GemvEpi epi) {
  if ((int64_t)N * K < ((int64_t)1 << 24)) return false;
  const GemvFp8Plan p = plan_gemv_mxfp4(epi == GEMV_SILU_MUL ? N / 2 : N, K, epi);
  return K % (512 * p.U) == 0;
}

int gemv_mxfp4_num_tiles(int N, int K) { return plan_gemv_mxfp4(N, K, GEMV_LOGITS).grid; }

void debug_plan_gemv_mxfp4(int N, int K, GemvEpi epi, bool has_norm, int* out5) { debug_plan_out(plan_gemv_mxfp4(N, K, epi), K, has_norm, out5); }

void launch_gemv_mxfp4(const GemvArgs& g, const void* q, const uint32_t* scales, GemvEpi epi, hipStream_t st) {
  if (g.N <= 0 || g.K <= 0) return;
  launch_mx<Fp4Kernels>(g, q, scales, epi, plan_gemv_mxfp4(g.N, g.K, epi), st);
}

}  // namespace aha
