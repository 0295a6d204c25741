// Batched decode matvec from MXFP8 weights (kernels.h "MXFP8 weight copies"; model_quantize_weights, model.hip).
//
//   gemv_rows_mxfp8_kernel   gemv_rows_body (gemv_rows_body.h) with the GemvRowsMxfp8 weight form: every output bit equals gemv_rows on
//                            W' = dequantised W (tests/test_weights_fp8_gpu.py).  Writes the same f32 slabs: the launch ends in
//                            gemv_rows_merge_kernel, unchanged.
//   mxfp8_quantize_kernel    bf16 W -> q bytes, scale words, W' (may overwrite W): one 32-lane max per block.
//   mxfp8_check_kernel       ORs 1 into a flag when a weight cannot be quantised (non-finite, or so large that it rounds past bf16).
#include "gemv_rows_body.h"
#include "mxfp8.h"

namespace aha {

namespace {

template <int CW, int NRT>
__global__ __launch_bounds__(256, 2) void gemv_rows_mxfp8_kernel(GemvRowsArgs a, const void* wq, const uint32_t* wscales) {
  __shared__ __attribute__((aligned(16))) float red[4 * 2 * NRT * 256];
  gemv_rows_body<GemvRowsMxfp8, CW, NRT>(a, wq, wscales, red);
}

// wr may be w (a thread reads its element before it writes it; no other thread touches it).
__global__ __launch_bounds__(256) void mxfp8_quantize_kernel(const bf16_t* w, int64_t n_elems, int K, uint8_t* __restrict__ qo,
                                                             uint8_t* __restrict__ so, bf16_t* wr) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n_elems) return;
  const bf16_t b = w[i];
  const int e = mx_block_exp(mx_block_amax(b & 0x7fffu));
  // w * 2^-e is exact; a product below f32's normal range is below half of E4M3's smallest subnormal with or without flushing
  const float v = bf2f(b) * mx_exp2(-e);
  const uint32_t code = mx_e4m3_rne(v);
  qo[i] = (uint8_t)code;
  if (wr) {
    const float r = mx_e4m3_f32(code) * mx_exp2(e);
    wr[i] = (bf16_t)(__float_as_uint(r) >> 16);   // exact: at most 4 significant bits, |r| >= 2^-126 or 0
  }
  mx_store_scale(so, i, K, e);
}

__global__ __launch_bounds__(256) void mxfp8_check_kernel(const bf16_t* __restrict__ w, int64_t n_elems, int* flag) {
  mx_check_body<MX_BF16_ABS_LIMIT>(w, n_elems, flag);
}

}  // namespace

size_t mxfp8_scale_words(int N, int K) { return (size_t)N * ((K + GR_CHUNK - 1) / GR_CHUNK); }

void launch_gemv_rows_mxfp8(const GemvRowsArgs& a, const void* wq, const uint32_t* wscales, GemvEpi epi, hipStream_t st) {
  static constexpr void (*kern[2][2])(GemvRowsArgs, const void*, const uint32_t*) = {
      {gemv_rows_mxfp8_kernel<1, 1>, gemv_rows_mxfp8_kernel<1, 2>}, {gemv_rows_mxfp8_kernel<2, 1>, gemv_rows_mxfp8_kernel<2, 2>}};
  launch_gemv_rows_form(kern, a, epi, st, wq, wscales);
}

void launch_mxfp8_quantize(const void* w, int N, int K, void* q_out, uint32_t* scales_out, void* w_roundtrip_out, hipStream_t st) {
  launch_mx_quantize(mxfp8_quantize_kernel, w, N, K, q_out, scales_out, w_roundtrip_out, st);
}

void launch_mxfp8_check(const void* w, int64_t n_elems, int* flag, hipStream_t st) { launch_mx_check(mxfp8_check_kernel, w, n_elems, flag, st); }

}  // namespace aha
