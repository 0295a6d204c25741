// Batched decode matvec from MXFP4 weights (kernels.h "MXFP4 weight copies"; model_quantize_weights, model.hip).
//
//   gemv_rows_mxfp4_kernel   gemv_rows_body (gemv_rows_body.h) with the GemvRowsMxfp4 weight form: every output bit equals gemv_rows on
//                            W' = dequantised W (tests/test_weights_fp4_gpu.py).  Writes the same f32 slabs: the launch ends in
//                            gemv_rows_merge_kernel, unchanged.
//   mxfp4_quantize_kernel    bf16 W -> q nibbles, scale words, W' (may overwrite W): one 32-lane max per block, two lanes per byte.
//   mxfp4_check_kernel       ORs 1 into a flag when a weight cannot be quantised (non-finite, or above 1.5 * 2^127 in magnitude).
#include "gemv_rows_body.h"
#include "mxfp4.h"

namespace aha {

namespace {

template <int CW, int NRT>
__global__ __launch_bounds__(256, 2) void gemv_rows_mxfp4_kernel(GemvRowsArgs a, const void* wq, const uint32_t* wscales) {
  __shared__ __attribute__((aligned(16))) float red[4 * 2 * NRT * 256];
  gemv_rows_body<GemvRowsMxfp4, CW, NRT>(a, wq, wscales, red);
}

// Two neighbouring lanes = one byte (the even-k lane stores it).  wr may be w (a thread reads its element before anything is written; no
// other thread touches it).
__global__ __launch_bounds__(256) void mxfp4_quantize_kernel(const bf16_t* w, int64_t n_elems, int K, uint8_t* __restrict__ qo,
                                                             uint8_t* __restrict__ so, bf16_t* wr) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n_elems) return;
  const bf16_t b = w[i];
  const uint32_t abs = b & 0x7fffu;
  const int e = mx4_block_exp(mx_block_amax(abs));
  const uint32_t idx = mx4_e2m1_index(mx4_scaled_abs(abs, e));
  const uint32_t code = ((uint32_t)(b >> 12) & 8u) | idx;     // the sign is kept: a negative weight that rounds to 0 gives 0x8 (-0)
  const uint32_t other = (uint32_t)__shfl_xor((int)code, 1);  // K is even: the neighbour belongs to the same row
  if ((threadIdx.x & 1) == 0) qo[i >> 1] = (uint8_t)(code | (other << 4));
  if (wr) {
    const float r = mx4_e2m1_mag(idx) * mx_exp2(e);           // exact: two significant bits, r >= 2^-126 or 0
    wr[i] = (bf16_t)((__float_as_uint(r) >> 16) | (b & 0x8000u));
  }
  mx_store_scale(so, i, K, e);
}

__global__ __launch_bounds__(256) void mxfp4_check_kernel(const bf16_t* __restrict__ w, int64_t n_elems, int* flag) {
  mx_check_body<MX4_BF16_ABS_LIMIT>(w, n_elems, flag);
}

}  // namespace

void launch_gemv_rows_mxfp4(const GemvRowsArgs& a, const void* wq, const uint32_t* wscales, GemvEpi epi, hipStream_t st) {
  static constexpr void (*kern[2][2])(GemvRowsArgs, const void*, const uint32_t*) = {
      {gemv_rows_mxfp4_kernel<1, 1>, gemv_rows_mxfp4_kernel<1, 2>}, {gemv_rows_mxfp4_kernel<2, 1>, gemv_rows_mxfp4_kernel<2, 2>}};
  launch_gemv_rows_form(kern, a, epi, st, wq, wscales);
}

void launch_mxfp4_quantize(const void* w, int N, int K, void* q_out, uint32_t* scales_out, void* w_roundtrip_out, hipStream_t st) {
  launch_mx_quantize(mxfp4_quantize_kernel, w, N, K, q_out, scales_out, w_roundtrip_out, st);
}

void launch_mxfp4_check(const void* w, int64_t n_elems, int* flag, hipStream_t st) { launch_mx_check(mxfp4_check_kernel, w, n_elems, flag, st); }

}  // namespace aha
