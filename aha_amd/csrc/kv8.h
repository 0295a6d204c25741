// KV8 element arithmetic on the device: one (token, kv head) vector of 128 dims -> 128 E4M3 codes and one E8M0 scale byte, with mxfp8.h's
// exponent and rounding.  Shared by the page quantiser, the append kernel (kernels_attn_kv8.hip) and the KV8 form of the fused decode
// attention (attn_decode_body.h); aha_amd/quant.py quantize_kv restates it in torch.
#pragma once
#include "common.h"
#include "mxfp8.h"

namespace aha {

// Selections below are sign masks ((int)(x - y) >> 31), not compares: a compare's result is a scalar register pair, and a quantiser that
// converts 64 elements per lane runs out of them.
__device__ __forceinline__ uint32_t kv8_lt_mask(uint32_t x, uint32_t y) { return (uint32_t)((int32_t)(x - y) >> 31); }   // x < y (both < 2^31): ~0

// What a bf16 bit pattern contributes to its block's maximum: NaN nothing, +-Inf and what 2^120 cannot scale into E4M3's range the
// largest magnitude that survives (the activation row quantiser's rule, kernels_gemm_fp8.hip).
__device__ __forceinline__ uint32_t kv8_amax_term(uint32_t bits) {
  const uint32_t a = bits & 0x7fffu;
  return min(a, MX_BF16_ABS_LIMIT - 1) & ~kv8_lt_mask(0x7f80u, a);
}
// mx_e4m3_rne with both of its paths computed and one selected, the round-up as an add
__device__ __forceinline__ uint32_t kv8_e4m3_rne(float v) {
  const uint32_t u = __float_as_uint(v), sign = (u >> 24) & 0x80u, a = u & 0x7fffffffu;
  const uint32_t subn = __float_as_uint(__uint_as_float(a) * 512.0f + 8388608.0f) & 0xfu;   // |v| < 2^-6: multiples of 2^-9
  const uint32_t norm = ((a + 0x7ffffu + ((a >> 20) & 1u)) >> 20) - ((127u - 7u) << 3);       // nearest, a tie to the even code
  const uint32_t m = kv8_lt_mask(a, 0x3c800000u);
  return sign | (subn & m) | (norm & ~m);
}
// E4M3 code of a bf16 bit pattern under the block's 2^-e
__device__ __forceinline__ uint32_t kv8_code(uint32_t bits, float inv) {
  const uint32_t a = bits & 0x7fffu, sign = (bits >> 8) & 0x80u;
  const uint32_t special = ~kv8_lt_mask(a, MX_BF16_ABS_LIMIT);   // saturates, or NaN
  // w * 2^-e is exact; a product below f32's normal range is below half of E4M3's smallest subnormal with or without flushing.
  // A special element goes through as +0 (code 0) and its code is or-ed in.
  const uint32_t fin = kv8_e4m3_rne(bf2f((bf16_t)(bits & ~special)) * inv);
  return fin | (special & (sign | 0x7eu | (kv8_lt_mask(0x7f80u, a) & 1u)));
}
// code * 2^e as a bf16 bit pattern: exact (at most 4 significant bits, 2^-126 <= |r| < 2^128 or 0); the NaN code gives a quiet NaN
__device__ __forceinline__ bf16_t kv8_dequant(uint32_t code, int e) {
  const uint32_t r = __float_as_uint(mx_e4m3_f32(code) * mx_exp2(e)) >> 16;
  return (bf16_t)((code & 0x7fu) == 0x7fu ? ((code & 0x80u) << 8) | 0x7fc0u : r);
}
// mx_block_exp without its branches and its normalising loop (they cost the kernels scalar registers for the saved exec masks): a
// subnormal or zero maximum has a biased exponent of 0 and ends at MX_EXP_MIN through the clamp, as there
__device__ __forceinline__ int kv8_block_exp(uint32_t amax_bf16) {
  const int e = (int)(amax_bf16 >> 7) - 135 + ((amax_bf16 & 0x7fu) > 0x60u ? 1 : 0);
  return max(MX_EXP_MIN, min(MX_EXP_MAX, e));
}
// 2^e of an E8M0 scale byte the quantiser wrote (10 .. 247); the byte 0 of a zeroed page gives 0, 0xff gives +Inf (softmax_tile_kv8
// clamps V's; K's only meets a score that the mask then replaces)
__device__ __forceinline__ float kv8_scale_f32(uint32_t byte) { return __uint_as_float(byte << 23); }
// maximum over the 64 lanes of values below 2^24 (exact as f32)
__device__ __forceinline__ uint32_t kv8_wave_max(uint32_t v) { return (uint32_t)wave_max((float)v); }

// One 8-byte piece of a KV8 fragment (two dwords, element 0 in the low byte of the first) -> the bf16 MFMA operand: the code values
// themselves (scale 1, |q| <= 448 exact in bf16); the block scales ride the scores (K) and the probabilities (V), attn_common.h.
__device__ __forceinline__ bf16x8_t kv8_frag(uint32_t w0, uint32_t w1) {
  const bf16x2_t a = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(w0, 1.0f, false);
  const bf16x2_t b = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(w0, 1.0f, true);
  const bf16x2_t c = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(w1, 1.0f, false);
  const bf16x2_t d = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(w1, 1.0f, true);
  union { u32x4_t u; bf16x8_t f; } x;
  x.u = u32x4_t{__builtin_bit_cast(uint32_t, a), __builtin_bit_cast(uint32_t, b), __builtin_bit_cast(uint32_t, c), __builtin_bit_cast(uint32_t, d)};
  return x.f;
}

}  // namespace aha
