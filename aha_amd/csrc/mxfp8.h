// MXFP8 (OCP microscaling, E4M3 elements, E8M0 block scales) arithmetic of the weight quantiser, in integer / exact f32 operations that
// mean the same on the host and on the device (aha_amd/quant.py restates them in torch; tests/test_weights_fp8_*.py compare the two).
//
// A block is 32 consecutive k of one weight row.  e = the smallest integer in [-117, 120] with amax <= 448 * 2^e (an all-zero block: -117);
// scale byte = e + 127; q = e4m3fn(w / 2^e), round to nearest even (|w / 2^e| <= 448: no saturation, never the NaN code 0x7f / 0xff);
// w' = q * 2^e, at most 4 significant bits and |w'| >= 2^-126 or 0: exact in bf16.
#pragma once
#include <stdint.h>

#ifndef __HIPCC__
#define __host__
#define __device__
#endif

namespace aha {

constexpr int MX_BLOCK = 32;
constexpr int MX_EXP_MIN = -117, MX_EXP_MAX = 120;
// |w| from this bf16 pattern on (1.9375 * 2^127) rounds to 256 * 2^120 = 2^128, which bf16 does not hold: refused with the non-finite ones
constexpr uint32_t MX_BF16_ABS_LIMIT = 0x7f78u;

__host__ __device__ inline float mx_bits_f32(uint32_t u) {
  union { uint32_t u; float f; } x;
  x.u = u;
  return x.f;
}
__host__ __device__ inline uint32_t mx_f32_bits(float f) {
  union { uint32_t u; float f; } x;
  x.f = f;
  return x.u;
}

// block exponent from the largest |w| of the block as a bf16 bit pattern (sign cleared, finite)
__host__ __device__ inline int mx_block_exp(uint32_t amax_bf16) {
  if (amax_bf16 == 0) return MX_EXP_MIN;
  int ex = (int)(amax_bf16 >> 7);         // biased exponent
  uint32_t man = amax_bf16 & 0x7fu;       // 7 mantissa bits
  if (ex == 0) {                          // subnormal: man * 2^-133, normalise
    ex = 1;
    while (!(man & 0x80u)) man <<= 1, --ex;
    man &= 0x7fu;
  }
  // amax = (1 + man / 128) * 2^(ex - 127); 448 = 1.75 * 2^8: amax <= 448 * 2^e  <=>  e >= ex - 135 (+ 1 when 1 + man / 128 > 1.75)
  int e = ex - 135 + (man > 0x60u ? 1 : 0);
  return e < MX_EXP_MIN ? MX_EXP_MIN : e > MX_EXP_MAX ? MX_EXP_MAX : e;
}

// 2^e as f32 for e in [-126, 127]
__host__ __device__ inline float mx_exp2(int e) { return mx_bits_f32((uint32_t)(e + 127) << 23); }

// f32 (|v| <= 448) -> OCP e4m3fn byte, round to nearest even
__host__ __device__ inline uint32_t mx_e4m3_rne(float v) {
  const uint32_t u = mx_f32_bits(v), sign = (u >> 24) & 0x80u, a = u & 0x7fffffffu;
  if (a < 0x3c800000u) {                  // |v| < 2^-6: the subnormal grid, multiples of 2^-9 (a tie goes to the even multiple)
    // |v| * 2^9 + 2^23 rounds to an integer in f32's default mode (nearest even); f32 subnormal inputs end at 0 with or without flushing
    const float t = mx_bits_f32(a) * 512.0f + 8388608.0f;
    return sign | (mx_f32_bits(t) & 0xfu);   // 0 .. 8 (8 = 0x08: the smallest normal)
  }
  const uint32_t keep = a >> 20, rem = a & 0xfffffu;   // exponent | 3 mantissa bits
  const uint32_t up = (rem > 0x80000u || (rem == 0x80000u && (keep & 1u))) ? 1u : 0u;
  return sign | (keep + up - ((127u - 7u) << 3));       // a carry out of the mantissa bumps the exponent
}

// OCP e4m3fn byte (not a NaN code) -> f32, exact
__host__ __device__ inline float mx_e4m3_f32(uint32_t b) {
  const uint32_t ex = (b >> 3) & 0xfu, man = b & 7u;
  const float mag = ex ? mx_bits_f32(((ex + 120u) << 23) | (man << 20)) : (float)man * 0.001953125f;
  return (b & 0x80u) ? -mag : mag;
}

}  // namespace aha
