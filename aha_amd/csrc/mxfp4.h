// MXFP4 (OCP microscaling, E2M1 elements, E8M0 block scales) arithmetic of the weight quantiser, in integer / exact f32 operations that
// mean the same on the host and on the device (aha_amd/quant.py restates them in torch; tests/test_weights_fp4_*.py compare the two).
//
// A block is 32 consecutive k of one weight row.  e = the smallest integer in [-125, 125] with amax <= 6 * 2^e (an all-zero block: -125)
// -- no element saturates; not the OCP text's floor(log2 amax) - 2; scale byte = e + 127.  q = the E2M1 code (sign << 3 | index into
// {0, 0.5, 1, 1.5, 2, 3, 4, 6}) nearest to w / 2^e, a tie to the even index; the sign is kept, so 0x8 (-0) occurs.  w' = q * 2^e has two
// significant bits and |w'| >= 2^-126 or 0: exact in bf16.
#pragma once
#include "mxfp8.h"

namespace aha {

constexpr int MX4_EXP_MIN = -125, MX4_EXP_MAX = 125;
// |w| from this bf16 pattern on (one step above 1.5 * 2^127) rounds past 6 * 2^125: refused with the non-finite ones
constexpr uint32_t MX4_BF16_ABS_LIMIT = 0x7f41u;

// block exponent from the largest |w| of the block as a bf16 bit pattern (sign cleared, finite)
__host__ __device__ inline int mx4_block_exp(uint32_t amax_bf16) {
  if (amax_bf16 == 0) return MX4_EXP_MIN;
  int ex = (int)(amax_bf16 >> 7);         // biased exponent
  uint32_t man = amax_bf16 & 0x7fu;       // 7 mantissa bits
  if (ex == 0) {                          // subnormal: man * 2^-133, normalise
    ex = 1;
    while (!(man & 0x80u)) man <<= 1, --ex;
    man &= 0x7fu;
  }
  // amax = (1 + man / 128) * 2^(ex - 127); 6 = 1.5 * 2^2: amax <= 6 * 2^e  <=>  e >= ex - 129 (+ 1 when 1 + man / 128 > 1.5)
  int e = ex - 129 + (man > 0x40u ? 1 : 0);
  return e < MX4_EXP_MIN ? MX4_EXP_MIN : e > MX4_EXP_MAX ? MX4_EXP_MAX : e;
}

// |w| / 2^e of a bf16 magnitude pattern (finite, |w| <= 6 * 2^e), exact in f32 and free of f32 subnormals: |w| = M * 2^E with an 8-bit
// M, and a quotient below 2^-13 is returned as 0 (it rounds to the code 0 either way)
__host__ __device__ inline float mx4_scaled_abs(uint32_t abs_bf16, int e) {
  const int ex = (int)(abs_bf16 >> 7);
  const uint32_t M = ex ? 0x80u | (abs_bf16 & 0x7fu) : abs_bf16 & 0x7fu;
  const int sh = (ex ? ex : 1) - 134 - e;   // <= -5
  return sh < -20 ? 0.0f : (float)M * mx_exp2(sh);
}

// v in [0, 6] -> index of the nearest E2M1 magnitude; a value half way between two goes to the even index (0.25 -> 0, 0.75 -> 1,
// 1.25 -> 1, 1.75 -> 2, 2.5 -> 2, 3.5 -> 4, 5 -> 4)
__host__ __device__ inline uint32_t mx4_e2m1_index(float v) {
  return (uint32_t)(v > 0.25f) + (uint32_t)(v >= 0.75f) + (uint32_t)(v > 1.25f) + (uint32_t)(v >= 1.75f) + (uint32_t)(v > 2.5f) +
         (uint32_t)(v >= 3.5f) + (uint32_t)(v > 5.0f);
}

// E2M1 index 0..7 -> its magnitude
__host__ __device__ inline float mx4_e2m1_mag(uint32_t idx) {
  return idx < 2 ? 0.5f * (float)idx : mx_bits_f32(((126u + (idx >> 1)) << 23) | ((idx & 1u) << 22));
}

}  // namespace aha
