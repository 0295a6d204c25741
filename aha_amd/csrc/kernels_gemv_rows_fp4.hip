// Batched decode matvec from MXFP4 weights (kernels.h "MXFP4 weight copies"; model_quantize_weights, model.hip).
//
//   gemv_rows_mxfp4_kernel   gemv_rows_kernel (kernels_batch.hip) with the weight operand read as one E2M1 nibble per element plus one E8M0
//                            scale per 32 k: 0.53125 bytes per weight from HBM instead of 2.  Same blocks, chunks, lane roles, K splits,
//                            MFMA sequence and LDS reduction; a lane's 32 k of one column in one chunk are exactly one MX block, so it
//                            issues one 16-byte load where the MXFP8 kernel issues two and the bf16 kernel four.  Dword j of the load is
//                            fragment j (8 k), converted by four v_cvt_scalef32_pk_bf16_fp4 (one per byte) with the block scale folded
//                            in.  q * 2^e is exact in bf16 (the conversion returns -0.0 for the code 0x8), so the MFMA operands are bit
//                            for bit those the bf16 kernel loads from W' = dequantised W, the accumulation order is the same, and every
//                            output bit equals gemv_rows on W' (tests/test_weights_fp4_gpu.py).  Writes the same f32 slabs: the launch
//                            ends in gemv_rows_merge_kernel, unchanged.
//   mxfp4_quantize_kernel    bf16 W -> q nibbles, scale words, W' (may overwrite W): one 32-lane max per block, two lanes per byte.
//   mxfp4_check_kernel       ORs 1 into a flag when a weight cannot be quantised (non-finite, or above 1.5 * 2^127 in magnitude).
#include <hip/hip_runtime.h>

#include "attn_common.h"   // mfma16, as_frag
#include "common.h"
#include "kernels.h"
#include "mxfp4.h"

namespace aha {

namespace {

typedef const __attribute__((address_space(1))) char* gcchar_t;
typedef const __attribute__((address_space(1))) uint32_t* gcu32_t;
typedef __attribute__((address_space(1))) float* gf_t;
template <class T>
__device__ __forceinline__ T gp(const void* p) { return reinterpret_cast<T>((uint64_t)(uintptr_t)p); }

constexpr int GR_CHUNK = 128;   // as in kernels_batch.hip
constexpr int GR_NB = 32;

// 8 E2M1 nibbles (k ascending from bits 0..3 of w) -> the MFMA fragment of 8 bf16, each nibble's value times `scale` (a power of two)
__device__ __forceinline__ u32x4_t mx4_frag(uint32_t w, float scale) {
  const bf16x2_t a = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w, scale, 0);
  const bf16x2_t b = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w, scale, 1);
  const bf16x2_t c = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w, scale, 2);
  const bf16x2_t d = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w, scale, 3);
  return u32x4_t{__builtin_bit_cast(uint32_t, a), __builtin_bit_cast(uint32_t, b), __builtin_bit_cast(uint32_t, c),
                 __builtin_bit_cast(uint32_t, d)};
}

template <int CW, int NRT>
__global__ __launch_bounds__(256, 2) void gemv_rows_mxfp4_kernel(GemvRowsArgs a, const void* wq, const uint32_t* wscales) {
  __shared__ __attribute__((aligned(16))) float red[4 * 2 * NRT * 256];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int c = lane & 15, q = lane >> 4;
  const int n0 = blockIdx.x * GR_NB, ks = blockIdx.y;
  const int K = a.K, N = a.N, R = a.R;
  const int nchunks = (K + GR_CHUNK - 1) / GR_CHUNK;
  const int cbase = (ks * 4 + wave) * CW;
  const gcchar_t Q = gp<gcchar_t>(wq);
  const gcu32_t S = gp<gcu32_t>(wscales);
  const gcchar_t X = gp<gcchar_t>(a.x);
  // weight rows of this lane in the two column tiles (rows past N re-read row N-1: finite values whose outputs are never stored)
  const int r0 = min(n0 + c, N - 1), r1 = min(n0 + 16 + c, N - 1);
  const int64_t wr0 = (int64_t)r0 * (K / 2), wr1 = (int64_t)r1 * (K / 2);   // q rows are K / 2 bytes
  const int64_t sr0 = (int64_t)r0 * nchunks, sr1 = (int64_t)r1 * nchunks;
  u32x4_t wf[CW][2], xf[CW][NRT][4];
  uint32_t sw[CW][2];
#pragma unroll
  for (int i = 0; i < CW; ++i) {
    const int ch = cbase + i;
    const int chc = min(ch, nchunks - 1);   // waves past the end of K re-read the last chunk; their x is zero
#pragma unroll
    for (int rt = 0; rt < NRT; ++rt) {
      const int row = rt * 16 + c;
      const int64_t xr = (int64_t)min(row, R - 1) * a.ldx;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int k = ch * GR_CHUNK + q * 32 + j * 8;
        const int kc = min(chc * GR_CHUNK + q * 32 + j * 8, K - 8);
        u32x4_t v = *reinterpret_cast<gptr16_t>(X + (xr + kc) * 2);
        if (row >= R || k >= K) v = u32x4_t{0u, 0u, 0u, 0u};
        xf[i][rt][j] = v;
      }
    }
    // the lane's MX block of the chunk, 16 bytes (K % 32 == 0: a block is inside K or past it as a whole; past it, the last block is
    // re-read)
    const int kb = min(chc * GR_CHUNK + q * 32, K - 32);
    wf[i][0] = __builtin_nontemporal_load(reinterpret_cast<gptr16_t>(Q + (wr0 + kb / 2)));
    wf[i][1] = __builtin_nontemporal_load(reinterpret_cast<gptr16_t>(Q + (wr1 + kb / 2)));
    sw[i][0] = __builtin_nontemporal_load(S + (sr0 + chc));
    sw[i][1] = __builtin_nontemporal_load(S + (sr1 + chc));
  }
  f32x4_t acc[2][NRT];
#pragma unroll
  for (int nt = 0; nt < 2; ++nt)
#pragma unroll
    for (int rt = 0; rt < NRT; ++rt) acc[nt][rt] = f32x4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int i = 0; i < CW; ++i) {
    // byte q of the chunk's scale word -> 2^e
    const float s0 = __uint_as_float(((sw[i][0] >> (q * 8)) & 0xffu) << 23), s1 = __uint_as_float(((sw[i][1] >> (q * 8)) & 0xffu) << 23);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const u32x4_t b0 = mx4_frag(wf[i][0][j], s0);
      const u32x4_t b1 = mx4_frag(wf[i][1][j], s1);
#pragma unroll
      for (int nt = 0; nt < 2; ++nt)
#pragma unroll
        for (int rt = 0; rt < NRT; ++rt) acc[nt][rt] = mfma16(as_frag(xf[i][rt][j]), as_frag(nt ? b1 : b0), acc[nt][rt]);
    }
  }
  // lane l holds out[row (l>>4)*4 + e][col l & 15] of each (column tile, row tile)
#pragma unroll
  for (int nt = 0; nt < 2; ++nt)
#pragma unroll
    for (int rt = 0; rt < NRT; ++rt)
#pragma unroll
      for (int e = 0; e < 4; ++e) red[((wave * 2 + nt) * NRT + rt) * 256 + (q * 4 + e) * 16 + c] = acc[nt][rt][e];
  __syncthreads();
  // ((w0 + w1) + w2) + w3, then the f32 partial of this K split: ws[ks][row][n]
  gf_t ws = gp<gf_t>(a.ws) + (int64_t)ks * a.R * a.ldws;
  for (int e = tid; e < 2 * NRT * 256; e += 256) {
    const int nt = e / (NRT * 256), rt = (e / 256) % NRT, m = (e >> 4) & 15, n = e & 15;
    float s = red[e];
#pragma unroll
    for (int w = 1; w < 4; ++w) s += red[w * 2 * NRT * 256 + e];
    const int row = rt * 16 + m, col = n0 + nt * 16 + n;
    if (row < R && col < N) ws[(int64_t)row * a.ldws + col] = s;
  }
}

// Thread = one element, 32 consecutive lanes = one block, two neighbouring lanes = one byte (the even-k lane stores it).  wr may be w (a
// thread reads its element before anything is written; no other thread touches it).
__global__ __launch_bounds__(256) void mxfp4_quantize_kernel(const bf16_t* w, int64_t n_elems, int K, uint8_t* __restrict__ qo,
                                                             uint8_t* __restrict__ so, bf16_t* wr) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;   // n_elems % 32 == 0: a block is inside or outside as a whole
  if (i >= n_elems) return;
  const bf16_t b = w[i];
  const uint32_t abs = b & 0x7fffu;
  uint32_t amax = abs;
#pragma unroll
  for (int off = 16; off > 0; off >>= 1) amax = max(amax, (uint32_t)__shfl_xor((int)amax, off));
  const int e = mx4_block_exp(amax);
  const uint32_t idx = mx4_e2m1_index(mx4_scaled_abs(abs, e));
  const uint32_t code = ((uint32_t)(b >> 12) & 8u) | idx;     // the sign is kept: a negative weight that rounds to 0 gives 0x8 (-0)
  const uint32_t other = (uint32_t)__shfl_xor((int)code, 1);  // K is even: the neighbour belongs to the same row
  if ((threadIdx.x & 1) == 0) qo[i >> 1] = (uint8_t)(code | (other << 4));
  if (wr) {
    const float r = mx4_e2m1_mag(idx) * mx_exp2(e);           // exact: two significant bits, r >= 2^-126 or 0
    wr[i] = (bf16_t)((__float_as_uint(r) >> 16) | (b & 0x8000u));
  }
  if ((threadIdx.x & 31) == 0) {
    // scale word layout (kernels.h): row n, chunk k / 128, byte (k / 32) % 4; a last chunk's missing blocks keep the buffer's 127 fill
    const int64_t row = i / K;
    const int k = (int)(i - row * K);
    const int nchunks = (K + 127) / 128;
    so[(row * nchunks + k / 128) * 4 + (k / 32) % 4] = (uint8_t)(e + 127);
  }
}

__global__ __launch_bounds__(256) void mxfp4_check_kernel(const bf16_t* __restrict__ w, int64_t n_elems, int* flag) {
  int bad = 0;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n_elems; i += (int64_t)gridDim.x * 256)
    bad |= (uint32_t)(w[i] & 0x7fffu) >= MX4_BF16_ABS_LIMIT;
  if (bad) atomicOr(flag, 1);
}

}  // namespace

void launch_gemv_rows_mxfp4(const GemvRowsArgs& a0, const void* wq, const uint32_t* wscales, GemvEpi epi, hipStream_t st) {
  if (a0.R <= 0 || a0.N <= 0 || a0.K <= 0) return;
  GemvRowsArgs a = a0;
  a.W = nullptr;
  a.ldws = a.N;
  int cw, nks;
  gemv_rows_plan(a.N, a.K, &cw, &nks);
  const dim3 grid((unsigned)((a.N + GR_NB - 1) / GR_NB), (unsigned)nks);
  const bool two = a.R > 16;
  if (cw == 2) {
    if (two) hipLaunchKernelGGL((gemv_rows_mxfp4_kernel<2, 2>), grid, dim3(256), 0, st, a, wq, wscales);
    else hipLaunchKernelGGL((gemv_rows_mxfp4_kernel<2, 1>), grid, dim3(256), 0, st, a, wq, wscales);
  } else {
    if (two) hipLaunchKernelGGL((gemv_rows_mxfp4_kernel<1, 2>), grid, dim3(256), 0, st, a, wq, wscales);
    else hipLaunchKernelGGL((gemv_rows_mxfp4_kernel<1, 1>), grid, dim3(256), 0, st, a, wq, wscales);
  }
  launch_gemv_rows_merge(a, epi, nks, st);
}

void launch_mxfp4_quantize(const void* w, int N, int K, void* q_out, uint32_t* scales_out, void* w_roundtrip_out, hipStream_t st) {
  const int64_t n = (int64_t)N * K;
  if (n <= 0) return;
  (void)hipMemsetAsync(scales_out, 127, mxfp8_scale_words(N, K) * 4, st);
  hipLaunchKernelGGL(mxfp4_quantize_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, (const bf16_t*)w, n, K, (uint8_t*)q_out,
                     (uint8_t*)scales_out, (bf16_t*)w_roundtrip_out);
}

void launch_mxfp4_check(const void* w, int64_t n_elems, int* flag, hipStream_t st) {
  if (n_elems <= 0) return;
  const unsigned blocks = (unsigned)std::min<int64_t>((n_elems + 255) / 256, 4096);
  hipLaunchKernelGGL(mxfp4_check_kernel, dim3(blocks), dim3(256), 0, st, (const bf16_t*)w, n_elems, flag);
}

}  // namespace aha
