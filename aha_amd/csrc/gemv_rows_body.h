// The batched decode matvec (kernels.h "multi-sequence decode"), once for its three weight forms: gemv_rows_kernel (bf16 weights,
// kernels_batch.hip), gemv_rows_mxfp8_kernel (kernels_gemv_rows_fp8.hip) and gemv_rows_mxfp4_kernel (kernels_gemv_rows_fp4.hip) are
// gemv_rows_body with a weight form each.  Blocks, chunks, lane roles, K splits, tail rules, MFMA sequence, LDS reduction and slab
// store are this one text, so the k permutation and the summation order of the three kernels cannot drift apart: row isolation and
// "MX output == bf16 output on W', every bit" rest on that.  A weight form says only how a lane's 32 k of one weight row in one chunk
// are loaded and how MFMA fragment j is made from what was loaded.  Below the body: the <CW, NRT> launch ladder of the three launchers,
// and what the two MX quantisers and their check kernels share.
#pragma once
#include <algorithm>

#include <hip/hip_runtime.h>

#include "attn_common.h"   // mfma16, as_frag
#include "common.h"
#include "kernels.h"

namespace aha {

typedef const __attribute__((address_space(1))) char* gcchar_t;
typedef const __attribute__((address_space(1))) uint32_t* gcu32_t;
typedef __attribute__((address_space(1))) float* gf_t;
// generic pointer -> explicitly global one (global loads / stores, never flat: see common.h gptr16_t)
template <class T>
__device__ __forceinline__ T gp(const void* p) { return reinterpret_cast<T>((uint64_t)(uintptr_t)p); }

constexpr int GR_CHUNK = 128;   // k per chunk: 4 MFMA k-steps of 32; lane group q = lane / 16 holds k q*32 .. q*32+31 of the chunk
constexpr int GR_NB = 32;       // weight rows (output columns) per block: two 16-wide MFMA column tiles

// ---- weight forms -----------------------------------------------------------------------------------------------------------
// LOADS: 16-byte loads of a lane's 32 k of one weight row; addr(r, K, k0, l): byte offset of load l for weight row r, k0 the lane's
// first k of the (clamped) chunk; SCALED: a scale word per (row, chunk) is read, byte q of it the lane's E8M0 block scale;
// frag(w, j, scale): MFMA fragment j (k0 + 8j .. + 7 as 8 bf16) from the LOADS registers.  For the MX forms a lane's 32 k are exactly
// one MX block (K % 32 == 0: a block is inside K or past it as a whole; past it, the last block is re-read), and q * 2^e is exact in
// bf16, so frag returns bit for bit what the bf16 form loads from W' = dequantised W.

// bf16 weights (N, K), 2 bytes per weight from HBM: load j is fragment j; a ragged K (K % 8 == 0) re-reads the last 8 k.
struct GemvRowsBf16 {
  static constexpr int LOADS = 4;
  static constexpr bool SCALED = false;
  static __device__ __forceinline__ int64_t addr(int64_t r, int K, int k0, int l) { return (r * K + min(k0 + l * 8, K - 8)) * 2; }
  static __device__ __forceinline__ u32x4_t frag(const u32x4_t (&w)[LOADS], int j, float) { return w[j]; }
};

// MXFP8 copy (kernels.h "MXFP8 weight copies"): one E4M3 byte per element, 1.03125 bytes per weight with the scales.  Two dwords
// (k ascending from the low byte of the first) are fragment j, each byte's value times the block scale.
struct GemvRowsMxfp8 {
  static constexpr int LOADS = 2;
  static constexpr bool SCALED = true;
  static __device__ __forceinline__ int64_t addr(int64_t r, int K, int k0, int l) { return r * K + min(k0, K - 32) + l * 16; }
  static __device__ __forceinline__ u32x4_t frag(const u32x4_t (&w)[LOADS], int j, float scale) {
    const uint32_t w0 = w[j >> 1][(j & 1) * 2], w1 = w[j >> 1][(j & 1) * 2 + 1];
    const bf16x2_t a = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(w0, scale, false);
    const bf16x2_t b = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(w0, scale, true);
    const bf16x2_t c = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(w1, scale, false);
    const bf16x2_t d = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(w1, scale, true);
    return u32x4_t{__builtin_bit_cast(uint32_t, a), __builtin_bit_cast(uint32_t, b), __builtin_bit_cast(uint32_t, c),
                   __builtin_bit_cast(uint32_t, d)};
  }
};

// MXFP4 copy (kernels.h "MXFP4 weight copies"): one E2M1 nibble per element, q rows of K / 2 bytes, 0.53125 bytes per weight with the
// scales.  Dword j of the one load (k ascending from bits 0..3) is fragment j, converted by four v_cvt_scalef32_pk_bf16_fp4, one per
// byte; the conversion returns -0.0 for the code 0x8, as W' holds it.
struct GemvRowsMxfp4 {
  static constexpr int LOADS = 1;
  static constexpr bool SCALED = true;
  static __device__ __forceinline__ int64_t addr(int64_t r, int K, int k0, int) { return r * (K / 2) + min(k0, K - 32) / 2; }
  static __device__ __forceinline__ u32x4_t frag(const u32x4_t (&w)[LOADS], int j, float scale) {
    const bf16x2_t a = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w[0][j], scale, 0);
    const bf16x2_t b = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w[0][j], scale, 1);
    const bf16x2_t c = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w[0][j], scale, 2);
    const bf16x2_t d = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w[0][j], scale, 3);
    return u32x4_t{__builtin_bit_cast(uint32_t, a), __builtin_bit_cast(uint32_t, b), __builtin_bit_cast(uint32_t, c),
                   __builtin_bit_cast(uint32_t, d)};
  }
};

// ---- the body ---------------------------------------------------------------------------------------------------------------
// One wave: columns n0 .. n0+31 (two tiles) x chunks c0 .. c0+CW-1 of K, for NRT row tiles of x.  Lane l: column / row c = l & 15 of a
// tile, k group q = l >> 4.  MFMA step j of chunk c covers k = c*128 + q*32 + j*8 .. +7 in lane group q: a fixed permutation of the k
// order, the same for W and x.  Requests are issued x(c), W(c) (and its scale words) in chunk order, all up front; the MFMAs of chunk c
// then wait only for what was requested before chunk c+1.  red: 4 * 2 * NRT * 256 floats of LDS, 16-byte aligned.
template <class WF, int CW, int NRT>
__device__ __forceinline__ void gemv_rows_body(const GemvRowsArgs& a, const void* w, const uint32_t* wscales, float* red) {
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int c = lane & 15, q = lane >> 4;
  const int n0 = blockIdx.x * GR_NB, ks = blockIdx.y;
  const int K = a.K, N = a.N, R = a.R;
  const int nchunks = (K + GR_CHUNK - 1) / GR_CHUNK;
  const int cbase = (ks * 4 + wave) * CW;
  const gcchar_t W = gp<gcchar_t>(w);
  const gcu32_t S = gp<gcu32_t>(wscales);
  const gcchar_t X = gp<gcchar_t>(a.x);
  // weight rows of this lane in the two column tiles (rows past N re-read row N-1: finite values whose outputs are never stored)
  const int64_t wr[2] = {min(n0 + c, N - 1), min(n0 + 16 + c, N - 1)};
  u32x4_t wf[CW][2][WF::LOADS], xf[CW][NRT][4];
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
#pragma unroll
    for (int l = 0; l < WF::LOADS; ++l)
#pragma unroll
      for (int nt = 0; nt < 2; ++nt)
        wf[i][nt][l] = __builtin_nontemporal_load(reinterpret_cast<gptr16_t>(W + WF::addr(wr[nt], K, chc * GR_CHUNK + q * 32, l)));
    if constexpr (WF::SCALED) {
#pragma unroll
      for (int nt = 0; nt < 2; ++nt) sw[i][nt] = __builtin_nontemporal_load(S + (wr[nt] * nchunks + chc));
    }
  }
  f32x4_t acc[2][NRT];
#pragma unroll
  for (int nt = 0; nt < 2; ++nt)
#pragma unroll
    for (int rt = 0; rt < NRT; ++rt) acc[nt][rt] = f32x4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int i = 0; i < CW; ++i) {
    float s[2] = {0.f, 0.f};
    if constexpr (WF::SCALED) {   // byte q of the chunk's scale word -> 2^e
#pragma unroll
      for (int nt = 0; nt < 2; ++nt) s[nt] = __uint_as_float(((sw[i][nt] >> (q * 8)) & 0xffu) << 23);
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const u32x4_t b[2] = {WF::frag(wf[i][0], j, s[0]), WF::frag(wf[i][1], j, s[1])};
#pragma unroll
      for (int nt = 0; nt < 2; ++nt)
#pragma unroll
        for (int rt = 0; rt < NRT; ++rt) acc[nt][rt] = mfma16(as_frag(xf[i][rt][j]), as_frag(b[nt]), acc[nt][rt]);
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

// The two launches of a gemv_rows call: the K-split plan, the grid, the <CW, NRT> instantiation kern[CW - 1][NRT - 1] (two row tiles
// above 16 rows) with the form's trailing arguments, and the merge.
template <class... Extra>
inline void launch_gemv_rows_form(void (*const (&kern)[2][2])(GemvRowsArgs, Extra...), GemvRowsArgs a, GemvEpi epi, hipStream_t st,
                                  Extra... extra) {
  if (a.R <= 0 || a.N <= 0 || a.K <= 0) return;
  a.ldws = a.N;
  int cw, nks;
  gemv_rows_plan(a.N, a.K, &cw, &nks);
  const dim3 grid((unsigned)((a.N + GR_NB - 1) / GR_NB), (unsigned)nks);
  hipLaunchKernelGGL(kern[cw - 1][a.R > 16], grid, dim3(256), 0, st, a, extra...);
  launch_gemv_rows_merge(a, epi, nks, st);
}

// ---- MX weight copies: what the MXFP8 and MXFP4 quantisers share (their element rounding is mxfp8.h / mxfp4.h) ------------------
// The quantise kernels: thread = one element, 32 consecutive lanes = one block; n_elems % 32 == 0, so a block is inside or outside as a
// whole.  The largest bf16 magnitude pattern of the thread's block:
__device__ __forceinline__ uint32_t mx_block_amax(uint32_t abs_bf16) {
  uint32_t amax = abs_bf16;
#pragma unroll
  for (int off = 16; off > 0; off >>= 1) amax = max(amax, (uint32_t)__shfl_xor((int)amax, off));
  return amax;
}

// The block's first lane stores its E8M0 byte.  Scale word layout (kernels.h): row n, chunk k / 128, byte (k / 32) % 4; a last chunk's
// missing blocks keep the buffer's 127 fill.
__device__ __forceinline__ void mx_store_scale(uint8_t* so, int64_t i, int K, int e) {
  if ((threadIdx.x & 31) != 0) return;
  const int64_t row = i / K;
  const int k = (int)(i - row * K);
  const int nchunks = (K + GR_CHUNK - 1) / GR_CHUNK;
  so[(row * nchunks + k / GR_CHUNK) * 4 + (k / 32) % 4] = (uint8_t)(e + 127);
}

// ORs 1 into *flag when a weight cannot be quantised: its bf16 magnitude pattern is at or above LIMIT (non-finite, or so large that
// its quantised value rounds past what the format's largest scale holds).
template <uint32_t LIMIT>
__device__ __forceinline__ void mx_check_body(const bf16_t* __restrict__ w, int64_t n_elems, int* flag) {
  int bad = 0;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n_elems; i += (int64_t)gridDim.x * 256)
    bad |= (uint32_t)(w[i] & 0x7fffu) >= LIMIT;
  if (bad) atomicOr(flag, 1);
}

typedef void (*mx_quantize_kernel_t)(const bf16_t*, int64_t, int, uint8_t*, uint8_t*, bf16_t*);
inline void launch_mx_quantize(mx_quantize_kernel_t kern, const void* w, int N, int K, void* q_out, uint32_t* scales_out,
                               void* w_roundtrip_out, hipStream_t st) {
  const int64_t n = (int64_t)N * K;
  if (n <= 0) return;
  (void)hipMemsetAsync(scales_out, 127, mxfp8_scale_words(N, K) * 4, st);
  hipLaunchKernelGGL(kern, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, (const bf16_t*)w, n, K, (uint8_t*)q_out,
                     (uint8_t*)scales_out, (bf16_t*)w_roundtrip_out);
}

inline void launch_mx_check(void (*kern)(const bf16_t*, int64_t, int*), const void* w, int64_t n_elems, int* flag, hipStream_t st) {
  if (n_elems <= 0) return;
  const unsigned blocks = (unsigned)std::min<int64_t>((n_elems + 255) / 256, 4096);
  hipLaunchKernelGGL(kern, dim3(blocks), dim3(256), 0, st, (const bf16_t*)w, n_elems, flag);
}

}  // namespace aha
