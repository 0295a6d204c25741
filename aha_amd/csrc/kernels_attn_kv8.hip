// Decode attention over an E4M3 KV cache ("KV8"; format: kernels.h, page layout: common.h "KV8 page layout", arithmetic: kv8.h).
//
//   kv_pages_quantize_kernel      bf16 pages -> KV8 pages, one block per (page, kv head, layer): the prompt's pages after the prefill.
//   attn_decode_batch_kv8_kernel  attn_decode_batch_kernel (kernels_batch.hip) over KV8 pages: attn_decode_fused_body<.., KV8 = true>
//                                 with the same row table, split rule, partial publication, arrival counter and final merge.
//   attn_decode_rows_kv8_kernel   the same without the append (draft-and-verify steps), behind
//   kv_append_rows_kv8_kernel     the k-norm + RoPE + quantise + append of every row in a launch of its own: the bytes the fused append writes.
//
// What the format buys is bytes: a page of one kv head is 16 512 B instead of 32 768 B, in the same 1 KB wave loads.  What it costs is
// vector work: 4 v_cvt_scalef32_pk_bf16_fp8 per MFMA operand (128 per page and wave next to its 48 MFMAs) and 32 scale multiplies in the
// softmax.  The MFMAs, their order and the f32 accumulators are the bf16 kernel's, and code * 2^e is exact in bf16, so the output is what
// the bf16 kernel gives over the dequantised cache up to the order of the power-of-two scalings (exact).
#include <hip/hip_runtime.h>

#include "attn_decode_body.h"
#include "common.h"
#include "kernels.h"
#include "kv8.h"

namespace aha {

namespace {

typedef const __attribute__((address_space(1))) bf16_t* gcbf_t;
typedef const __attribute__((address_space(1))) float* gcf_t;
typedef const __attribute__((address_space(1))) int32_t* gci32_t;
typedef const __attribute__((address_space(1))) uint64_t* gcu64_t;
typedef __attribute__((address_space(1))) uint8_t* gu8_t;
typedef __attribute__((address_space(1))) u32x4_t* gst16_t;
typedef __attribute__((ext_vector_type(2))) uint32_t u32x2_t;
typedef __attribute__((address_space(1))) u32x2_t* gst8_t;
template <class T>
__device__ __forceinline__ T gp(const void* p) { return reinterpret_cast<T>((uint64_t)(uintptr_t)p); }

__device__ __forceinline__ uint32_t umax(uint32_t a, uint32_t b) { return a > b ? a : b; }
// element i (0..7) of a 16-byte bf16 piece
__device__ __forceinline__ uint32_t piece_elem(const u32x4_t& v, int i) { return (v[i >> 1] >> ((i & 1) * 16)) & 0xffffu; }
// the 8 codes of a piece under 2^-e = inv(i) of element i, element 0 in the low byte of .x
template <typename InvFn>
__device__ __forceinline__ u32x2_t piece_codes(const u32x4_t& v, InvFn inv) {
  uint32_t w[2] = {0u, 0u};
#pragma unroll
  for (int i = 0; i < 8; ++i) w[i >> 2] |= kv8_code(piece_elem(v, i), inv(i)) << ((i & 3) * 8);
  return u32x2_t{w[0], w[1]};
}

// Block (page, kv head, layer), 4 waves, no LDS: every wave owns whole blocks of the format.
//   waves 0, 1: K of token sub-tiles 2w, 2w + 1.  The four k4 fragments of a sub-tile are four 16-byte loads per lane (the attention's own);
//               lane (G, c) holds 32 of token sub*16 + c's dims, the token's maximum is taken over them and then across the four lane
//               groups; two converted fragments side by side are one 16-byte store per lane, 1 KB per wave.
//   waves 2, 3: V of token slots kk*32 .. +32, kk = w - 2.  The eight ds fragments are eight loads; element i of a lane's pieces is token
//               slot kk*32 + G*8 + i in every one of them, its maximum is taken over the eight pieces and then across the 16 lanes
//               (dims) of the group; a converted piece is one 8-byte store, and the group's eight scale bytes are contiguous
//               (kv8_scale_byte: slot G*8 + i of half kk is byte G*16 + kk*8 + i).
__global__ __launch_bounds__(256) void kv_pages_quantize_kernel(const uint64_t* src_ptrs, const uint64_t* dst_ptrs, int kvh,
                                                                uint64_t src_layer_stride, uint64_t dst_layer_stride) {
  const int page = blockIdx.x, kvhd = blockIdx.y, layer = blockIdx.z;
  const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6), lane = threadIdx.x & 63, G = lane >> 4, c = lane & 15;
  const uint64_t src = gp<gcu64_t>(src_ptrs)[page] + (uint64_t)layer * src_layer_stride;
  const uint64_t dst = gp<gcu64_t>(dst_ptrs)[page] + (uint64_t)layer * dst_layer_stride;
  const uint64_t sc = dst + (uint64_t)kvh * (2 * KV8_HEAD_BYTES) + (uint64_t)kvhd * KV8_SCALE_BYTES;
  if (wave < 2) {
    const uint64_t kb = src + (uint64_t)kvhd * (KV_PAGE_TOKENS * 256), kd = dst + (uint64_t)kvhd * KV8_HEAD_BYTES;
    u32x4_t f[2][4];
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
      for (int k4 = 0; k4 < 4; ++k4) f[s][k4] = ld_nt16_global(kb + ((wave * 2 + s) * 4 + k4) * 1024 + lane * 16);
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      const int sub = wave * 2 + s;
      uint32_t am = 0;
#pragma unroll
      for (int k4 = 0; k4 < 4; ++k4)
#pragma unroll
        for (int i = 0; i < 8; ++i) am = umax(am, kv8_amax_term(piece_elem(f[s][k4], i)));
      am = umax(am, (uint32_t)__shfl_xor((int)am, 16, 64));
      am = umax(am, (uint32_t)__shfl_xor((int)am, 32, 64));
      const int e = kv8_block_exp(am);
      const float inv = mx_exp2(-e);
#pragma unroll
      for (int p = 0; p < 2; ++p) {
        const u32x2_t lo = piece_codes(f[s][2 * p], [&](int) { return inv; }), hi = piece_codes(f[s][2 * p + 1], [&](int) { return inv; });
        *reinterpret_cast<gst16_t>(kd + (sub * 2 + p) * 1024 + lane * 16) = u32x4_t{lo[0], lo[1], hi[0], hi[1]};
      }
      if (G == 0) reinterpret_cast<gu8_t>(sc)[kv8_scale_byte(sub * 16 + c)] = (uint8_t)(e + 127);
    }
  } else {
    const int kk = wave - 2;
    const uint64_t vb = src + (uint64_t)kvh * (KV_PAGE_TOKENS * 256) + (uint64_t)kvhd * (128 * KV_PAGE_TOKENS * 2);
    const uint64_t vd = dst + (uint64_t)(kvh + kvhd) * KV8_HEAD_BYTES;
    u32x4_t f[8];
#pragma unroll
    for (int ds = 0; ds < 8; ++ds) f[ds] = ld_nt16_global(vb + (ds * 2 + kk) * 1024 + lane * 16);
    float inv[8];
    uint32_t sw[2] = {0u, 0u};
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      uint32_t am = 0;
#pragma unroll
      for (int ds = 0; ds < 8; ++ds) am = umax(am, kv8_amax_term(piece_elem(f[ds], i)));
#pragma unroll
      for (int x = 1; x < 16; x <<= 1) am = umax(am, (uint32_t)__shfl_xor((int)am, x, 64));
      const int e = kv8_block_exp(am);
      inv[i] = mx_exp2(-e);
      sw[i >> 2] |= (uint32_t)(e + 127) << ((i & 3) * 8);
    }
#pragma unroll
    for (int ds = 0; ds < 8; ++ds)
      *reinterpret_cast<gst8_t>(vd + ds * 1024 + lane * 16 + kk * 8) = piece_codes(f[ds], [&](int i) { return inv[i]; });
    if (c == 0) *reinterpret_cast<gst8_t>(sc + KV_PAGE_TOKENS + G * 16 + kk * 8) = u32x2_t{sw[0], sw[1]};
  }
}

// Block (kv head, split, row): attn_decode_batch_block of kernels_batch.hip with the KV8 body.  Splits past the row's own count return at once.
template <bool APPEND>
__device__ __forceinline__ void attn_decode_batch_kv8_block(const AttnDecodeBatchArgs& b, char* smem) {
  const int kvhd = blockIdx.x, split = blockIdx.y, r = blockIdx.z;
  const int32_t* t = b.row_tab + (int64_t)r * GEN_ROW_WORDS;
  const int nsplit = __builtin_amdgcn_readfirstlane(t[GEN_ROW_NSPLIT]);
  if (split >= nsplit) return;
  const int page0 = __builtin_amdgcn_readfirstlane(t[GEN_ROW_PAGE0]);
  const int kv_len = __builtin_amdgcn_readfirstlane(t[GEN_ROW_KVLEN]);
  const unsigned ctr0 = (unsigned)__builtin_amdgcn_readfirstlane(t[GEN_ROW_CTR]);
  AttnDecodeFusedArgs a{};
  a.qkv = (const bf16_t*)b.qkv + (int64_t)r * (b.nh + 2 * b.kvh) * 128;
  a.q_norm_w = b.q_norm_w;
  a.k_norm_w = b.k_norm_w;
  a.rope = b.rope + (int64_t)r * 128;
  a.kv.page_ptrs = b.page_ptrs + page0;
  a.kv.layer_off = b.layer_off;
  a.kv.kvh = b.kvh;
  a.kv.d = 128;
  a.kv_start_v = kv_len - 1;
  a.kv_len_v = kv_len;
  a.part_o = b.part_o + (int64_t)r * b.max_nsplit * b.nh * 128;
  a.part_ml = b.part_ml + (int64_t)r * b.max_nsplit * b.nh * 2;
  a.o = (bf16_t*)b.o + (int64_t)r * b.nh * 128;
  a.head_ctr = b.head_ctr + (int64_t)__builtin_amdgcn_readfirstlane(t[GEN_ROW_CTRROW]) * b.kvh * 32;
  a.ctr_target = ctr0 + (unsigned)b.ctr_step * (unsigned)nsplit;
  a.trace = nullptr;
  a.nh = b.nh;
  a.kvh = b.kvh;
  a.nsplit = nsplit;
  a.eps = b.eps;
  a.scale = b.scale;
  attn_decode_fused_body<APPEND, false, true>(a, smem, kvhd, split, nsplit);
}

__global__ __launch_bounds__(256, 2) void attn_decode_batch_kv8_kernel(AttnDecodeBatchArgs b) {
  __shared__ __attribute__((aligned(16))) char smem[ATTN_DECODE_FUSED_LDS];
  attn_decode_batch_kv8_block<true>(b, smem);
}

__global__ __launch_bounds__(256, 2) void attn_decode_rows_kv8_kernel(AttnDecodeBatchArgs b) {
  __shared__ __attribute__((aligned(16))) char smem[ATTN_DECODE_FUSED_LDS];
  attn_decode_batch_kv8_block<false>(b, smem);
}

// One wave per (kv head, row): kv_append_rows_kernel's k-norm + RoPE (kernels_batch.hip), expression by expression, then the body's
// quantiser on (k roped, v raw) -- a lane holds dims lane and lane + 64 of both -- and the codes and scale bytes into slot kv_len - 1.
__global__ __launch_bounds__(64) void kv_append_rows_kv8_kernel(AttnDecodeBatchArgs b) {
  const int kvhd = blockIdx.x, r = blockIdx.y, lane = (int)threadIdx.x;
  const gci32_t t = gp<gci32_t>(b.row_tab) + (int64_t)r * GEN_ROW_WORDS;
  const int page0 = __builtin_amdgcn_readfirstlane(t[GEN_ROW_PAGE0]);
  const int kv_len = __builtin_amdgcn_readfirstlane(t[GEN_ROW_KVLEN]);
  const gcbf_t qkv = gp<gcbf_t>(b.qkv) + (int64_t)r * (b.nh + 2 * b.kvh) * 128;
  const gcbf_t ksrc = qkv + (int64_t)(b.nh + kvhd) * 128, vsrc = qkv + (int64_t)(b.nh + b.kvh + kvhd) * 128;
  const gcbf_t nw = gp<gcbf_t>(b.k_norm_w);
  const gcf_t rope = gp<gcf_t>(b.rope) + (int64_t)r * 128;
  const bf16_t bx0 = ksrc[lane], bx1 = ksrc[lane + 64];
  const bf16_t bw0 = nw[lane], bw1 = nw[lane + 64];
  const float cs = rope[lane], sn = rope[64 + lane];
  const bf16_t v0 = vsrc[lane], v1 = vsrc[lane + 64];
  const int slot = kv_len - 1, pg = slot / KV_PAGE_TOKENS, tk = slot % KV_PAGE_TOKENS;
  const uint64_t base = gp<gcu64_t>(b.page_ptrs)[page0 + pg] + b.layer_off;
  float x0 = bf2f(bx0), x1 = bf2f(bx1);
  const float ss = wave_sum(fmaf(x0, x0, x1 * x1));
  const float rinv = 1.0f / sqrtf(ss / 128.0f + b.eps);
  x0 = rbf(x0 * rinv * bf2f(bw0));
  x1 = rbf(x1 * rinv * bf2f(bw1));
  const bf16_t y0 = f2bf(rbf(x0 * cs) + rbf(-x1 * sn));
  const bf16_t y1 = f2bf(rbf(x1 * cs) + rbf(x0 * sn));
  const int ek = kv8_block_exp(kv8_wave_max(umax(kv8_amax_term(y0), kv8_amax_term(y1))));
  const int ev = kv8_block_exp(kv8_wave_max(umax(kv8_amax_term(v0), kv8_amax_term(v1))));
  const float ik = mx_exp2(-ek), iv = mx_exp2(-ev);
  const gu8_t kd = reinterpret_cast<gu8_t>(base + (uint64_t)kvhd * KV8_HEAD_BYTES);
  const gu8_t vd = reinterpret_cast<gu8_t>(base + (uint64_t)(b.kvh + kvhd) * KV8_HEAD_BYTES);
  const gu8_t sd = reinterpret_cast<gu8_t>(base + (uint64_t)b.kvh * (2 * KV8_HEAD_BYTES) + (uint64_t)kvhd * KV8_SCALE_BYTES);
  kd[kv8_kpage_byte(tk, lane)] = (uint8_t)kv8_code(y0, ik);
  kd[kv8_kpage_byte(tk, lane + 64)] = (uint8_t)kv8_code(y1, ik);
  vd[kv8_vpage_byte(tk, lane)] = (uint8_t)kv8_code(v0, iv);
  vd[kv8_vpage_byte(tk, lane + 64)] = (uint8_t)kv8_code(v1, iv);
  if (lane == 0) {
    sd[kv8_scale_byte(tk)] = (uint8_t)(ek + 127);
    sd[KV_PAGE_TOKENS + kv8_scale_byte(tk)] = (uint8_t)(ev + 127);
  }
}

}  // namespace

void launch_attn_decode_batch_kv8(const AttnDecodeBatchArgs& b, int rows, int max_nsplit_rows, hipStream_t st, bool append) {
  if (rows <= 0) return;
  const dim3 grid((unsigned)b.kvh, (unsigned)max_nsplit_rows, (unsigned)rows);
  if (append) hipLaunchKernelGGL(attn_decode_batch_kv8_kernel, grid, dim3(256), 0, st, b);
  else hipLaunchKernelGGL(attn_decode_rows_kv8_kernel, grid, dim3(256), 0, st, b);
}

void launch_kv_append_rows_kv8(const AttnDecodeBatchArgs& b, int rows, hipStream_t st) {
  if (rows <= 0) return;
  hipLaunchKernelGGL(kv_append_rows_kv8_kernel, dim3((unsigned)b.kvh, (unsigned)rows), dim3(64), 0, st, b);
}

void launch_kv_pages_quantize(const uint64_t* src_ptrs, const uint64_t* dst_ptrs, int n_pages, int kvh, int n_layers, uint64_t src_layer_stride,
                              uint64_t dst_layer_stride, hipStream_t st) {
  if (n_pages <= 0 || n_layers <= 0) return;
  hipLaunchKernelGGL(kv_pages_quantize_kernel, dim3((unsigned)n_pages, (unsigned)kvh, (unsigned)n_layers), dim3(256), 0, st, src_ptrs, dst_ptrs,
                     kvh, src_layer_stride, dst_layer_stride);
}

}  // namespace aha
