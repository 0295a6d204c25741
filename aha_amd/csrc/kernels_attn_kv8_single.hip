// Single-sequence decode attention over an E4M3 KV cache ("KV8"; format: kernels.h, page layout: common.h "KV8 page layout", arithmetic: kv8.h).
//
//   attn_decode_fused_kv8_kernel        attn_decode_fused_kernel (kernels_attn.hip) over the KV8 twins of a request whose twins are an
//                                       arithmetic progression: attn_decode_fused_body<true, LINEAR = true, KV8 = true>
//   attn_decode_fused_kv8_table_kernel  the same through the twin page table (a second slab, shuffled pages)
//
// Both take the flat argument form of the bf16 kernels: the 14 leading dwords -- qkv row, the two page arguments, rope table, norm weights,
// cache length, packed head / split counts -- arrive in user SGPRs at wave launch (kernarg preload, build.py), the rest travels in the
// trailing struct and is first used behind the first requests.  In the linear form the two page arguments are (address of twin page 0 of
// the layer, byte step between twins): the unit's first K request is scalar arithmetic on preloaded registers, no load and no wait in
// front of it.  What differs from the bf16 kernel is the body's KV8 side: 8 + 8 fragment loads and two 16-byte scale pieces per page
// instead of 16 + 16 loads, 4 v_cvt_scalef32_pk_bf16_fp8 per MFMA operand, the block scales on the scores and the probabilities, and the
// new token quantised behind the prologue's barrier (codes and scale bytes to the twin, the dequantised values back to LDS).
// This unit is compiled without the packed-f32 instructions, like kernels_attn_kv8.hip, and with the kernarg preload of kernels_attn.hip.
// There are no traced twins: AHA_ATTN_TRACE on such a model says so once (model.hip).
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>

#include "attn_decode_body.h"
#include "common.h"
#include "kernels.h"
#include "kv8.h"

namespace aha {

namespace {

// kernels_attn.hip's AttnDecodeFusedTail, member for member (the trace pointer stays in the layout and is never read here)
struct AttnDecodeFusedTail {
  float* part_o;
  float* part_ml;
  void* o;
  unsigned* head_ctr;
  unsigned long long* trace;
  unsigned ctr_target;
  int kv_start_v, kv_kvh, kv_d;
  float eps, scale;
};

template <bool LINEAR>
__device__ __forceinline__ void attn_decode_fused_kv8_flat(const void* qkv, uint64_t pages, uint64_t pages2, const float* rope,
                                                           const void* q_norm_w, const void* k_norm_w, int kv_len_v, int dims,
                                                           const AttnDecodeFusedTail& t, char* smem) {
  AttnDecodeFusedArgs a;
  a.qkv = qkv; a.q_norm_w = q_norm_w; a.k_norm_w = k_norm_w; a.rope = rope;
  a.kv.page_ptrs = LINEAR ? nullptr : reinterpret_cast<const uint64_t*>(pages); a.kv.layer_off = LINEAR ? 0 : pages2;
  a.lin_page0 = LINEAR ? pages : 0; a.lin_step = LINEAR ? (int64_t)pages2 : 0;
  a.kv.kvh = t.kv_kvh; a.kv.d = t.kv_d;
  a.kv_start_v = t.kv_start_v; a.kv_len_v = kv_len_v;
  a.part_o = t.part_o; a.part_ml = t.part_ml; a.o = t.o; a.head_ctr = t.head_ctr; a.ctr_target = t.ctr_target;
  a.trace = nullptr;
  a.nh = dims & 1023; a.kvh = (dims >> 10) & 1023; a.nsplit = dims >> 20; a.eps = t.eps; a.scale = t.scale;
  attn_decode_fused_body<true, LINEAR, true>(a, smem, (int)blockIdx.x, (int)blockIdx.y, a.nsplit);
}

__global__ __launch_bounds__(256, 2) void attn_decode_fused_kv8_kernel(const void* qkv, uint64_t lin_page0, uint64_t lin_step, const float* rope,
                                                                       const void* q_norm_w, const void* k_norm_w, int kv_len_v, int dims,
                                                                       AttnDecodeFusedTail t) {
  __shared__ __attribute__((aligned(16))) char smem[ATTN_DECODE_FUSED_LDS];
  attn_decode_fused_kv8_flat<true>(qkv, lin_page0, lin_step, rope, q_norm_w, k_norm_w, kv_len_v, dims, t, smem);
}

__global__ __launch_bounds__(256, 2) void attn_decode_fused_kv8_table_kernel(const void* qkv, uint64_t page_ptrs, uint64_t layer_off,
                                                                             const float* rope, const void* q_norm_w, const void* k_norm_w,
                                                                             int kv_len_v, int dims, AttnDecodeFusedTail t) {
  __shared__ __attribute__((aligned(16))) char smem[ATTN_DECODE_FUSED_LDS];
  attn_decode_fused_kv8_flat<false>(qkv, page_ptrs, layer_off, rope, q_norm_w, k_norm_w, kv_len_v, dims, t, smem);
}

}  // namespace

// a.kv.page_ptrs / a.kv.layer_off or a.lin_page0 / a.lin_step address KV8 pages; a.trace is ignored
void launch_attn_decode_fused_kv8(const AttnDecodeFusedArgs& a, hipStream_t st) {
  const AttnDecodeFusedTail t{a.part_o, a.part_ml, a.o, a.head_ctr, nullptr, a.ctr_target, a.kv_start_v, a.kv.kvh, a.kv.d, a.eps, a.scale};
  // the bf16 launch's limits: 10 bits each for the head counts, g * nsplit <= 1024 for the LDS tables of the split merge
  if (a.nh > 1023 || a.kvh > 1023 || a.nsplit > 1024 || a.nsplit < 1 || a.kv.d != 128) {
    fprintf(stderr, "launch_attn_decode_fused_kv8: head / split counts out of range, or head_dim is not 128\n");
    abort();
  }
  const int dims = a.nh | (a.kvh << 10) | (a.nsplit << 20);
  const dim3 grid((unsigned)a.kvh, (unsigned)a.nsplit);
  if (a.lin_step != 0)
    hipLaunchKernelGGL(attn_decode_fused_kv8_kernel, grid, dim3(256), 0, st, a.qkv, a.lin_page0, (uint64_t)a.lin_step, a.rope, a.q_norm_w,
                       a.k_norm_w, a.kv_len_v, dims, t);
  else
    hipLaunchKernelGGL(attn_decode_fused_kv8_table_kernel, grid, dim3(256), 0, st, a.qkv, (uint64_t)(uintptr_t)a.kv.page_ptrs, a.kv.layer_off,
                       a.rope, a.q_norm_w, a.k_norm_w, a.kv_len_v, dims, t);
}

}  // namespace aha
