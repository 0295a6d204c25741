// Prefill GEMM from MXFP8 operands on gfx950's block-scaled matrix instruction (kernels.h "MXFP8 prefill GEMM"; model.hip prefill_layers of a
// model quantised with AHA_WQ_PREFILL):
//
//   C[M,N] = epilogue( (Aq . a_scales)[M,K] . (Wq . w_scales)[N,K]^T )       E4M3 bytes + E8M0 block scales in, bf16 out, f32 accumulate
//
//   mxfp8_quantize_rows_kernel   bf16 activation rows -> (Aq, a_scales) in the layout of the weight copies, mxfp8.h's arithmetic: 16 lanes per
//                                128-k chunk of a row, 16-byte loads, the block maximum over a lane quad by DPP, 8-byte stores, the chunk's
//                                scale word assembled by two row rotations.
//   gemm_mxfp8_kernel            256 x 128 tile on four waves (2 x 2, 128 x 64 each, one wave per SIMD), v_mfma_scale_f32_16x16x128_f8f6f4.
//
// Operand roles, as measured on MI355X with one-hot operands (profiles/prefill_fp8.md): lane (row = lane & 15, G = lane >> 4) feeds the
// instruction TWO 16-byte runs of its row's 128-k chunk -- registers 0-3 = k 16G .. 16G + 15, registers 4-7 = k 64 + 16G .. 64 + 16G + 15 -- so
// a lane's 32 bytes lie in two MX blocks (G >> 1 and 2 + (G >> 1)), not in one.  The block scales are applied per 32 consecutive k all the
// same: block b takes its scale from the scale operand of lane group b.  So lane group G supplies byte G of the (row, chunk) scale word;
// the byte selector of the instruction is an immediate, hence a lane shifts its own byte down (word >> 8G) and every instruction selects
// byte 0.  (Feeding a lane 32 consecutive k pairs the right elements but scales half of them with a neighbour block's byte.)  The MFMA is
// issued W-fragment x A-fragment as in the bf16 kernels: a lane ends with 4 consecutive output columns of one row and the epilogue chain
// of gemm256_body.h (epilogue<>, the same SiLU) applies unchanged.
// Staging.  A 128-k step of a byte matrix is a 128-byte row piece -- the LDS image of the bf16 kernels' 64-k step: XOR-swizzled 16-byte slots,
// filled by global_load_lds_dwordx4 with the swizzle on the source address, read back as two ds_read_b128 per fragment (slots G and 4 + G).
// A ring of three stages of [A 256 rows | W 128 rows | scale words] = 49.5 KiB each: tile kt + 2 is requested while tile kt is multiplied, one
// counted vmcnt wait and one raw barrier per k step.  Tiles past the end are requested again from the last one (into a stage nobody reads) so
// the counts stay uniform.
// Scales travel with the tile through the same DMA ring: (256 + 128) words per k step, one global_load_lds_dword per wave and operand, read
// back as one ds_read_b32 per fragment row.  The other choice -- a dword load per fragment row into registers one step ahead -- was written
// first: the compiler cannot count register loads across the loop's back edge next to the LDS-DMA requests and put an s_waitcnt vmcnt(0) in
// front of their first use, which drains the ring every step.  Through LDS the step's one vmcnt(14) covers them and nothing else waits.
// Rows past M / N are clamped to the last row (never fetched out of bounds, never stored).  K is a multiple of 128; no split-K.
#include "common.h"
#include "gemm256_body.h"
#include "kernels.h"
#include "mxfp8.h"

namespace aha {

namespace {

typedef __attribute__((ext_vector_type(8))) int i32x8_t;

constexpr int F8_TM = 256, F8_TN = 128, F8_BK = 128, F8_NST = 3;
constexpr int F8_A_BYTES = F8_TM * F8_BK, F8_W_BYTES = F8_TN * F8_BK, F8_STAGE = F8_A_BYTES + F8_W_BYTES + (F8_TM + F8_TN) * 4;
constexpr int F8_LPT = 14;   // LDS-DMA requests per wave and k step: 8 pieces (8 rows x 128 B) of A, 4 of W, 2 x 64 scale words

// ---- activation row quantiser ------------------------------------------------------------------------------------------------
// A non-finite activation or one at or above MX_BF16_ABS_LIMIT does not fail anything: +-Inf and the too-large values saturate to
// +-448 * 2^120 (code 0x7e under the largest block exponent), NaN becomes the E4M3 NaN code 0x7f and takes no part in the block maximum.
__global__ __launch_bounds__(256) void mxfp8_quantize_rows_kernel(const bf16_t* __restrict__ A, int64_t lda, int M, int chunks,
                                                                  uint8_t* __restrict__ q, uint32_t* __restrict__ scales) {
  const int64_t total = (int64_t)M * chunks, grp = ((int64_t)blockIdx.x * 256 + threadIdx.x) >> 4;
  const bool live = grp < total;
  const int64_t g = live ? grp : total - 1;   // the last wave's idle lanes redo the last chunk (the cross-lane steps want every lane) and store nothing
  const int64_t row = g / chunks;
  const int ch = (int)(g - row * chunks), l16 = threadIdx.x & 15;
  const u32x4_t v = ld16(A + row * lda + ch * 128 + l16 * 8);
  uint32_t b[8], amax = 0;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    b[i] = (v[i >> 1] >> ((i & 1) * 16)) & 0xffffu;
    const uint32_t a = b[i] & 0x7fffu;
    const uint32_t am = a > 0x7f80u ? 0u : a >= MX_BF16_ABS_LIMIT ? MX_BF16_ABS_LIMIT - 1 : a;
    amax = amax > am ? amax : am;
  }
  // block maximum: the quad's four lanes hold the block's 32 elements
  {
    const uint32_t o = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)amax, 0xB1 /* quad_perm:[1,0,3,2] */, 0xf, 0xf, false);
    amax = amax > o ? amax : o;
  }
  {
    const uint32_t o = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)amax, 0x4E /* quad_perm:[2,3,0,1] */, 0xf, 0xf, false);
    amax = amax > o ? amax : o;
  }
  const int e = mx_block_exp(amax);
  const float inv = mx_exp2(-e);
  uint32_t code[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const uint32_t a = b[i] & 0x7fffu, sign = (b[i] >> 8) & 0x80u;
    // w * 2^-e is exact; a product below f32's normal range is below half of E4M3's smallest subnormal with or without flushing
    const uint32_t fin = mx_e4m3_rne(bf2f((bf16_t)(a < MX_BF16_ABS_LIMIT ? b[i] : 0)) * inv);
    code[i] = a > 0x7f80u ? (sign | 0x7fu) : a >= MX_BF16_ABS_LIMIT ? (sign | 0x7eu) : fin;
  }
  uint2 out;
  out.x = code[0] | (code[1] << 8) | (code[2] << 16) | (code[3] << 24);
  out.y = code[4] | (code[5] << 8) | (code[6] << 16) | (code[7] << 24);
  // the chunk's scale word: quad g holds byte g; two rotations inside the 16-lane row bring the other three
  uint32_t w = (uint32_t)(e + 127) << (8 * (l16 >> 2));
  w |= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)w, 0x128 /* row_ror:8 */, 0xf, 0xf, false);
  w |= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)w, 0x124 /* row_ror:4 */, 0xf, 0xf, false);
  if (live) {
    *reinterpret_cast<uint2*>(q + (row * chunks + ch) * 128 + l16 * 8) = out;
    if (l16 == 0) scales[row * chunks + ch] = w;
  }
}

// ---- the GEMM ----------------------------------------------------------------------------------------------------------------
// a.A / a.W: the E4M3 bytes (row pitch K bytes), asc / wsc: their scale words (row pitch K / 128 words); the rest of GemmArgs as for the
// bf16 kernels (C, ldc, residual, M, N, K, tile_group).
template <int ACT, bool HAS_RES>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 1))) void gemm_mxfp8_kernel(GemmArgs a, const uint32_t* __restrict__ asc,
                                                                                                    const uint32_t* __restrict__ wsc) {
  char* const smem = gemm_smem;   // F8_NST x [A tile | W tile]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, G = lane >> 4, c = lane & 15;
  const int wm = wave >> 1, wn = wave & 1;
  int m0, n0;
  tile_of_block<F8_TM, F8_TN>(a, m0, n0);
  const int nk = a.K / F8_BK;
  const uint8_t* A = (const uint8_t*)a.A;
  const uint8_t* W = (const uint8_t*)a.W;

  // staging: wave w issues the 8-row pieces j * 4 + w (A: j < 8, W: j < 4).  Lane i of a piece lands on image row piece * 8 + (i >> 3),
  // physical slot i & 7, and therefore fetches logical slot (i & 7) ^ ((row >> 1) & 7).
  const uint8_t* ga[8];
  const uint8_t* gw[4];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int row = (j * 4 + wave) * 8 + (lane >> 3);
    const int sl = (lane & 7) ^ ((row >> 1) & 7);
    ga[j] = A + (int64_t)min(m0 + row, a.M - 1) * a.K + sl * 16;
    if (j < 4) gw[j] = W + (int64_t)min(n0 + row, a.N - 1) * a.K + sl * 16;
  }
  const uint32_t* gsa = asc + (int64_t)min(m0 + wave * 64 + lane, a.M - 1) * nk;
  const uint32_t* gsw = wsc + (int64_t)min(n0 + (wave & 1) * 64 + lane, a.N - 1) * nk;
  auto stage = [&](int kt, int st_) __attribute__((always_inline)) {
    const int kc = min(kt, nk - 1), ko = kc * F8_BK;   // past the end: the last tile again, into a stage nobody reads any more
    char* sa = smem + st_ * F8_STAGE;
    char* sw = sa + F8_A_BYTES;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      __builtin_amdgcn_global_load_lds((glb_ptr_t)(ga[j] + ko), (lds_ptr_t)(sa + (j * 4 + wave) * 1024), 16, 0, 0);
      if (j < 4) __builtin_amdgcn_global_load_lds((glb_ptr_t)(gw[j] + ko), (lds_ptr_t)(sw + (j * 4 + wave) * 1024), 16, 0, 0);
    }
    // the step's scale words: one dword per lane and row -- A rows 64 wave .., W rows 64 (wave & 1) .. (waves 2 and 3 write what waves 0 and
    // 1 write: every wave issues the same number of pieces)
    __builtin_amdgcn_global_load_lds((glb_ptr_t)(gsa + kc), (lds_ptr_t)(sw + F8_W_BYTES + wave * 256), 4, 0, 0);
    __builtin_amdgcn_global_load_lds((glb_ptr_t)(gsw + kc), (lds_ptr_t)(sw + F8_W_BYTES + F8_TM * 4 + (wave & 1) * 256), 4, 0, 0);
  };
  f32x4_t acc[4][8];   // [ni][mi]
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[i][j] = f32x4_t{0.f, 0.f, 0.f, 0.f};

#define AHA_F8_BAR()                             \
  do {                                           \
    __builtin_amdgcn_sched_barrier(0);           \
    __builtin_amdgcn_s_barrier();                \
    __builtin_amdgcn_sched_barrier(0);           \
  } while (0)
  auto read_frag = [&](const char* tile, int row) __attribute__((always_inline)) {
    const u32x4_t lo = *reinterpret_cast<const u32x4_t*>(tile + swz(row, G));
    const u32x4_t hi = *reinterpret_cast<const u32x4_t*>(tile + swz(row, 4 + G));
    return i32x8_t{(int)lo[0], (int)lo[1], (int)lo[2], (int)lo[3], (int)hi[0], (int)hi[1], (int)hi[2], (int)hi[3]};
  };
  stage(0, 0);
  stage(1, 1);
  int st = 0, st_new = 2;
  for (int kt = 0; kt < nk; ++kt) {
    // everything but the newest tile's pieces has landed: this wave's pieces of tile kt.  vmcnt is a 6-bit field, [3:0] and [15:14]; the
    // other counters stay untouched (0x0F70)
    __builtin_amdgcn_sched_barrier(0);
    __builtin_amdgcn_s_waitcnt(0x0F70 | (F8_LPT & 15) | ((F8_LPT >> 4) << 14));
    AHA_F8_BAR();   // tile kt is whole, and nobody reads tile kt - 1 any more: its stage takes tile kt + 2
    stage(kt + 2, st_new);
    __builtin_amdgcn_sched_barrier(0);
    const char* sa = smem + st * F8_STAGE;
    const char* sw = sa + F8_A_BYTES;
    const char* ssa = sw + F8_W_BYTES;
    const char* ssw = ssa + F8_TM * 4;
    // the W fragments and scale bytes stay for the step; the A fragments are read one ahead of the four MFMAs that use them
    i32x8_t wf[4], af[2];
    int sws[4], sas[8];
#pragma unroll
    for (int i = 0; i < 4; ++i) wf[i] = read_frag(sw, wn * 64 + i * 16 + c);
    af[0] = read_frag(sa, wm * 128 + c);
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      sas[i] = (int)(*reinterpret_cast<const uint32_t*>(ssa + (wm * 128 + i * 16 + c) * 4) >> (8 * G));
      if (i < 4) sws[i] = (int)(*reinterpret_cast<const uint32_t*>(ssw + (wn * 64 + i * 16 + c) * 4) >> (8 * G));
    }
#pragma unroll
    for (int mi = 0; mi < 8; ++mi) {
      if (mi < 7) af[(mi + 1) & 1] = read_frag(sa, wm * 128 + (mi + 1) * 16 + c);
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int ni = 0; ni < 4; ++ni)
        acc[ni][mi] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(wf[ni], af[mi & 1], acc[ni][mi], 0, 0, 0, sws[ni], 0, sas[mi]);
      __builtin_amdgcn_sched_barrier(0);
    }
    st_new = st;
    st = (st + 1 == F8_NST) ? 0 : st + 1;
  }
  __builtin_amdgcn_s_waitcnt(0x0F70);   // the requests past the end still write their pieces: nothing in flight when the block retires
  AHA_F8_BAR();
#undef AHA_F8_BAR
  epilogue<ACT, false, HAS_RES, 8, 4>(a, acc, m0 + wm * 128, n0 + wn * 64, G, c);
}

}  // namespace

void launch_mxfp8_quantize_rows(const void* A, int64_t lda, int M, int K, void* q_out, uint32_t* scales_out, hipStream_t st) {
  const int chunks = K / F8_BK;
  const int64_t threads = (int64_t)M * chunks * 16;
  mxfp8_quantize_rows_kernel<<<dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, st>>>((const bf16_t*)A, lda, M, chunks, (uint8_t*)q_out,
                                                                                          scales_out);
}

bool gemm_mxfp8_shape_ok(int M, int N, int K, int act) {
  return M >= 1 && N >= 16 && N % 16 == 0 && K >= F8_BK && K % F8_BK == 0 && (act == ACT_NONE || (act == ACT_SILU_MUL_PAIRS && N % 32 == 0));
}

void debug_plan_gemm_mxfp8(int M, int N, int K, int act, int* out4) {
  (void)K;
  (void)act;
  out4[0] = F8_TM;
  out4[1] = F8_TN;
  out4[2] = ((M + F8_TM - 1) / F8_TM) * ((N + F8_TN - 1) / F8_TN);
  out4[3] = F8_NST;
}

void launch_gemm_mxfp8(const GemmArgs& a, const uint32_t* a_scales, const uint32_t* w_scales, hipStream_t st) {
  GemmArgs g = a;
  g.lda = g.ldw = g.K;
  g.bias = nullptr;
  g.groups = 1;
  int plan[4];
  debug_plan_gemm_mxfp8(g.M, g.N, g.K, g.act, plan);
  void (*kern)(GemmArgs, const uint32_t*, const uint32_t*) =
      g.act == ACT_SILU_MUL_PAIRS ? gemm_mxfp8_kernel<ACT_SILU_MUL_PAIRS, false>
                                  : g.residual ? gemm_mxfp8_kernel<ACT_NONE, true> : gemm_mxfp8_kernel<ACT_NONE, false>;
  constexpr int LDS = F8_NST * F8_STAGE;   // 144 KiB: above the 64 KiB a kernel gets without asking (the attribute is per device; setting it again is free)
  if (hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, LDS) != hipSuccess) return;   // (the caller reads hipGetLastError)
  kern<<<dim3((unsigned)plan[2]), dim3(256), LDS, st>>>(g, a_scales, w_scales);
  if (g.norm_w && g.norm_out) launch_rmsnorm_rows(g.C, g.norm_w, g.norm_out, g.M, g.N, g.ldc, g.N, g.norm_eps, st);
}

}  // namespace aha
