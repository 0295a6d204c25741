// Multi-sequence decode (model_generate_batch, model.hip): the kernels one step of R independent sequences runs on top of the
// row-wise norms.
//
//   gemv_rows_kernel         out[R, N] = x[R, K] . W[N, K]^T for R <= 32: every weight element is read from HBM ONCE per launch
//                            (non-temporal, straight to VGPRs) and multiplied with all R rows by v_mfma_f32_16x16x32_bf16 -- the rows
//                            are the A operand, padded to 16 (one or two row tiles), 32 weight rows the B operand of two MFMAs.
//                            gemv_rows_body (gemv_rows_body.h) with the GemvRowsBf16 weight form; the MXFP8 / MXFP4 kernels are the
//                            same body with theirs.
//   gemv_rows_merge_kernel   the fixed-order sum of the K-split partials + the epilogue (store / residual / SiLU.mul pairs / logits).
//   argmax_rows_kernel       per-row pick of the logits epilogue's (max, index) partials -> the device token vector.
//   gen_embed_kernel         the R token embeddings (tokens read from the device vector the previous step's pick wrote) + every row's
//                            rope cos / sin table.
//   attn_decode_batch_kernel q/k-norm + RoPE + KV append + split-KV attention + split merge of ALL rows in one launch: one block per
//                            (kv head, split, row), each running attn_decode_fused_body on its row's qkv, rope row and pages.
//   kv_append_rows_kernel    draft-and-verify steps (aha_hip_generate_batch_spec): the k-norm + RoPE + KV append of every row in a launch of
//                            its own, so that row i + 1 of a sequence finds row i's K/V in the pages; the attention launch that follows is
//                            attn_decode_rows_kernel, the batch attention with the body's append compiled out.
//   spec_accept_rows_kernel  per sequence, the longest draft prefix the step's argmax vector confirms -> its emitted tokens.
//   spec_accept_split_kernel the same for the engine's row layout (aha_hip_engine_submit_spec): a request's own row among the step's mandatory
//                            rows, its draft rows behind them.
//
// Row isolation (tests/test_generate_batch_gpu.py): every output element of gemv_rows is summed in an order that depends only on
// (N, K) -- within a wave the MFMA chain over its chunks, across the 4 waves of a block ((w0 + w1) + w2) + w3 through LDS, across the
// K splits slab 0, 1, ... in the merge kernel -- and an MFMA output row depends only on its own A row.  So a row's bits do not depend on
// R or on the other rows.  The attention of a row is attn_decode_fused_body with that row's arguments and the single-sequence split rule,
// so it is bit-identical to attn_decode_fused_kernel on the same inputs.
#include <hip/hip_runtime.h>

#include "attn_decode_body.h"
#include "common.h"
#include "gemv_body.h"   // silu_f: the matvec's activation, for the same bits
#include "gemv_rows_body.h"
#include "kernels.h"

namespace aha {

namespace {

typedef const __attribute__((address_space(1))) bf16_t* gcbf_t;
typedef __attribute__((address_space(1))) bf16_t* gbf_t;
typedef const __attribute__((address_space(1))) float* gcf_t;

template <int CW, int NRT>
__global__ __launch_bounds__(256, 2) void gemv_rows_kernel(GemvRowsArgs a) {
  __shared__ __attribute__((aligned(16))) float red[4 * 2 * NRT * 256];
  gemv_rows_body<GemvRowsBf16, CW, NRT>(a, a.W, nullptr, red);
}

// Sum of the K splits in slab order + the epilogue.  Block (bx, row): 256 output columns of one row.  The Linear output is rounded to
// bf16 first, as candle_nn::Linear's output tensor is (gemv_body.h: lin = rbf(acc)).
template <int EPI>
__global__ __launch_bounds__(256) void gemv_rows_merge_kernel(GemvRowsArgs a, int nks) {
  const int row = blockIdx.y, tid = threadIdx.x;
  const int nout = EPI == GEMV_SILU_MUL ? a.N / 2 : a.N;
  const int j = blockIdx.x * 256 + tid;
  const gcf_t ws = gp<gcf_t>(a.ws) + (int64_t)row * a.ldws;
  const int64_t slab = (int64_t)a.R * a.ldws;
  float best = -INFINITY;
  uint32_t best_i = 0xffffffffu;
  if (j < nout) {
    if (EPI == GEMV_SILU_MUL) {   // output column j: gate row (j/16)*32 + j%16, up row 16 further (ACT_SILU_MUL_PAIRS block layout)
      const int ng = (j >> 4) * 32 + (j & 15), nu = ng + 16;
      float g = ws[ng], u = ws[nu];
      for (int s = 1; s < nks; ++s) g += ws[s * slab + ng], u += ws[s * slab + nu];
      const float ga = rbf(silu_f(rbf(g)));   // gate_proj -> act_fn   (modules.rs:82)
      gp<gbf_t>(a.y)[(int64_t)row * a.ldy + j] = f2bf(ga * rbf(u));   // * up_proj (modules.rs:83-84)
    } else {
      float s0 = ws[j];
      for (int s = 1; s < nks; ++s) s0 += ws[s * slab + j];
      const float lin = rbf(s0);
      if (EPI == GEMV_STORE) {
        gp<gbf_t>(a.y)[(int64_t)row * a.ldy + j] = f2bf(lin);
      } else if (EPI == GEMV_RESIDUAL) {
        const float r = bf2f(gp<gcbf_t>(a.residual)[(int64_t)row * a.ldy + j]);
        gp<gbf_t>(a.y)[(int64_t)row * a.ldy + j] = f2bf(r + lin);
      } else {   // GEMV_LOGITS: the bf16 logits read back as f32 (generate.rs:75)
        gp<gf_t>(a.y_f32)[(int64_t)row * a.ldf + j] = lin;
        best = lin;
        best_i = (uint32_t)j;
      }
    }
  }
  if (EPI == GEMV_LOGITS) {   // (max, first index) of the block's 256 columns
    __shared__ float sv[4];
    __shared__ uint32_t si[4];
    for (int off = 32; off > 0; off >>= 1) {
      const float ov = __shfl_xor(best, off);
      const uint32_t oi = __shfl_xor(best_i, off);
      if (ov > best || (ov == best && oi < best_i)) best = ov, best_i = oi;
    }
    if ((tid & 63) == 0) sv[tid >> 6] = best, si[tid >> 6] = best_i;
    __syncthreads();
    if (tid == 0) {
      for (int w = 1; w < 4; ++w)
        if (sv[w] > best || (sv[w] == best && si[w] < best_i)) best = sv[w], best_i = si[w];
      a.blk_max[(int64_t)row * gridDim.x + blockIdx.x] = best;
      a.blk_idx[(int64_t)row * gridDim.x + blockIdx.x] = best_i;
    }
  }
}

// one block per row: the first maximal index over the row's tiles (argmax_partials' rule)
__global__ __launch_bounds__(256) void argmax_rows_kernel(const float* __restrict__ blk_max, const uint32_t* __restrict__ blk_idx, int ntiles,
                                                          uint32_t* __restrict__ out) {
  const int row = blockIdx.x, tid = threadIdx.x;
  float best = -INFINITY;
  uint32_t best_i = 0xffffffffu;
  for (int t = tid; t < ntiles; t += 256) {
    const float v = blk_max[(int64_t)row * ntiles + t];
    const uint32_t i = blk_idx[(int64_t)row * ntiles + t];
    if (v > best || (v == best && i < best_i)) best = v, best_i = i;
  }
  for (int off = 32; off > 0; off >>= 1) {
    const float ov = __shfl_xor(best, off);
    const uint32_t oi = __shfl_xor(best_i, off);
    if (ov > best || (ov == best && oi < best_i)) best = ov, best_i = oi;
  }
  __shared__ float sv[4];
  __shared__ uint32_t si[4];
  if ((tid & 63) == 0) sv[tid >> 6] = best, si[tid >> 6] = best_i;
  __syncthreads();
  if (tid == 0) {
    for (int w = 1; w < 4; ++w)
      if (sv[w] > best || (sv[w] == best && si[w] < best_i)) best = sv[w], best_i = si[w];
    out[row] = best_i == 0xffffffffu ? 0u : best_i;   // all-NaN logits: a valid id, never an index past the embedding table
  }
}

// Block r: x[r] = embedding of tok_in[row_tab[r].src] (the previous step's pick), and row r's rope table from its position -- the same
// cos / sin rounding as embed_state_kernel (model.hip).
__global__ __launch_bounds__(256) void gen_embed_kernel(const bf16_t* __restrict__ table, const uint32_t* __restrict__ tok_in,
                                                        const int32_t* __restrict__ row_tab, bf16_t* __restrict__ x, int H,
                                                        const float* __restrict__ inv_freq, const int32_t* __restrict__ axis_map,
                                                        float* __restrict__ rope) {
  const int r = blockIdx.x;
  const int32_t* t = row_tab + (int64_t)r * GEN_ROW_WORDS;
  const uint32_t tok = tok_in[t[GEN_ROW_SRC]];
  const u32x4_t* src = reinterpret_cast<const u32x4_t*>(table + (size_t)tok * H);
  u32x4_t* dst = reinterpret_cast<u32x4_t*>(x + (size_t)r * H);
  for (int i = threadIdx.x; i < H / 8; i += 256) dst[i] = src[i];
  if (threadIdx.x < 64) {
    const int i = threadIdx.x;
    const float ang = (float)t[GEN_ROW_POS] * inv_freq[i];   // a decode step's three M-RoPE positions are equal (offset + rope_delta)
    (void)axis_map;
    rope[r * 128 + i] = rbf(cosf(ang));
    rope[r * 128 + 64 + i] = rbf(sinf(ang));
  }
}

// Block (kv head, split, row).  Splits past the row's own count return at once.
template <bool APPEND>
__device__ __forceinline__ void attn_decode_batch_block(const AttnDecodeBatchArgs& b, char* smem) {
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
  attn_decode_fused_body<APPEND>(a, smem, kvhd, split, nsplit);
}

// (spelled out rather than attn_decode_batch_block<true>: the instruction stream of this kernel is the one its measurements were taken on)
__global__ __launch_bounds__(256, 2) void attn_decode_batch_kernel(AttnDecodeBatchArgs b) {
  __shared__ __attribute__((aligned(16))) char smem[ATTN_DECODE_FUSED_LDS];
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
  attn_decode_fused_body(a, smem, kvhd, split, nsplit);
}

// The same without the append: every row's K/V was written by kv_append_rows_kernel in the launch before, so rows of one sequence at
// consecutive positions see each other's tokens in the pages (tokens < kv_len - 1), and their own from LDS, as a row decoding alone does.
__global__ __launch_bounds__(256, 2) void attn_decode_rows_kernel(AttnDecodeBatchArgs b) {
  __shared__ __attribute__((aligned(16))) char smem[ATTN_DECODE_FUSED_LDS];
  attn_decode_batch_block<false>(b, smem);
}

// One wave per (kv head, row): k-norm + RoPE of the row's k head, (k roped, v raw) -> slot kv_len - 1 of the row's sequence.  The
// arithmetic and its rounding points are attn_decode_fused_body's norm_rope lambda and append (attn_decode_body.h), expression by
// expression: the page bits are those the fused kernel's own append writes (tests/test_generate_spec_gpu.py compares whole generations).
__global__ __launch_bounds__(64) void kv_append_rows_kernel(AttnDecodeBatchArgs b) {
  typedef const __attribute__((address_space(1))) int32_t* gci32_t;
  typedef const __attribute__((address_space(1))) uint64_t* gcu64_t;
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
  const gbf_t kd = reinterpret_cast<gbf_t>(base) + (int64_t)kvhd * KV_PAGE_TOKENS * 128;
  const gbf_t vd = reinterpret_cast<gbf_t>(base) + (int64_t)b.kvh * KV_PAGE_TOKENS * 128 + (int64_t)kvhd * 128 * KV_PAGE_TOKENS;
  kd[kpage_elem(tk, lane, 4)] = y0;
  kd[kpage_elem(tk, lane + 64, 4)] = y1;
  vd[vpage_elem(tk, lane)] = v0;
  vd[vpage_elem(tk, lane + 64)] = v1;
}

// Thread s: sequence s of the step, rows row0 .. row0 + k (its last token, then its k draft tokens; a row's input token is word
// GEN_ROW_TOK of its table entry).  a = the longest prefix with argmax(row0 + i) == draft i + 1; the emitted tokens are
// argmax(row0 .. row0 + a): the a confirmed drafts and the token the last confirmed row chose.
__global__ __launch_bounds__(64) void spec_accept_rows_kernel(const uint32_t* argmax, const int32_t* row_tab, const int32_t* seq_tab, int n_seqs,
                                                              uint32_t* out) {
  typedef const __attribute__((address_space(1))) int32_t* gci32_t;
  typedef const __attribute__((address_space(1))) uint32_t* gcu32_t;
  typedef __attribute__((address_space(1))) uint32_t* gu32_t;
  const int s = blockIdx.x * 64 + (int)threadIdx.x;
  if (s >= n_seqs) return;
  const gci32_t st = gp<gci32_t>(seq_tab) + (int64_t)s * SPEC_SEQ_WORDS;
  const gci32_t rt = gp<gci32_t>(row_tab);
  const gcu32_t am = gp<gcu32_t>(argmax);
  const gu32_t o = gp<gu32_t>(out) + (int64_t)s * SPEC_OUT_WORDS;
  const int row0 = st[SPEC_SEQ_ROW0], k = min(st[SPEC_SEQ_NDRAFT], SPEC_MAX_DRAFT);
  int a = 0;
  uint32_t tok = am[row0];
  o[SPEC_OUT_TOKENS] = tok;
  while (a < k && tok == (uint32_t)rt[(int64_t)(row0 + a + 1) * GEN_ROW_WORDS + GEN_ROW_TOK]) {
    ++a;
    tok = am[row0 + a];
    o[SPEC_OUT_TOKENS + a] = tok;
  }
  o[SPEC_OUT_COUNT] = (uint32_t)(a + 1);
  o[SPEC_OUT_LAST_ROW] = (uint32_t)(row0 + a);
}

// The engine's layout (model.hip engine_step): a request's own row sits among the step's mandatory rows, its k draft rows are rows
// d0 .. d0 + k - 1 behind them.  Thread s: position 0 is the own row, position i >= 1 is row d0 + i - 1, whose input token (GEN_ROW_TOK) is
// draft i.  The same rule and the same record as spec_accept_rows_kernel: a = the longest prefix with argmax(position i) == draft i + 1,
// the emitted tokens are argmax(position 0 .. a), the last row is position a's.
__global__ __launch_bounds__(64) void spec_accept_split_kernel(const uint32_t* argmax, const int32_t* row_tab, const int32_t* seq_tab, int n_seqs,
                                                               uint32_t* out) {
  typedef const __attribute__((address_space(1))) int32_t* gci32_t;
  typedef const __attribute__((address_space(1))) uint32_t* gcu32_t;
  typedef __attribute__((address_space(1))) uint32_t* gu32_t;
  const int s = blockIdx.x * 64 + (int)threadIdx.x;
  if (s >= n_seqs) return;
  const gci32_t st = gp<gci32_t>(seq_tab) + (int64_t)s * ENG_SEQ_WORDS;
  const gci32_t rt = gp<gci32_t>(row_tab);
  const gcu32_t am = gp<gcu32_t>(argmax);
  const gu32_t o = gp<gu32_t>(out) + (int64_t)s * SPEC_OUT_WORDS;
  const int own = st[ENG_SEQ_ROW], d0 = st[ENG_SEQ_DRAFT0], k = min(st[ENG_SEQ_NDRAFT], SPEC_MAX_DRAFT);
  int a = 0, row = own;
  uint32_t tok = am[own];
  o[SPEC_OUT_TOKENS] = tok;
  while (a < k && tok == (uint32_t)rt[(int64_t)(d0 + a) * GEN_ROW_WORDS + GEN_ROW_TOK]) {
    row = d0 + a;
    ++a;
    tok = am[row];
    o[SPEC_OUT_TOKENS + a] = tok;
  }
  o[SPEC_OUT_COUNT] = (uint32_t)(a + 1);
  o[SPEC_OUT_LAST_ROW] = (uint32_t)row;
}

}  // namespace

// K-split plan of gemv_rows: a function of (N, K) only (row isolation).  Chunks per wave cw in {1, 2}; splits nks = ceil(chunks / 4cw);
// cw drops to 1 when the grid would leave CUs idle.
void gemv_rows_plan(int N, int K, int* cw, int* nks) {
  const int chunks = (K + GR_CHUNK - 1) / GR_CHUNK, nb = (N + GR_NB - 1) / GR_NB;
  int c = chunks > 4 ? 2 : 1;
  int s = (chunks + 4 * c - 1) / (4 * c);
  if (c == 2 && (int64_t)nb * s < 256) {
    c = 1;
    s = (chunks + 3) / 4;
  }
  *cw = c;
  *nks = s;
}

int gemv_rows_num_tiles(int N) { return (N + 255) / 256; }

size_t gemv_rows_ws_floats(int R, int N, int K) {
  int cw, nks;
  gemv_rows_plan(N, K, &cw, &nks);
  return (size_t)nks * R * N;
}

void launch_gemv_rows(const GemvRowsArgs& a, GemvEpi epi, hipStream_t st) {
  static constexpr void (*kern[2][2])(GemvRowsArgs) = {{gemv_rows_kernel<1, 1>, gemv_rows_kernel<1, 2>},
                                                       {gemv_rows_kernel<2, 1>, gemv_rows_kernel<2, 2>}};
  launch_gemv_rows_form(kern, a, epi, st);
}

// the second launch of a gemv_rows call: a.ws holds the nks slabs (a.ldws set)
void launch_gemv_rows_merge(const GemvRowsArgs& a, GemvEpi epi, int nks, hipStream_t st) {
  const int nout = epi == GEMV_SILU_MUL ? a.N / 2 : a.N;
  const dim3 mgrid((unsigned)((nout + 255) / 256), (unsigned)a.R);
  switch (epi) {
    case GEMV_STORE: hipLaunchKernelGGL(gemv_rows_merge_kernel<GEMV_STORE>, mgrid, dim3(256), 0, st, a, nks); break;
    case GEMV_RESIDUAL: hipLaunchKernelGGL(gemv_rows_merge_kernel<GEMV_RESIDUAL>, mgrid, dim3(256), 0, st, a, nks); break;
    case GEMV_SILU_MUL: hipLaunchKernelGGL(gemv_rows_merge_kernel<GEMV_SILU_MUL>, mgrid, dim3(256), 0, st, a, nks); break;
    default: hipLaunchKernelGGL(gemv_rows_merge_kernel<GEMV_LOGITS>, mgrid, dim3(256), 0, st, a, nks); break;
  }
}

void launch_argmax_rows(const float* blk_max, const uint32_t* blk_idx, int ntiles, int rows, uint32_t* out, hipStream_t st) {
  if (rows <= 0) return;
  hipLaunchKernelGGL(argmax_rows_kernel, dim3((unsigned)rows), dim3(256), 0, st, blk_max, blk_idx, ntiles, out);
}

void launch_gen_embed(const void* table, const uint32_t* tok_in, const int32_t* row_tab, int rows, void* x, int H, const float* inv_freq,
                      const int32_t* axis_map, float* rope, hipStream_t st) {
  if (rows <= 0) return;
  hipLaunchKernelGGL(gen_embed_kernel, dim3((unsigned)rows), dim3(256), 0, st, (const bf16_t*)table, tok_in, row_tab, (bf16_t*)x, H, inv_freq,
                     axis_map, rope);
}

int attn_decode_nsplit(int kv_len_after, int g, int max_nsplit) {
  // enqueue_decode_step's rule (model.hip): one block (4 waves = 4 KV units) per AHA_ATTN_PAGES_PER_BLOCK pages, at most max_nsplit, and
  // g * nsplit <= 1024 for the merge's LDS tables
  static const char* e_div = getenv("AHA_ATTN_PAGES_PER_BLOCK");
  const int div = e_div ? std::max(1, atoi(e_div)) : 4;
  const int npages = (kv_len_after + KV_PAGE_TOKENS - 1) / KV_PAGE_TOKENS;
  const int nsplit = (npages + div - 1) / div;
  return std::max(1, std::min(std::min(nsplit, max_nsplit), 1024 / g));
}

void launch_attn_decode_batch(const AttnDecodeBatchArgs& b, int rows, int max_nsplit_rows, hipStream_t st, bool append) {
  if (rows <= 0) return;
  const dim3 grid((unsigned)b.kvh, (unsigned)max_nsplit_rows, (unsigned)rows);
  if (append) hipLaunchKernelGGL(attn_decode_batch_kernel, grid, dim3(256), 0, st, b);
  else hipLaunchKernelGGL(attn_decode_rows_kernel, grid, dim3(256), 0, st, b);
}

void launch_kv_append_rows(const AttnDecodeBatchArgs& b, int rows, hipStream_t st) {
  if (rows <= 0) return;
  hipLaunchKernelGGL(kv_append_rows_kernel, dim3((unsigned)b.kvh, (unsigned)rows), dim3(64), 0, st, b);
}

void launch_spec_accept_rows(const uint32_t* argmax, const int32_t* row_tab, const int32_t* seq_tab, int n_seqs, uint32_t* out, hipStream_t st) {
  if (n_seqs <= 0) return;
  hipLaunchKernelGGL(spec_accept_rows_kernel, dim3((unsigned)((n_seqs + 63) / 64)), dim3(64), 0, st, argmax, row_tab, seq_tab, n_seqs, out);
}

void launch_spec_accept_split(const uint32_t* argmax, const int32_t* row_tab, const int32_t* seq_tab, int n_seqs, uint32_t* out, hipStream_t st) {
  if (n_seqs <= 0) return;
  hipLaunchKernelGGL(spec_accept_split_kernel, dim3((unsigned)((n_seqs + 63) / 64)), dim3(64), 0, st, argmax, row_tab, seq_tab, n_seqs, out);
}

}  // namespace aha
