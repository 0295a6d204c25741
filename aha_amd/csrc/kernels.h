// Host-callable launchers for the gfx950 kernels.  All pointers are device pointers; all launches are asynchronous
// on `st`.  Shapes/strides are in elements unless a name says bytes.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <utility>
#include <vector>

namespace aha {

// Paged KV cache view of ONE layer.  Page p of this layer lives at page_ptrs[p] + layer_off (bytes):
//   K block  [kvh][KV_PAGE_TOKENS * d]   fragment-major (common.h kpage_elem): the QK^T MFMA operand fragments, 1 KB each
//   V block  [kvh][d * KV_PAGE_TOKENS]   fragment-major (common.h vpage_elem): the P.V operand fragments, slot-permuted
struct KvLayer {
  const uint64_t* page_ptrs;  // device array, byte addresses of each logical page's layer-0 storage
  uint64_t layer_off;         // byte offset of this layer inside a page's slab slot
  int kvh, d;
};

// GEMV_PARTIAL_F32: tensor-parallel row-split projection -- y_f32[n] = un-rounded f32 partial sum over this rank's K slice
enum GemvEpi { GEMV_STORE = 0, GEMV_RESIDUAL = 1, GEMV_SILU_MUL = 2, GEMV_LOGITS = 3, GEMV_PARTIAL_F32 = 4 };

struct GemvArgs {
  const void* W;         // (N,K) bf16 row-major; for GEMV_SILU_MUL the gate matrix (I,K)
  const void* W2;        // GEMV_SILU_MUL: the up matrix (I,K)
  const void* x;         // (K) bf16
  const void* norm_w;    // optional (K) bf16: fuse h = RMSNorm(x; norm_w, eps)
  const void* residual;  // GEMV_RESIDUAL: (N) bf16, may alias y
  void* y;               // (N) bf16   [GEMV_LOGITS: unused]
  float* y_f32;          // GEMV_LOGITS: (N) f32 logits
  float* blk_max;        // GEMV_LOGITS: per-tile (max value, index) partials for the on-device argmax
  uint32_t* blk_idx;
  void* h_out;           // optional (K) bf16: block 0 also writes the normalised input (debug / last hidden)
  int N, K;
  float eps;
  int cached;            // 0 (default): non-temporal weight loads (streamed once); 1: default cache policy
  unsigned long long* trace;  // optional (AHA_GEMV_TRACE): 100 MHz stamps of blocks 0 / 255 / last: start, issued, prologue done,
                              // first group consumed, last group consumed, end
  // the weight copies' launches (launch_gemv_mxfp8 / _mxfp4 / _pk13) fill these in, with W = the copy; callers leave them alone
  const uint8_t* scales;  // MXFP8 / MXFP4: the scale words of "MXFP8 weight copies" as bytes: byte k / 32 of a row of 4 * ceil(K / 128)
  int bh;                 // 13-bit copy: the matrix's exponent base: code h != 0 is E >> 1 == bh + h
};
void launch_gemv(const GemvArgs& a, GemvEpi epi, hipStream_t st);
int gemv_num_tiles(int N, int K);  // number of (max,idx) partials GEMV_LOGITS writes
void debug_plan_gemv(int N, int K, GemvEpi epi, bool has_norm, int* out5);   // host only: {R, U, grid, FAST, PRO} of launch_gemv; N = output rows

void launch_argmax_partials(const float* blk_max, const uint32_t* blk_idx, int n, uint32_t* out, hipStream_t st);
// vocab-parallel lm_head (tensor parallelism): per-rank (max, global index) pair into a zeroed 2T vector / pick after the all-reduce
void launch_argmax_pair(const float* blk_max, const uint32_t* blk_idx, int n, int row0, float* pairs, int rank, int T, hipStream_t st);
void launch_argmax_pick(const float* pairs, int T, uint32_t* out, hipStream_t st);
void launch_argmax_f32(const float* x, int64_t n, float* ws_max, uint32_t* ws_idx, uint32_t* out, hipStream_t st);

// D11 candidates (kernels_sample.hip): repeat penalty into a working copy of the logits; k largest + full-vocabulary softmax
// normaliser.  cand_* hold (sample_stage1_waves(V) + 16) * 64 entries (stage-1 candidates, then the 16 x k intermediates),
// part_* one entry per stage-1 wave, out_ms = {max, sumexp}.
int sample_stage1_waves(int V);
bool sample_shape_ok(int V, int k);
void launch_repeat_penalty(const float* logits, float* work, const uint32_t* ctx, int n, float penalty, int V, hipStream_t st);
void launch_topk_candidates(const float* x, int V, int k, float inv_temp, float* cand_val, unsigned* cand_idx, float* part_m,
                            float* part_s, float* out_val, unsigned* out_idx, float* out_ms, hipStream_t st);
// The same pipeline for `rows` rows of f32 logits (pitch ld) in one launch per stage (stage 0: stage 1, 1: stage 2a, 2: stage 2b; the
// caller scopes each for the profile), row s of `tab` (device, SAMPLE_ROW_WORDS int32 per row) naming its logits row, k, 1/T, penalty and
// context slice of `ctx` (distinct ids < V).  Row s: cand_* [s * (sample_stage1_waves(V) + 16) * 64, ...), part_* [s * nw, ...), out
// [s * SAMPLE_OUT_WORDS, ...) = {vals[64] f32, max, sumexp, idx[64] u32}.  Bit-identical per row to launch_repeat_penalty +
// launch_topk_candidates on that row; the logits are only read.
// Addends (logit_bias, presence / frequency penalties): row s adds adj_val[i] to the penalised logit of adj_id[i] for i in
// [ADJ0, ADJ0 + NADJ) -- ids sorted ascending, distinct and < V; NADJ == 0 (adj_* may then be null): the row's work is what it was
// before addends existed.
// Allowed-token masks: row s with MASK = i >= 0 reads the ceil(V / 32) words masks[i * ceil(V / 32) ..) -- id t is allowed iff bit t & 31 of
// word t >> 5 is set, and every other penalised, adjusted logit becomes -inf before the max; MASK < 0 (masks may then be null): no mask.
constexpr int SAMPLE_ROW_WORDS = 9;
constexpr int SAMPLE_ROW_LROW = 0, SAMPLE_ROW_K = 1, SAMPLE_ROW_INVT = 2, SAMPLE_ROW_PEN = 3, SAMPLE_ROW_CTX0 = 4, SAMPLE_ROW_NCTX = 5;
constexpr int SAMPLE_ROW_ADJ0 = 6, SAMPLE_ROW_NADJ = 7, SAMPLE_ROW_MASK = 8;
constexpr int SAMPLE_OUT_WORDS = 64 + 2 + 64;
void launch_topk_rows(const float* logits, int64_t ld, int V, int rows, const int32_t* tab, const uint32_t* ctx, float* cand_val,
                      unsigned* cand_idx, float* part_m, float* part_s, float* out, int stage, hipStream_t st,
                      const uint32_t* adj_id = nullptr, const float* adj_val = nullptr, const uint32_t* masks = nullptr);

// Per-token log-probabilities (kernels_logprob.hip) for `rows` rows of f32 logits (pitch ld), one launch per stage (stage 0: stage 1,
// 1: stage 2; the caller scopes each for the profile).  Row s of `tab` (device, LOGPROB_ROW_WORDS int32 per row): its logits row, its n_top
// (0 .. LOGPROB_MAX_TOP), the entry of `tokens` (device) that holds its token, and the row of `sample_out` (launch_topk_rows' out; -1:
// none) whose 64 candidate ids it gathers raw logits for.  Row s: cand_* [s * nw * LOGPROB_MAX_TOP, ...) with nw = logprob_stage1_waves(V),
// part_* [s * nw, ...), out [s * LOGPROB_OUT_WORDS, ...) = {an aha_token_logprobs (lp(token), n_top, ids[20], lps[20]), M, log S,
// raw[64]}.  Temperature 1, no penalty; a row's output depends on its own row only; the logits are only read.
constexpr int LOGPROB_MAX_TOP = 20;
constexpr int LOGPROB_ROW_WORDS = 4;
constexpr int LOGPROB_ROW_LROW = 0, LOGPROB_ROW_NTOP = 1, LOGPROB_ROW_TOK = 2, LOGPROB_ROW_CSLOT = 3;
constexpr int LOGPROB_OUT_LP = 0, LOGPROB_OUT_NTOP = 1, LOGPROB_OUT_IDS = 2, LOGPROB_OUT_LPS = 2 + LOGPROB_MAX_TOP;
constexpr int LOGPROB_OUT_M = 2 + 2 * LOGPROB_MAX_TOP, LOGPROB_OUT_LOGS = LOGPROB_OUT_M + 1, LOGPROB_OUT_RAW = LOGPROB_OUT_M + 2;
constexpr int LOGPROB_OUT_WORDS = LOGPROB_OUT_RAW + 64;
int logprob_stage1_waves(int V);
bool logprob_shape_ok(int V);
void launch_logprob_rows(const float* logits, int64_t ld, int V, int rows, const int32_t* tab, const uint32_t* tokens, float* cand_val,
                         unsigned* cand_idx, float* part_m, float* part_s, const float* sample_out, float* out, int stage, hipStream_t st);

void launch_embed_gather(const void* table, const uint32_t* ids, void* out, int S, int H, hipStream_t st);
void launch_rmsnorm_rows(const void* x, const void* w, void* y, int64_t rows, int dim, int64_t ldx, int64_t ldy,
                         float eps, hipStream_t st);
// Packed multi-sequence embedding (model_embed_batch): for every segment {row0, len, page0} of seg_tab, the last row x[row0 + len - 1]
// -> final RMSNorm (rmsnorm_rows_kernel's arithmetic, bf16 result) -> f32 -> x / sqrt(sum x^2 + 1e-6) -> out[segment] (dim floats)
void launch_embed_pool(const void* x, const int32_t* seg_tab, int n_segs, const void* w, float* out, int dim, float eps, hipStream_t st);

struct RopeArgs {
  const void* qkv;      // (S, ld) bf16: [q heads | k heads | v heads] per token
  int64_t ld;
  const void* q_norm_w; // (d) bf16
  const void* k_norm_w;
  const int32_t* pos;   // (3, pos_ld) rows T,H,W
  int64_t pos_ld;
  const float* inv_freq;    // (d/2)
  const int32_t* axis_map;  // (d/2) frequency slot -> row of pos
  void* q_out;          // (S, nh*d) bf16
  // paged destination (kv.page_ptrs != nullptr) or contiguous token-major k_out/v_out (S, kvh*d)
  KvLayer kv;
  const int32_t* kv_start;  // device scalar: cache position of token 0 of this call
  void* k_out;
  void* v_out;
  int S, nh, kvh, d;
  float eps;
  int kv_start_host = -1;   // the same value as *kv_start when the caller knows it on the host (prefill): selects the row-vectorised kernel
  const void* rope_tab = nullptr;  // optional (S, 128) bf16: cos[64] | sin[64] of every token's angles (launch_rope_table), else computed in place
  int skip_q = 0;           // row-vectorised prefill kernel only: the q heads are normed and rotated by the attention kernel's Q load (AttnPrefillArgs::q_norm_w); K and V only here
  // Packed independent sequences (row-vectorised kernel only; model_embed_batch): row r's K / V go to cache slot row_slot[r] instead of
  // kv_start_host + r, and page p of 0 .. n_pages-1 takes its V rows from page_rows[2p] .. + page_rows[2p + 1] (its first packed row, row count)
  const int32_t* row_slot = nullptr;
  const int32_t* page_rows = nullptr;
  int n_pages = 0;
};
void launch_qknorm_rope(const RopeArgs& a, hipStream_t st);
// cos / sin of pos[axis(i)] * inv_freq[i], rounded to bf16 as apply_rotary_pos_emb casts them (rope.rs:96-132): computed ONCE per
// prefill for all layers (precise cosf / sinf of angles up to 1e5 rad cost more than the rest of the rope kernel)
void launch_rope_table(const int32_t* pos, int64_t pos_ld, const float* inv_freq, const int32_t* axis_map, int S, void* tab, hipStream_t st);

// contiguous token-major (L, kvh*d) K,V -> pages (op-level tests and TP KV gather)
void launch_kv_pack_pages(const void* k, const void* v, KvLayer kv, int L, hipStream_t st);

struct AttnDecodeArgs {
  const void* q;           // (nh*d) bf16, normed + roped
  KvLayer kv;
  const int32_t* kv_len;   // device scalar: number of valid tokens (including the one just appended)
  float* part_o;           // workspace (nsplit, nh, d) f32 un-normalised
  float* part_ml;          // workspace (nsplit, nh, 2) running max / sum
  void* o;                 // (nh*d) bf16
  int nh, kvh, d, nsplit;
  float scale;
};
void launch_attn_decode(const AttnDecodeArgs& a, hipStream_t st);

// Fused decode step of the attention block: q/k norm + rope + KV append + split-KV attention (kernels_attn.hip).
// The last split block of a kv head to finish merges the nsplit partials of the head's query heads and writes the bf16
// attention output (o); head_ctr / ctr_target decide who is last (monotonic counters, one 128-byte line per kv head).
struct AttnDecodeFusedArgs {
  const void* qkv;          // ((nh+2kvh)*128) bf16: output of the fused QKV matvec
  const void* q_norm_w;     // (128) bf16
  const void* k_norm_w;
  const float* rope;        // (128) f32: cos[64], sin[64] of the step's rope angles, already rounded to bf16 values
                            // (rope_step_kernel: once per step instead of once per layer and block)
  KvLayer kv;
  // Linear form (lin_step != 0): every page the launch touches -- pages 0 .. kv_start_v / KV_PAGE_TOKENS -- is at lin_page0 + i * lin_step
  // (lin_page0 includes the layer offset) and the kernel forms the addresses by arithmetic instead of reading kv.page_ptrs.  Set by
  // the single-request decode step when the model's page map is such a progression (model.h lin_pages); 0: the table form.
  uint64_t lin_page0 = 0;
  int64_t lin_step = 0;
  int kv_start_v;           // cache slot of the token (host value: the step is enqueued with its lengths known)
  int kv_len_v;             // cache length after the append (= kv_start_v + 1)
  float* part_o;            // (nsplit, nh, 128) f32
  float* part_ml;           // (nsplit, nh, 2) f32
  void* o;                  // (nh*128) bf16 attention output
  unsigned* head_ctr;       // [32 * kvhd]: split blocks of the head that have published their partial (all launches)
  unsigned ctr_target;      // value head_ctr reaches when this launch's nsplit blocks have all arrived
  unsigned long long* trace;  // optional timeline (AHA_ATTN_TRACE)
  int nh, kvh, nsplit;
  float eps, scale;
};
void launch_attn_decode_fused(const AttnDecodeFusedArgs& a, hipStream_t st);

struct AttnPrefillArgs {
  const void* q;           // (S, nh*d) bf16
  KvLayer kv;
  void* o;                 // (S, nh*d) bf16
  int S, nh, kvh, d;
  int kv_offset;           // q row i sees cache positions <= kv_offset + i (causal) or < kv_total (full)
  int kv_total;            // number of valid cache tokens
  int causal;
  float scale;
  int64_t q_ld;            // elements between consecutive q rows; 0 => nh * padded head dim
  int nqb;                 // set by the launcher: > 0 selects the XCD-aware 1-D block order over nqb q blocks x nh heads
  // Optional second causal segment in the same launch (context-parallel rank: its late chunk): q / o rows [S, S + S2) of the same
  // buffers, row S + i sees cache positions <= kv_offset2 + i, < kv_total2.  Needs causal; one launch where the XCD-aware order
  // applies (the late segment's blocks first, the early one's fill its last round), else two launches.
  int S2 = 0, kv_offset2 = 0, kv_total2 = 0;
  int epi_rows = 0;        // set by the launcher: output rows stored in row order through LDS (16 B per lane)
  // head_dim 72 only: every real token's V^T pad row 72 holds 1.0 (kernels_vit.hip vit_rope_pack_kernel), so output row 72 of V^T . P^T is
  // the softmax row sum and the f32-chain kernels may drop their own.  Only the packer that wrote the pages can promise it: unset, the
  // kernels keep the f32 sum of the probabilities.
  int v_ones_row = 0;
  // Rows of the WHOLE request this launch is a part of (0 = S + S2).  The automatic choice of the kernel form goes by it, so that a
  // context-parallel rank's share of a prompt runs the form the un-sharded prompt would: the forms agree to the parity bound, not bit for bit
  // (another MFMA shape = another accumulation order), and tests/test_cp_gpu.py demands bit-identical rows.
  int rows_hint = 0;
  // q-norm + RoPE of Q inside the kernel's Q load (round 6; head_dim 128, the 16-rows-per-wave kernel): `q` then points at the RAW q heads of
  // the qkv GEMM's output (q_ld = its row stride), q_norm_w = the (128) bf16 RMSNorm weight, q_rope_tab = the (rows, 128) bf16 cos | sin
  // table of launch_rope_table for the same rows as q, q_eps the norm's epsilon.  Same operations in the same order as qknorm_rope_rows_kernel
  // (bit-identical q); ask attn_prefill_takes_qfuse first -- the 64-row form does not take it.
  const void* q_norm_w = nullptr;
  const void* q_rope_tab = nullptr;
  float q_eps = 0.f;
  // Packed independent sequences (the 16-rows-per-wave kernel, 4 waves): seg_tab = (segments, 3) int32 {row0, len, page0} on the device --
  // segment j is q / o rows row0 .. row0 + len - 1 and its cache positions 0 .. len - 1 live on pages page0, page0 + 1, ... of
  // kv.page_ptrs; seg_items = (n_items, 2) int32 {segment, 64-row q block}, most expensive first.  One block per (item, head); S = the
  // packed rows, kv_offset / kv_total / S2 unused.  Causal (model_embed_batch, generate_batch: head_dim 128, raw q heads with q_norm_w), or
  // non-causal (the ViT's block-diagonal attention, vision_tower.hip: head_dim 72, q rows in the (N, nh, 96) layout, v_ones_row; the audio
  // encoder's, audio_tower.hip: head_dim 64, q rows of the fused qkv activation with q_ld = 3 * D); a row's bits are those of its segment's
  // own launch on the 16-row kernel.
  const int32_t* seg_tab = nullptr;
  const int32_t* seg_items = nullptr;
  int n_items = 0;
  // Optional cache prefix per segment (causal seg_tab launches; the engine's chunked prefill): seg_kv0 = (segments) int32 on the device.
  // Segment j's q rows are then its cache positions kv0 .. kv0 + len - 1, row i seeing keys 0 .. kv0 + i on pages page0, page0 + 1, ...
  // (the prefix's pages first).  nullptr = every kv0 0: the launch is the one without the field, bit for bit.
  const int32_t* seg_kv0 = nullptr;
};
// The seg_items of a host seg_tab ({row0, len, page0} per segment): {segment, 64-row q block} pairs in segment order, then stable-sorted
// most expensive first.  Causal: a block costs the keys its last row sees, kv0 + min(len, (b + 1) * 64) (kv0: the segment's cache prefix,
// AttnPrefillArgs::seg_kv0; none = 0); non-causal: its segment's length.
inline std::vector<int32_t> seg_items_of(const std::vector<int32_t>& seg_tab, bool causal, const std::vector<int32_t>* kv0 = nullptr) {
  constexpr int QB = 64;   // q rows per block (launch_attn_prefill: 4 waves with seg_tab)
  std::vector<std::pair<int32_t, int32_t>> items;
  for (size_t j = 0; 3 * j < seg_tab.size(); ++j)
    for (int32_t b = 0; b * QB < seg_tab[3 * j + 1]; ++b) items.emplace_back((int32_t)j, b);
  auto cost = [&](const std::pair<int32_t, int32_t>& it) {
    const int32_t len = seg_tab[3 * (size_t)it.first + 1];
    return causal ? (kv0 ? (*kv0)[(size_t)it.first] : 0) + std::min(len, (it.second + 1) * QB) : len;
  };
  std::stable_sort(items.begin(), items.end(), [&](const auto& x, const auto& y) { return cost(x) > cost(y); });
  std::vector<int32_t> out;
  out.reserve(2 * items.size());
  for (const auto& it : items) out.push_back(it.first), out.push_back(it.second);
  return out;
}
void launch_attn_prefill(const AttnPrefillArgs& a, hipStream_t st);
bool attn_prefill_takes_qfuse(const AttnPrefillArgs& a);
int attn_prefill_form_of(const AttnPrefillArgs& a);       // the kernel form launch_attn_prefill takes: 0 = the 16-rows-per-wave kernel, 64 / 65   // would launch_attn_prefill run a kernel that norms + rotates Q itself for these arguments?
// the one-wave-per-SIMD, 64-q-rows-per-wave form (kernels_attn64.hip); false = not a shape of that kernel, nothing launched
bool launch_attn_prefill64(const AttnPrefillArgs& a, hipStream_t st, int pipe);
void set_attn_form_override(int form);     // test hook: -1 = automatic, 16 = the 16-rows-per-wave kernel, 64 / 65 = the 64-row kernel (plain / pipelined)
void set_attn_variant_override(int smx);   // test hook: -1 = the environment's / default choice

// ACT_PARTIAL_F32: tensor-parallel row-split projection -- C is (M,N) f32, the un-rounded partial sums over this rank's K slice
enum GemmAct { ACT_NONE = 0, ACT_GELU_TANH = 1, ACT_GELU_ERF = 2, ACT_SILU = 3, ACT_SILU_MUL_PAIRS = 4, ACT_PARTIAL_F32 = 5 };
struct GemmArgs {
  const void* A;  // (M,K) bf16, row stride lda
  const void* W;  // (N,K) bf16, row stride ldw
  void* C;        // (M,N) bf16, row stride ldc   [ACT_SILU_MUL_PAIRS: (M,N/2)]
  const void* bias;      // optional (N) bf16
  const void* residual;  // optional (M,N) bf16 with stride ldc, may alias C
  int M, N, K;
  int64_t lda, ldw, ldc;
  int act;
  // RMSNorm of the finished output rows as part of the call (candle_nn::RmsNorm over N, weight norm_w (N) bf16): norm_out (M, N)
  // bf16, row pitch N.  Where the plan ends in a split-K reduce pass the norm runs inside it (the pass holds the finished row in
  // registers); otherwise launch_gemm appends launch_rmsnorm_rows -- the same values either way.
  const void* norm_w = nullptr;
  void* norm_out = nullptr;
  float norm_eps = 0.f;
  // norm_b != nullptr: the riding norm is a LayerNorm (candle_nn::LayerNorm, weight norm_w + bias norm_b over N: the ViT block's norm1 /
  // norm2, /root/reference/src/models/qwen3vl/model.rs:346-370) instead of an RMSNorm.  Folded into a split-K reduce pass where the plan has
  // one (gemm_splitk_reduce_layernorm_kernel), else launch_gemm appends launch_layernorm_rows: the same bits either way.
  const void* norm_b = nullptr;
  void* workspace = nullptr;     // optional f32 scratch for split-K slabs (splitk * M * N * 4 bytes) / the persistent kernel's chunks
  size_t workspace_bytes = 0;
  void* sk_counters = nullptr;   // optional SK_MAX_COUNTERS zeroed u32 words that belong to `workspace` (one per tile cut along K by the
                                 // persistent kernel, kernels_gemm_sk.hip; every launch leaves them zero again)
  int tile_group = 8;            // band width of the grouped tile order inside an XCD's run (kernels_gemm.hip tile_of_block); 0 = plain
  int partial_rows = 1;          // ACT_PARTIAL_F32 on the four-wave kernel: f32 sums stored in row order through LDS (0: fragment order; A/B)
  // Row groups (launch_gemm_grouped; tensor-parallel prefill: the staging layout of the chunked all-gather, csrc/model.hip
  // norm_gather_gemm): `groups` row segments of M rows each share W.  Segment g reads A rows [g * a_gstride, + M) and writes C rows
  // [c_row0 + g * c_gstride, + M), clipped to rows < m_total.
  int groups = 1, a_gstride = 0, c_gstride = 0, c_row0 = 0, m_total = 0;
};
void launch_gemm(const GemmArgs& a, hipStream_t st);
// One launch over all row segments on the four-wave 256 x 256 / 256 x 192 kernels (plain and gate+up epilogues, whole K tiles, M >= 256);
// any other shape: one launch_gemm per segment.  Every output element is the same K-ordered sum as in an ungrouped GEMM over its row.
void launch_gemm_grouped(const GemmArgs& a, hipStream_t st);
// split-K scratch used by launch_gemm calls of this THREAD whose GemmArgs carry none (the model sets it per forward)
void set_gemm_workspace(void* ws, size_t bytes, void* sk_counters = nullptr);
// ---- the persistent, segment-table-driven kernel (kernels_gemm_sk.hip) ----
constexpr int SK_MAX_COUNTERS = 4096;   // u32 words of GemmArgs::sk_counters
bool streamk_has_kernel(int act, bool has_bias, bool has_res, bool n192);
double streamk_estimate(const GemmArgs& a, int tile_n, int* n_chunks, int* n_split);   // k steps on the slowest worker; < 0: cannot plan
bool launch_gemm_streamk(const GemmArgs& a, int tile_n, hipStream_t st);               // false: nothing was launched
void set_streamk_forced_cut(int code);  // tests: style * 10 + cuts of the last round's tiles (style 0 = equal pieces, 1 = big + remainder); 0 = automatic
int gemm_streamk_workers();
int gemm_streamk_cus();                // CUs of the device, rounded down to a multiple of 8            // workgroups of the persistent kernel = CUs - reserved, a multiple of 8
int get_gemm_reserved_cus();           // the raw setting (-1 = unset)
void set_gemm_reserved_cus(int n);     // CUs the persistent GEMM leaves free (RCCL beside the GEMMs under TP); < 0: AHA_GEMM_RESERVE_CUS
bool acquire_gemm_cu_reservation(int cus);   // the automatic, reference-counted reservation of a communication stream (kernels_gemm_sk.hip)
void release_gemm_cu_reservation();
int debug_streamk_plan(int M, int N, int K, int tile_n, int workers, int group, size_t ws_bytes, int* out, int cap, int* off_out, int* info);
void debug_plan_gemm(int M, int N, int K, int act, bool has_bias, bool has_res, size_t ws_bytes, int* out, bool has_norm = false);   // host only: {tile, splitk, n_split}
void set_gemm_plan_override(int tile, int splitk);  // tests: force the 128 / 256 tile kernel and a split-K factor; 0 = automatic
void get_gemm_workspace(void** ws, size_t* bytes, void** sk_counters);
struct GemmWorkspaceScope {   // nests: the vision tower's own workspace inside the prefill's
  GemmWorkspaceScope(void* ws, size_t bytes, void* sk_counters = nullptr) {
    get_gemm_workspace(&prev_ws, &prev_bytes, &prev_ctrs);
    set_gemm_workspace(ws, bytes, sk_counters);
  }
  ~GemmWorkspaceScope() { set_gemm_workspace(prev_ws, prev_bytes, prev_ctrs); }
  GemmWorkspaceScope(const GemmWorkspaceScope&) = delete;
  GemmWorkspaceScope& operator=(const GemmWorkspaceScope&) = delete;
  void* prev_ws = nullptr;
  size_t prev_bytes = 0;
  void* prev_ctrs = nullptr;
};
// x[i] = bf16(x[i] + bf16(sum[i])): Linear output tensor (all-reduced f32 partials) -> bf16, then the residual add -> bf16
void launch_residual_add_f32(void* x, const float* sum, int64_t n, hipStream_t st);
void launch_poison_lds(uint32_t seed, hipStream_t st);
void launch_residual_add_f32_cols(void* x, int64_t ldx, const float* sum, int64_t lds, int64_t rows, int cols, hipStream_t st);
void launch_row_to_f32(const void* x_bf16_or_null, float* out, int n, hipStream_t st);   // nullptr: zeros
void launch_f32_to_row(const float* x, void* out_bf16, int n, hipStream_t st);

// ---- multi-sequence decode (kernels_batch.hip; model_generate_batch) ----------------------------------------------------
// y[R, N] = x[R, K] . W[N, K]^T for 1 <= R <= 32 rows, the weights streamed once.  Two launches: gemv_rows_kernel (f32 partials of the
// K splits into ws) and the merge (fixed-order sum + epilogue).  Every output element's summation order depends on (N, K) only.
// Epilogues: GEMV_STORE / GEMV_RESIDUAL (y = bf16(residual + bf16(lin)), residual may alias y) / GEMV_SILU_MUL (W in the 16-row gate / up
// block layout of ACT_SILU_MUL_PAIRS, N = 2I, y is (R, I)) / GEMV_LOGITS (y_f32 (R, ldf) f32 + per-(row, 256-column tile) (max, index)
// partials, gemv_rows_num_tiles(N) per row).
struct GemvRowsArgs {
  const void* W;
  const void* x;       // (R, ldx) bf16
  const void* residual;
  void* y;             // (R, ldy) bf16
  float* y_f32;        // GEMV_LOGITS
  float* blk_max;      // GEMV_LOGITS: (R, gemv_rows_num_tiles(N))
  uint32_t* blk_idx;
  float* ws;           // gemv_rows_ws_floats(R, N, K) f32
  int R, N, K;         // K % 8 == 0
  int64_t ldx, ldy, ldf;
  int64_t ldws = 0;    // set by the launcher
};
void launch_gemv_rows(const GemvRowsArgs& a, GemvEpi epi, hipStream_t st);
void launch_gemv_rows_merge(const GemvRowsArgs& a, GemvEpi epi, int nks, hipStream_t st);   // the call's second launch alone (a.ldws set)
// MXFP8 weight copies (kernels_gemv_rows_fp8.hip, mxfp8.h): a bf16 matrix W (N, K), K % 32 == 0, as
//   q       (N, K) bytes, row-major: OCP E4M3 (e4m3fn) codes of w / 2^e, e the exponent of the element's block of 32 consecutive k
//   scales  (N, ceil(K / 128)) u32: word (n, c) holds the E8M0 bytes e + 127 of row n's blocks 4c .. 4c + 3, block 4c + g in bits
//           8g .. 8g + 7 -- the four lane groups of a column in chunk c of gemv_rows share one dword load; bytes of blocks past K are 127
// launch_gemv_rows_mxfp8 is launch_gemv_rows with (q, scales) in place of a.W (ignored) -- the same kernel body with another weight
// form (gemv_rows_body.h) -- and bit-identical to launch_gemv_rows on W' = q * 2^e.  launch_mxfp8_quantize writes q, scales and (optional, may be w itself) W'; launch_mxfp8_check ORs 1 into *flag when a
// weight is non-finite or would round past bf16's range (|w| >= 1.9375 * 2^127).
struct WQuant {
  void* q = nullptr;
  uint32_t* scales = nullptr;
};
size_t mxfp8_scale_words(int N, int K);
void launch_gemv_rows_mxfp8(const GemvRowsArgs& a, const void* q, const uint32_t* scales, GemvEpi epi, hipStream_t st);
void launch_mxfp8_quantize(const void* w, int N, int K, void* q_out, uint32_t* scales_out, void* w_roundtrip_out, hipStream_t st);
void launch_mxfp8_check(const void* w, int64_t n_elems, int* flag, hipStream_t st);
// Batch-1 matvec from the same copies (kernels_gemv_fp8.hip): launch_gemv with (q, scales) in place of g.W / g.W2 (ignored; GEMV_SILU_MUL
// reads the fused 16-row gate / up block layout, g.N = I), g.cached and g.trace ignored, no GEMV_PARTIAL_F32.  Bit-identical to launch_gemv
// on W' = q * 2^e.  GEMV_LOGITS writes gemv_mxfp8_num_tiles(N, K) (max, index) partials -- its own plan's grid, not gemv_num_tiles'.
void launch_gemv_mxfp8(const GemvArgs& g, const void* q, const uint32_t* scales, GemvEpi epi, hipStream_t st);
int gemv_mxfp8_num_tiles(int N, int K);
bool gemv_mxfp8_by_plan(int N, int K, GemvEpi epi);   // does the model's single-sequence step read this matrix (N rows: 2I for gate+up) from its copy?
void debug_plan_gemv_mxfp8(int N, int K, GemvEpi epi, bool has_norm, int* out5);   // host only: {R, U, grid, FAST, PRO}; N = output rows
// MXFP4 weight copies (kernels_gemv_rows_fp4.hip, mxfp4.h): the same blocks and the same scale words as MXFP8, with
//   q       (N, K / 2) bytes, row-major: OCP E2M1 codes (sign << 3 | index into {0, 0.5, 1, 1.5, 2, 3, 4, 6}) of w / 2^e, byte (n, k / 2)
//           holds even k in bits 0..3 and odd k in bits 4..7 -- a lane's MX block of gemv_rows is one 16-byte load
// launch_gemv_rows_mxfp4 is launch_gemv_rows with (q, scales) in place of a.W (ignored) -- the third weight form of the one kernel body
// (gemv_rows_body.h) -- and bit-identical to launch_gemv_rows on W' = q * 2^e.  launch_mxfp4_quantize writes q, scales and (optional, may be w itself) W'; launch_mxfp4_check ORs 1 into *flag when a
// weight is non-finite or above 1.5 * 2^127 in magnitude (it would round past 6 * 2^125).
void launch_gemv_rows_mxfp4(const GemvRowsArgs& a, const void* q, const uint32_t* scales, GemvEpi epi, hipStream_t st);
void launch_mxfp4_quantize(const void* w, int N, int K, void* q_out, uint32_t* scales_out, void* w_roundtrip_out, hipStream_t st);
void launch_mxfp4_check(const void* w, int64_t n_elems, int* flag, hipStream_t st);
// Batch-1 matvec from the MXFP4 copies (kernels_gemv_fp4.hip): launch_gemv_mxfp8's twin, the same body with the other weight form, and
// bit-identical to launch_gemv on W' = q * 2^e.  GEMV_LOGITS writes gemv_mxfp4_num_tiles(N, K) (max, index) partials, its own plan's grid.
void launch_gemv_mxfp4(const GemvArgs& g, const void* q, const uint32_t* scales, GemvEpi epi, hipStream_t st);
int gemv_mxfp4_num_tiles(int N, int K);
bool gemv_mxfp4_by_plan(int N, int K, GemvEpi epi);   // as gemv_mxfp8_by_plan, for a model with MXFP4 copies
void debug_plan_gemv_mxfp4(int N, int K, GemvEpi epi, bool has_norm, int* out5);   // host only: {R, U, grid, FAST, PRO}; N = output rows
// Exact 13-bit copies (kernels_gemv_pk13.hip has the format): a bf16 matrix W (N, K), K % 4096 == 0, as pk13_bytes(N, K) = 0.8125 of its
// bytes plus one exponent base bh.  launch_pk13_stats (stats zeroed by the caller) leaves the maximum of E >> 1 over the finite weights and
// the count of weights the format cannot hold (Inf / NaN, non-zero values more than 30 binades below the maximum): a matrix with
// bad == 0 is packed as it is, with bh = pk13_base(max_e2) (exception rows: below).  launch_gemv_pk13 is launch_gemv with (packed, bh) in place of g.W / g.W2 (ignored;
// GEMV_SILU_MUL reads the fused 16-row gate / up block layout, g.N = I), g.cached and g.trace ignored, no GEMV_PARTIAL_F32, and
// gemv_pk13_shape_ok(g.N, g.K) required.  Bit-identical to launch_gemv on W.  GEMV_LOGITS writes gemv_pk13_num_tiles(N, K) partials.
// Exception rows: a finite weight below the window does not keep its matrix from being packed as long as at most PK13_MAX_EXC rows hold
// one (a condition of the format, not a tuned figure: the kernel keeps the list in SGPRs).  The copy has an arbitrary code at such a weight;
// launch_gemv_pk13 with (rows, nrows) -- rows of W in W's own order, GEMV_SILU_MUL: of the fused matrix, g.W the bf16 matrix -- launches the
// twin kernel gemv_kernel_rows_pk13, which computes those rows from W itself with the bf16 kernel's chain: still bit-identical to
// launch_gemv on W.  nrows == 0 is the plain kernel.  Inf / NaN (Pk13Stats::nonfinite) keep a matrix unpacked.
constexpr int PK13_MAX_EXC = 16;
struct Pk13Stats {
  int max_e2;
  int over;                       // more than PK13_MAX_EXC rows hold a finite weight below the window
  unsigned long long bad;         // all weights the format cannot hold: nonfinite + finite below the window
  unsigned long long nonfinite;   // Inf / NaN
  int row1[PK13_MAX_EXC];         // the rows with a finite weight below the window, + 1, in the order found; 0: free
};
__host__ __device__ inline int pk13_base(int max_e2) { return max_e2 > 15 ? max_e2 - 15 : 0; }
size_t pk13_bytes(int N, int K);
void launch_pk13_stats(const void* w, int N, int K, Pk13Stats* stats, hipStream_t st);
// host: the rows of s ascending into rows[PK13_MAX_EXC] (unused entries -1); returns their number, PK13_MAX_EXC + 1 if there are more
int pk13_exception_rows(const Pk13Stats& s, int* rows);
void launch_pk13_pack(const void* w, int N, int K, int bh, void* out, hipStream_t st);
bool gemv_pk13_shape_ok(int N, int K);
void launch_gemv_pk13(const GemvArgs& g, const void* packed, int bh, GemvEpi epi, hipStream_t st);
void launch_gemv_pk13(const GemvArgs& g, const void* packed, int bh, const int* rows, int nrows, GemvEpi epi, hipStream_t st);
int gemv_pk13_num_tiles(int N, int K);
bool gemv_pk13_by_plan(int N, int K, GemvEpi epi);   // does the model's single-sequence step read this matrix (N rows: 2I for gate+up) from its copy?
void debug_plan_gemv_pk13(int N, int K, GemvEpi epi, bool has_norm, int* out5);   // host only: {R, U = 8, grid, FAST = 1, PRO}; N = output rows
void gemv_rows_plan(int N, int K, int* chunks_per_wave, int* k_splits);
int gemv_rows_num_tiles(int N);
size_t gemv_rows_ws_floats(int R, int N, int K);
void launch_argmax_rows(const float* blk_max, const uint32_t* blk_idx, int ntiles, int rows, uint32_t* out, hipStream_t st);

// Per-step row table of the batched decode, GEN_ROW_WORDS int32 per active row
constexpr int GEN_ROW_WORDS = 8;
constexpr int GEN_ROW_PAGE0 = 0;   // first logical page of the row's sequence (its pages are consecutive)
constexpr int GEN_ROW_KVLEN = 1;   // cache length after this step's append
constexpr int GEN_ROW_NSPLIT = 2;  // KV splits (attn_decode_nsplit of the row's own length)
constexpr int GEN_ROW_CTR = 3;     // the row's split-arrival counters before this step (the layer's target: + ctr_step * nsplit)
constexpr int GEN_ROW_POS = 4;     // rope position of the step's token
constexpr int GEN_ROW_SRC = 5;     // row of the previous step's token vector that holds this row's input token
constexpr int GEN_ROW_CTRROW = 6;  // which (kvh, 32) block of head_ctr holds the row's counters (generate_batch: the row; the engine: its slot)
constexpr int GEN_ROW_TOK = 7;     // draft-and-verify steps: the row's input token, uploaded with the table (then SRC = r * GEN_ROW_WORDS + GEN_ROW_TOK
                                   // with the table itself as the token vector); 0 elsewhere
void launch_gen_embed(const void* table, const uint32_t* tok_in, const int32_t* row_tab, int rows, void* x, int H, const float* inv_freq,
                      const int32_t* axis_map, float* rope, hipStream_t st);

// Fused decode attention of many sequences in one launch: block (kv head, split, row) runs attn_decode_fused_body with row r's qkv row,
// rope row, pages (page_ptrs + page0), lengths and split count; bit-identical per row to launch_attn_decode_fused on the same inputs.
struct AttnDecodeBatchArgs {
  const void* qkv;            // (rows, (nh + 2kvh) * 128) bf16
  const void* q_norm_w;
  const void* k_norm_w;
  const float* rope;          // (rows, 128) f32, bf16-representable
  const uint64_t* page_ptrs;  // logical page -> layer-0 byte address
  uint64_t layer_off;
  const int32_t* row_tab;     // (rows, GEN_ROW_WORDS) device
  float* part_o;              // (rows, max_nsplit, nh, 128)
  float* part_ml;             // (rows, max_nsplit, nh, 2)
  void* o;                    // (rows, nh * 128) bf16
  unsigned* head_ctr;         // (counter rows, kvh, 32) monotonic split-arrival counters; row r uses block row_tab[r].ctrrow
  int ctr_step;               // target of row r = row_tab[r].ctr + ctr_step * nsplit
  int nh, kvh, max_nsplit;
  float eps, scale;
};
// append = false: the rows' K/V are in their slots already (launch_kv_append_rows before it); the body's append is compiled out
void launch_attn_decode_batch(const AttnDecodeBatchArgs& a, int rows, int max_nsplit_rows, hipStream_t st, bool append = true);
// Draft-and-verify steps: (k roped, v raw) of every row into slot kv_len - 1 of its sequence, the bits of the fused kernel's own append
// (reads qkv, k_norm_w, rope, page_ptrs, layer_off, row_tab, nh, kvh, eps of the batch arguments)
void launch_kv_append_rows(const AttnDecodeBatchArgs& a, int rows, hipStream_t st);
// Per sequence s of a draft-and-verify step: seq_tab[s] = {first row, draft rows after it}; out[s] = {emitted count, row whose logits chose
// the last emitted token, the emitted tokens}: the longest draft prefix the argmax vector confirms, plus the token that follows it
constexpr int SPEC_MAX_DRAFT = 15;
constexpr int SPEC_SEQ_WORDS = 2, SPEC_SEQ_ROW0 = 0, SPEC_SEQ_NDRAFT = 1;
constexpr int SPEC_OUT_WORDS = 2 + SPEC_MAX_DRAFT + 1, SPEC_OUT_COUNT = 0, SPEC_OUT_LAST_ROW = 1, SPEC_OUT_TOKENS = 2;
void launch_spec_accept_rows(const uint32_t* argmax, const int32_t* row_tab, const int32_t* seq_tab, int n_seqs, uint32_t* out, hipStream_t st);
// The same for the engine's row layout (every request's own row first, the draft rows behind them): seq_tab[s] = {own row, first draft
// row, draft rows}; out[s] is the same record, the last row being the own row when no draft is confirmed
constexpr int ENG_SEQ_WORDS = 3, ENG_SEQ_ROW = 0, ENG_SEQ_DRAFT0 = 1, ENG_SEQ_NDRAFT = 2;
void launch_spec_accept_split(const uint32_t* argmax, const int32_t* row_tab, const int32_t* seq_tab, int n_seqs, uint32_t* out, hipStream_t st);
int attn_decode_nsplit(int kv_len_after, int g, int max_nsplit);   // enqueue_decode_step's split rule

struct StepState;  // model.h
// words the fused decode attention synchronises through (zeroed once at model creation, monotonic afterwards)
constexpr size_t DECODE_SYNC_BYTES = 32768;
constexpr int DECODE_HEAD_CTR_WORD = 6144;  // + 32 * kv head: split-arrival counters of the fused decode attention

}  // namespace aha

// ---- Qwen3-VL vision tower (kernels_vit.hip) -----------------------------------------------------------------------
namespace aha {
constexpr int VIT_DQK = 96;  // ViT head_dim 72: Q/K rows zero-padded to 3 MFMA k-steps
constexpr int VIT_DV = 80;   //                   V block zero-padded to 5 16-row sub-tiles
void launch_layernorm_rows(const void* x, const void* w, const void* b, void* y, int64_t rows, int dim, float eps,
                           hipStream_t st);
// x[n,:] += bilinear pos-embed: sum_i table[idx[i][n],:] * wt[i][n]  (4 corners), every op rounded as the reference
void launch_pos_embed_add(void* x, const void* table, const int32_t* idx, const float* wt, int64_t N, int D,
                          hipStream_t st);
struct VitRopeArgs {
  const void* qkv;          // (N, 3*nh*hd) bf16: [q heads | k heads | v heads]
  const int32_t* rowcol;    // (N, 2) patch (row, col)
  const float* inv_freq;    // (hd/4)
  const int32_t* page_of;   // (N) page index of token n
  const int32_t* slot_of;   // (N) slot (0..63) of token n inside its page
  void* q_out;              // (N, nh, VIT_DQK) bf16, zero padded
  KvLayer kv;               // pages: K block [nh][64][VIT_DQK], V block [nh][VIT_DV][64]
  int N, nh, hd;
  const float* cs_tab = nullptr;   // (N, hd/2, 2) f32: bf16-rounded (cos, sin) per patch and rotary lane (launch_vit_rope_table)
  const int32_t* page_first = nullptr;  // (n_pages) first token of each page (a page holds consecutive tokens of one segment)
  const int32_t* page_cnt = nullptr;    // (n_pages) tokens in the page (64 except a segment's last page)
  int n_pages = 0;
};
void launch_vit_rope_pack(const VitRopeArgs& a, hipStream_t st);
void launch_vit_rope_table(const int32_t* rowcol, const float* inv_freq, int N, int hd, float* tab, hipStream_t st);
void launch_scatter_rows(void* dst, const void* src, const int32_t* rows, int64_t n, int D, int add, hipStream_t st);
// image_pre.hip (V0-pre): img_smart_resize (img_utils.rs:294-331) and resize_exact(.., CatmullRom) of an RGB8 image on the device
int img_smart_resize(uint32_t h, uint32_t w, uint32_t factor, uint32_t min_pixels, uint32_t max_pixels, uint32_t* h_out, uint32_t* w_out);
// the video path's host arithmetic (video_utils.rs:9-59, qwen3vl/processor.rs:283-307,481-535); host only
int video_smart_resize(uint32_t num_frames, uint32_t h, uint32_t w, uint32_t temporal_factor, uint32_t factor, uint32_t min_pixels,
                       uint32_t max_pixels, uint32_t video_ratio, uint32_t* h_out, uint32_t* w_out);
int video_sample_frames(uint32_t total_frames, float rate, uint32_t fps, uint32_t min_frames, uint32_t max_frames, uint32_t* nframes,
                        uint32_t* interval);
int64_t video_timestamps(const uint32_t* frame_indices, size_t n, float fps, uint32_t t_merge, float* out, size_t cap);
int image_resize(const uint8_t* src, int H, int W, uint8_t* dst, int new_h, int new_w, hipStream_t st);
int debug_resize_taps(int n_in, int n_out, int32_t* left, int32_t* count, float* weights, int64_t weights_cap);
void launch_video_to_patches(const uint8_t* frames, void* out, int T, int H, int W, int patch, int merge, const float* mean,
                             const float* stdv, hipStream_t st);
void launch_image_to_patches(const uint8_t* img, void* out, int H, int W, int patch, int merge, const float* mean,
                             const float* stdv, hipStream_t st);
}  // namespace aha

// ---- Qwen3-ASR audio path (kernels_audio.hip) ----------------------------------------------------------------------
namespace aha {
// Log-mel of n_clips clips in one launch pair.  d_clips: (n_clips, LOGMEL_CLIP_WORDS) int64 {sample offset in x, L_j, first output column,
// F_j = L_j / 160, first block} with the blocks ascending, n_groups = sum of ceil(F_j / 4); out: (128, ld) f32, clip j's frames in its
// columns; frame_max: ld floats of scratch.  Each clip's bits are those of the clip alone.
constexpr int LOGMEL_CLIP_WORDS = 5;
void launch_logmel(const float* x, const int64_t* d_clips, int n_clips, int64_t n_groups, int64_t ld, const float* window, const float* twid,
                   const float* melfb, float* out, float* frame_max, hipStream_t st);
// d_chunks: (C, 3) int32 {first feature column of the clip, its F, window index within the clip}
void launch_audio_im2col1(const float* feat, const int32_t* d_chunks, void* out, int64_t ld, int C, int Hin, int Win, hipStream_t st);
void launch_im2col_nhwc(const void* in, void* out, int B, int Hin, int Win, int Cin, hipStream_t st);
void launch_audio_tokens_gather(const void* in, void* out, int B, int Fq, int T, int Cc, hipStream_t st);
void launch_sinus_pe_add(void* x, int64_t rows, int d, int T, hipStream_t st);
void launch_kv_pack_generic(const void* src, int64_t ld, int k_off, int v_off, KvLayer kv, int N, int nh, int hd, hipStream_t st,
                            const int32_t* slot_of = nullptr);
}  // namespace aha
