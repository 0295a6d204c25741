// D11 on the device: the deterministic half of `sample_and_push` (reference src/models/common/generate.rs:70-86) --
// repeat penalty (src/models/common/sample.rs:41-60 -> candle_transformers::utils::apply_repeat_penalty) and the candidate
// set of candle's LogitsProcessor (Sampling::TopK / TopKThenTopP / TopP, sample.rs:7-38): the k largest penalised logits
// with their vocabulary indices, plus the max and the sum of exp((x - max) / T) over the WHOLE vocabulary, so that the host
// gets the same probabilities candle's full-vocabulary softmax would give those k tokens.  The random draw stays on the host
// (the caller's RNG): 8k + 8 bytes cross PCIe per token instead of the 608 KB logits vector.
//
// HBM-bound integer/compare work: one pass over V f32 logits (608 KB), no LDS staging needed.  Selection is k rounds of
// (wave max, lowest index among the maxima) over register-resident candidates: exact, ordered by (value desc, index asc).
#include "common.h"
#include "kernels.h"
#include "topk_rounds.h"

namespace aha {
namespace {

// work[t] = penalised logit of every context token t (reads the untouched logits, so duplicates in ctx write the same value:
// the reference applies the penalty once per distinct id through a HashSet).
__global__ void repeat_penalty_kernel(const float* logits, float* work, const uint32_t* ctx, int n, float penalty, int V) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint32_t t = ctx[i];
  if (t >= (uint32_t)V) return;  // `logits.get_mut(token_id)` is None: ignored
  const float x = logits[t];
  work[t] = x >= 0.f ? x / penalty : x * penalty;
}

constexpr int S1_C = 8;                      // elements per lane in stage 1
constexpr int S1_WAVE_ELEMS = 64 * S1_C;     // 512 logits per wave
constexpr int S1_WAVES_PER_BLOCK = 4;
__host__ __device__ constexpr int sample_stage1_waves_dev(int V) { return (V + S1_WAVE_ELEMS - 1) / S1_WAVE_ELEMS; }

// stage 1: every wave reduces 512 consecutive logits to its k best and its softmax partial (max, sum exp((x - max) * inv_temp)).
// PEN: the row's repeat penalty is applied as the logits are loaded -- ctx[0 .. n_ctx) are DISTINCT in-vocabulary ids (the host
// dedups them: apply_repeat_penalty's HashSet), so each hit is penalised once, from the untouched value, exactly as
// repeat_penalty_kernel writes work[t].  The logits buffer itself is never written.
// ADJ: after the penalty, adj_val[i] is added (one f32 add) to the logit of adj_id[i], i < n_adj -- ids sorted ascending and distinct.
// The wave finds the first entry inside its 512 logits by a wave-uniform binary search and walks on from there until an id leaves them:
// it reads at most ceil(log2 n_adj) + hits + 1 ids (the search's last upper probe is kept, so the walk's first id is not read again)
// and `hits` values.  A wave left with nothing but -inf contributes (max -inf, sum 0): exp(-inf - -inf) would be NaN.
// MASK: after the addends, every logit whose bit in the row's allowed-token mask is clear becomes -inf.  The wave's 512 logits are the 16
// consecutive words mask[16 w ..), of which lanes 0 .. 15 load one each (words at or past ceil(V / 32) are not read); element j of lane l
// takes bit l & 31 of word 2 j + (l >> 5) through two wave-uniform lane reads.  Bits at positions >= V belong to elements that are -inf anyway.
template <bool PEN, bool ADJ = false, bool MASK = false>
__device__ __forceinline__ void topk_stage1_body(const float* x, int V, int k, float inv_temp, const uint32_t* ctx, int n_ctx,
                                                 float penalty, int w, float* cand_val, unsigned* cand_idx, float* part_m, float* part_s,
                                                 const uint32_t* adj_id = nullptr, const float* adj_val = nullptr, int n_adj = 0,
                                                 const uint32_t* mask = nullptr) {
  const int lane = threadIdx.x & 63;
  if (ADJ || MASK) w = __builtin_amdgcn_readfirstlane(w);   // the search and the walk below run on scalars
  const int base = w * S1_WAVE_ELEMS;
  if (base >= V) return;
  float v[S1_C];
  unsigned id[S1_C];
#pragma unroll
  for (int j = 0; j < S1_C; ++j) {
    const int i = base + j * 64 + lane;
    const bool ok = i < V;
    v[j] = ok ? x[ok ? i : 0] : -INFINITY;
    id[j] = ok ? (unsigned)i : NO_IDX;
  }
  if (PEN) {
    for (int c = 0; c < n_ctx; ++c) {        // wave-uniform walk; only ids inside this wave's 512 logits touch registers
      const unsigned t = ctx[c];
      if (t - (unsigned)base >= (unsigned)S1_WAVE_ELEMS) continue;
#pragma unroll
      for (int j = 0; j < S1_C; ++j)
        if (id[j] == t) v[j] = v[j] >= 0.f ? v[j] / penalty : v[j] * penalty;
    }
  }
  if (ADJ) {
    int lo = 0, hi = n_adj;
    unsigned t = NO_IDX;                     // adj_id[hi] once hi < n_adj
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      const unsigned u = adj_id[mid];
      if (u < (unsigned)base) lo = mid + 1;
      else hi = mid, t = u;
    }
    for (int c = lo; c < n_adj; ++c) {
      if (c != lo) t = adj_id[c];
      if (t - (unsigned)base >= (unsigned)S1_WAVE_ELEMS) break;
      const float a = adj_val[c];
#pragma unroll
      for (int j = 0; j < S1_C; ++j)
        if (id[j] == t) v[j] = v[j] + a;
    }
  }
  if (MASK) {
    const int n_words = (V + 31) >> 5, wi = w * (S1_WAVE_ELEMS / 32) + lane;
    const bool ok = lane < S1_WAVE_ELEMS / 32 && wi < n_words;
    const unsigned word = ok ? mask[ok ? wi : 0] : 0u;
#pragma unroll
    for (int j = 0; j < S1_C; ++j) {
      const unsigned lo = __builtin_amdgcn_readlane(word, 2 * j), hi = __builtin_amdgcn_readlane(word, 2 * j + 1);
      if (!(((lane < 32 ? lo : hi) >> (lane & 31)) & 1u)) v[j] = -INFINITY;
    }
  }
  float lm = -INFINITY;
#pragma unroll
  for (int j = 0; j < S1_C; ++j) lm = fmaxf(lm, v[j]);
  const float wm = wave_max(lm);
  float s = 0.f;
  if (!(ADJ || MASK) || wm != -INFINITY) {
#pragma unroll
    for (int j = 0; j < S1_C; ++j)
      if (id[j] != NO_IDX) s += __expf((v[j] - wm) * inv_temp);
  }
  s = wave_sum(s);
  if (lane == 0) {
    part_m[w] = wm;
    part_s[w] = s;
  }
  wave_topk_rounds<S1_C>(v, id, k, [&](int r, float val, unsigned idx) {
    if (lane == 0) {
      cand_val[(size_t)w * k + r] = val;
      cand_idx[(size_t)w * k + r] = idx;
    }
  });
}

__global__ __launch_bounds__(64 * S1_WAVES_PER_BLOCK) void topk_stage1_kernel(const float* x, int V, int k, float inv_temp,
                                                                              float* cand_val, unsigned* cand_idx,
                                                                              float* part_m, float* part_s) {
  topk_stage1_body<false>(x, V, k, inv_temp, nullptr, 0, 1.f, blockIdx.x * S1_WAVES_PER_BLOCK + (threadIdx.x >> 6), cand_val, cand_idx,
                          part_m, part_s);
}

constexpr int S2_WAVES = 16;
constexpr int S2_C = 20;  // 16 waves x 64 lanes x 20 >= 297 stage-1 waves x 64 candidates

// stage 2a (16 one-wave blocks, one per CU -- the rounds are VALU-bound, so the waves must not share a SIMD): each wave
// reduces a contiguous sixteenth of the stage-1 candidates to its k best
__device__ __forceinline__ void topk_stage2a_body(const float* cand_val, const unsigned* cand_idx, int n_cand, int k, int wave,
                                                  float* mid_val, unsigned* mid_idx) {
  const int lane = threadIdx.x;
  const int chunk = (n_cand + S2_WAVES - 1) / S2_WAVES;
  const int c0 = wave * chunk, c1 = min(c0 + chunk, n_cand);
  float v[S2_C];
  unsigned id[S2_C];
#pragma unroll
  for (int j = 0; j < S2_C; ++j) {
    const int i = c0 + j * 64 + lane;
    const bool ok = i < c1;
    v[j] = ok ? cand_val[ok ? i : 0] : -INFINITY;
    id[j] = ok ? cand_idx[ok ? i : 0] : NO_IDX;
    if (id[j] == NO_IDX) v[j] = -INFINITY;
  }
  wave_topk_rounds<S2_C>(v, id, k, [&](int r, float val, unsigned idx) {
    if (lane == 0) {
      mid_val[wave * k + r] = val;
      mid_idx[wave * k + r] = idx;
    }
  });
}

__global__ __launch_bounds__(64) void topk_stage2a_kernel(const float* cand_val, const unsigned* cand_idx, int n_cand, int k,
                                                          float* mid_val, unsigned* mid_idx) {
  topk_stage2a_body(cand_val, cand_idx, n_cand, k, blockIdx.x, mid_val, mid_idx);
}

// stage 2b (one wave): 16 x k -> k in (value desc, index asc) order, and the softmax partials -> (max, sumexp)
__device__ __forceinline__ void topk_stage2b_body(const float* mid_val, const unsigned* mid_idx, const float* part_m, const float* part_s,
                                                  int n_part, int k, float inv_temp, float* out_val, unsigned* out_idx, float* out_ms) {
  const int lane = threadIdx.x;
  {
    float m = -INFINITY;
    for (int i = lane; i < n_part; i += 64) m = fmaxf(m, part_m[i]);
    const float M = wave_max(m);
    float s = 0.f;
    for (int i = lane; i < n_part; i += 64) s += part_s[i] * __expf((part_m[i] - M) * inv_temp);
    s = wave_sum(s);
    if (lane == 0) {
      out_ms[0] = M;
      out_ms[1] = s;
    }
  }
  float v[S2_WAVES];
  unsigned id[S2_WAVES];
#pragma unroll
  for (int j = 0; j < S2_WAVES; ++j) {
    const int i = j * 64 + lane;
    const bool ok = i < S2_WAVES * k;
    v[j] = ok ? mid_val[ok ? i : 0] : -INFINITY;
    id[j] = ok ? mid_idx[ok ? i : 0] : NO_IDX;
    if (id[j] == NO_IDX) v[j] = -INFINITY;
  }
  wave_topk_rounds<S2_WAVES>(v, id, k, [&](int r, float val, unsigned idx) {
    if (lane == 0) {
      out_val[r] = val;
      out_idx[r] = idx;
    }
  });
}

__global__ __launch_bounds__(64) void topk_stage2b_kernel(const float* mid_val, const unsigned* mid_idx, const float* part_m,
                                                          const float* part_s, int n_part, int k, float inv_temp,
                                                          float* out_val, unsigned* out_idx, float* out_ms) {
  topk_stage2b_body(mid_val, mid_idx, part_m, part_s, n_part, k, inv_temp, out_val, out_idx, out_ms);
}

// ---- the same three stages for R rows at once (batched sampled generation): blockIdx.y is the row of the sample table ----------
// Row s of the table (SAMPLE_ROW_WORDS int32): logits row, k, 1/T and penalty (f32 bits), its distinct context ids ctx[c0 .. c0 + n),
// its addends adj_id / adj_val [a0 .. a0 + n_adj) (sorted by id, distinct; a row without any takes the instantiation it always took),
// its allowed-token mask masks[SAMPLE_ROW_MASK * ceil(V / 32) ..) (SAMPLE_ROW_MASK < 0: none, and the instantiation it took without masks;
// a masked row takes one more, which also walks its possibly empty context and addend list).
// Row s owns cand_* [s * (nw + 16) * 64, +(nw + 16) * 64) (stage-1 candidates, then the 16 x k intermediates), part_* [s * nw, +nw) and
// out [s * SAMPLE_OUT_WORDS, +SAMPLE_OUT_WORDS) = {vals[64], max, sumexp, idx[64]}.  Every stage runs the single-row body on the row's
// own slices, so a row's outputs are those of the single-row pipeline (the penalty copy there, the load-time penalty here, give the
// same f32 values).
__global__ __launch_bounds__(64 * S1_WAVES_PER_BLOCK) void topk_rows_stage1_kernel(const float* logits, int64_t ld, int V,
                                                                                   const int32_t* tab, const uint32_t* ctx,
                                                                                   const uint32_t* adj_id, const float* adj_val,
                                                                                   const uint32_t* masks, float* cand_val, unsigned* cand_idx,
                                                                                   float* part_m, float* part_s) {
  const int32_t* t = tab + (size_t)blockIdx.y * SAMPLE_ROW_WORDS;
  const int nw = sample_stage1_waves_dev(V);
  const size_t cb = (size_t)blockIdx.y * (nw + S2_WAVES) * 64, pb = (size_t)blockIdx.y * nw;
  const float* x = logits + (int64_t)t[SAMPLE_ROW_LROW] * ld;
  const int w = blockIdx.x * S1_WAVES_PER_BLOCK + (threadIdx.x >> 6);
  const int n_ctx = t[SAMPLE_ROW_NCTX], n_adj = t[SAMPLE_ROW_NADJ], mrow = t[SAMPLE_ROW_MASK];
  if (mrow >= 0)
    topk_stage1_body<true, true, true>(x, V, t[SAMPLE_ROW_K], __int_as_float(t[SAMPLE_ROW_INVT]), ctx + t[SAMPLE_ROW_CTX0], n_ctx,
                                       __int_as_float(t[SAMPLE_ROW_PEN]), w, cand_val + cb, cand_idx + cb, part_m + pb, part_s + pb,
                                       adj_id + t[SAMPLE_ROW_ADJ0], adj_val + t[SAMPLE_ROW_ADJ0], n_adj,
                                       masks + (size_t)mrow * ((V + 31) >> 5));
  else if (n_adj > 0)
    topk_stage1_body<true, true>(x, V, t[SAMPLE_ROW_K], __int_as_float(t[SAMPLE_ROW_INVT]), ctx + t[SAMPLE_ROW_CTX0], n_ctx,
                                 __int_as_float(t[SAMPLE_ROW_PEN]), w, cand_val + cb, cand_idx + cb, part_m + pb, part_s + pb,
                                 adj_id + t[SAMPLE_ROW_ADJ0], adj_val + t[SAMPLE_ROW_ADJ0], n_adj);
  else if (n_ctx > 0)
    topk_stage1_body<true>(x, V, t[SAMPLE_ROW_K], __int_as_float(t[SAMPLE_ROW_INVT]), ctx + t[SAMPLE_ROW_CTX0], n_ctx,
                           __int_as_float(t[SAMPLE_ROW_PEN]), w, cand_val + cb, cand_idx + cb, part_m + pb, part_s + pb);
  else
    topk_stage1_body<false>(x, V, t[SAMPLE_ROW_K], __int_as_float(t[SAMPLE_ROW_INVT]), nullptr, 0, 1.f, w, cand_val + cb, cand_idx + cb,
                            part_m + pb, part_s + pb);
}

__global__ __launch_bounds__(64) void topk_rows_stage2a_kernel(int V, const int32_t* tab, float* cand_val, unsigned* cand_idx) {
  const int32_t* t = tab + (size_t)blockIdx.y * SAMPLE_ROW_WORDS;
  const int nw = sample_stage1_waves_dev(V), k = t[SAMPLE_ROW_K];
  const size_t cb = (size_t)blockIdx.y * (nw + S2_WAVES) * 64;
  float* cv = cand_val + cb;   // the row's 16 x k intermediates sit behind its stage-1 candidates
  unsigned* ci = cand_idx + cb;
  topk_stage2a_body(cv, ci, nw * k, k, blockIdx.x, cv + (size_t)nw * 64, ci + (size_t)nw * 64);
}

__global__ __launch_bounds__(64) void topk_rows_stage2b_kernel(int V, const int32_t* tab, const float* cand_val, const unsigned* cand_idx,
                                                               const float* part_m, const float* part_s, float* out) {
  const int32_t* t = tab + (size_t)blockIdx.y * SAMPLE_ROW_WORDS;
  const int nw = sample_stage1_waves_dev(V), k = t[SAMPLE_ROW_K];
  const size_t cb = (size_t)blockIdx.y * (nw + S2_WAVES) * 64 + (size_t)nw * 64, pb = (size_t)blockIdx.y * nw;
  float* o = out + (size_t)blockIdx.y * SAMPLE_OUT_WORDS;
  topk_stage2b_body(cand_val + cb, cand_idx + cb, part_m + pb, part_s + pb, nw, k, __int_as_float(t[SAMPLE_ROW_INVT]), o,
                    reinterpret_cast<unsigned*>(o + 66), o + 64);
}

}  // namespace

int sample_stage1_waves(int V) { return sample_stage1_waves_dev(V); }
// k <= 64 and the stage-1 candidates within what stage 2a holds in registers (16 waves x 64 lanes x 20)
bool sample_shape_ok(int V, int k) { return V > 0 && k >= 1 && k <= 64 && (int64_t)sample_stage1_waves(V) * k <= S2_WAVES * 64 * S2_C; }

void launch_repeat_penalty(const float* logits, float* work, const uint32_t* ctx, int n, float penalty, int V, hipStream_t st) {
  if (n <= 0) return;
  hipLaunchKernelGGL(repeat_penalty_kernel, dim3((n + 255) / 256), dim3(256), 0, st, logits, work, ctx, n, penalty, V);
}

void launch_topk_candidates(const float* x, int V, int k, float inv_temp, float* cand_val, unsigned* cand_idx, float* part_m,
                            float* part_s, float* out_val, unsigned* out_idx, float* out_ms, hipStream_t st) {
  const int nw = sample_stage1_waves(V);
  hipLaunchKernelGGL(topk_stage1_kernel, dim3((nw + S1_WAVES_PER_BLOCK - 1) / S1_WAVES_PER_BLOCK), dim3(64 * S1_WAVES_PER_BLOCK), 0,
                     st, x, V, k, inv_temp, cand_val, cand_idx, part_m, part_s);
  // the 16 x k intermediates live right behind the stage-1 candidates (model.hip sizes cand_* as (nw + 16) * 64)
  float* mid_val = cand_val + (size_t)nw * 64;
  unsigned* mid_idx = cand_idx + (size_t)nw * 64;
  hipLaunchKernelGGL(topk_stage2a_kernel, dim3(S2_WAVES), dim3(64), 0, st, cand_val, cand_idx, nw * k, k, mid_val, mid_idx);
  hipLaunchKernelGGL(topk_stage2b_kernel, dim3(1), dim3(64), 0, st, mid_val, mid_idx, part_m, part_s, nw, k, inv_temp, out_val,
                     out_idx, out_ms);
}

void launch_topk_rows(const float* logits, int64_t ld, int V, int rows, const int32_t* tab, const uint32_t* ctx, float* cand_val,
                      unsigned* cand_idx, float* part_m, float* part_s, float* out, int stage, hipStream_t st, const uint32_t* adj_id,
                      const float* adj_val, const uint32_t* masks) {
  if (rows <= 0) return;
  const int nw = sample_stage1_waves(V);
  if (stage == 0)
    hipLaunchKernelGGL(topk_rows_stage1_kernel, dim3((nw + S1_WAVES_PER_BLOCK - 1) / S1_WAVES_PER_BLOCK, rows), dim3(64 * S1_WAVES_PER_BLOCK),
                       0, st, logits, ld, V, tab, ctx, adj_id, adj_val, masks, cand_val, cand_idx, part_m, part_s);
  else if (stage == 1)
    hipLaunchKernelGGL(topk_rows_stage2a_kernel, dim3(S2_WAVES, rows), dim3(64), 0, st, V, tab, cand_val, cand_idx);
  else
    hipLaunchKernelGGL(topk_rows_stage2b_kernel, dim3(1, rows), dim3(64), 0, st, V, tab, cand_val, cand_idx, part_m, part_s, out);
}

}  // namespace aha
