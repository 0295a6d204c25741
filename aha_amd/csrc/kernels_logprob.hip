// Per-token log-probabilities (aha_token_logprobs, include/aha_hip.h): for every row of f32 logits x the log-softmax normaliser
// (M = max x, log S = log sum exp(x - M), temperature 1, no penalty), the row's n_top largest logits in (value desc, index asc) order
// with their log-probabilities, and lp(token) = (x[token] - M) - log S of the token the step emits.  Two launches for any number of rows
// (blockIdx.y = row of the table):
//   stage 1  one wave per 512 consecutive logits: its softmax partial (max, sum exp(x - max)) and its n_top best (value, index) pairs.
//            An HBM/L2-bound streaming pass over rows the lm_head has just written; no LDS.
//   stage 2  one workgroup per row: partials -> (M, log S); candidates -> the row's top n_top (16 waves reduce a sixteenth each, wave 0
//            merges the 16 x n_top through LDS); the raw logit of the row's token, and for a row whose token the host picks after the
//            step, the raw logits of its sampling candidates (the ids topk_rows_stage2b_kernel wrote on the same stream).
// The selection is exact: the top n of a union of per-part top-n lists under a total order is the global top n.  The logits are only read.
#include "common.h"
#include "kernels.h"
#include "topk_rounds.h"

namespace aha {
namespace {

constexpr int L1_C = 8;                      // logits per lane in stage 1
constexpr int L1_WAVE_ELEMS = 64 * L1_C;     // 512 logits per wave
constexpr int L1_WAVES_PER_BLOCK = 4;
constexpr int L2_WAVES = 16;                 // stage 2: one workgroup of 16 waves per row
constexpr int L2_C = 12;                     // 16 waves x 64 lanes x 12 stage-1 candidates
constexpr int L2_MERGE_C = (L2_WAVES * LOGPROB_MAX_TOP + 63) / 64;
__host__ __device__ constexpr int logprob_stage1_waves_dev(int V) { return (V + L1_WAVE_ELEMS - 1) / L1_WAVE_ELEMS; }

__global__ __launch_bounds__(64 * L1_WAVES_PER_BLOCK) void logprob_rows_stage1_kernel(const float* logits, int64_t ld, int V,
                                                                                      const int32_t* tab, float* cand_val,
                                                                                      unsigned* cand_idx, float* part_m, float* part_s) {
  const int32_t* t = tab + (size_t)blockIdx.y * LOGPROB_ROW_WORDS;
  const int nw = logprob_stage1_waves_dev(V);
  const int lane = threadIdx.x & 63;
  const int w = blockIdx.x * L1_WAVES_PER_BLOCK + (threadIdx.x >> 6);
  const int base = w * L1_WAVE_ELEMS;
  if (base >= V) return;
  const float* x = logits + (int64_t)t[LOGPROB_ROW_LROW] * ld;
  float v[L1_C];
  unsigned id[L1_C];
#pragma unroll
  for (int j = 0; j < L1_C; ++j) {
    const int i = base + j * 64 + lane;
    const bool ok = i < V;
    v[j] = ok ? x[ok ? i : 0] : -INFINITY;
    id[j] = ok ? (unsigned)i : NO_IDX;
  }
  float lm = -INFINITY;
#pragma unroll
  for (int j = 0; j < L1_C; ++j) lm = fmaxf(lm, v[j]);
  const float wm = wave_max(lm);
  float s = 0.f;
  if (wm > -INFINITY) {   // (a wave of -inf logits only: partial sum 0, not exp(-inf + inf))
#pragma unroll
    for (int j = 0; j < L1_C; ++j)
      if (id[j] != NO_IDX) s += expf(v[j] - wm);
  }
  s = wave_sum(s);
  const size_t pb = (size_t)blockIdx.y * nw;
  if (lane == 0) {
    part_m[pb + w] = wm;
    part_s[pb + w] = s;
  }
  const int n = t[LOGPROB_ROW_NTOP];
  const size_t cb = (size_t)blockIdx.y * nw * LOGPROB_MAX_TOP + (size_t)w * n;   // the row's candidates at pitch n
  wave_topk_rounds<L1_C>(v, id, n, [&](int r, float val, unsigned idx) {
    if (lane == 0) {
      cand_val[cb + r] = val;
      cand_idx[cb + r] = idx;
    }
  });
}

__global__ __launch_bounds__(64 * L2_WAVES) void logprob_rows_stage2_kernel(const float* logits, int64_t ld, int V, const int32_t* tab,
                                                                            const uint32_t* tokens, const float* cand_val,
                                                                            const unsigned* cand_idx, const float* part_m,
                                                                            const float* part_s, const float* sample_out, float* out) {
  __shared__ float s_max[L2_WAVES], s_sum[L2_WAVES];
  __shared__ float s_val[L2_WAVES * LOGPROB_MAX_TOP];
  __shared__ unsigned s_idx[L2_WAVES * LOGPROB_MAX_TOP];
  const int32_t* t = tab + (size_t)blockIdx.y * LOGPROB_ROW_WORDS;
  const int nw = logprob_stage1_waves_dev(V);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n = t[LOGPROB_ROW_NTOP];
  const float* x = logits + (int64_t)t[LOGPROB_ROW_LROW] * ld;
  const float* pm = part_m + (size_t)blockIdx.y * nw;
  const float* psum = part_s + (size_t)blockIdx.y * nw;
  float* o = out + (size_t)blockIdx.y * LOGPROB_OUT_WORDS;

  // (M, log S): every thread ends with the same values, summed in a fixed order
  float m = -INFINITY;
  for (int i = tid; i < nw; i += 64 * L2_WAVES) m = fmaxf(m, pm[i]);
  m = wave_max(m);
  if (lane == 0) s_max[wave] = m;
  __syncthreads();
  float M = s_max[0];
#pragma unroll
  for (int i = 1; i < L2_WAVES; ++i) M = fmaxf(M, s_max[i]);
  float s = 0.f;
  for (int i = tid; i < nw; i += 64 * L2_WAVES) s += psum[i] * expf(pm[i] - M);
  s = wave_sum(s);
  if (lane == 0) s_sum[wave] = s;
  __syncthreads();
  float S = s_sum[0];
#pragma unroll
  for (int i = 1; i < L2_WAVES; ++i) S += s_sum[i];
  const float logS = logf(S);

  if (n > 0) {   // (n is uniform over the workgroup)
    const float* cv = cand_val + (size_t)blockIdx.y * nw * LOGPROB_MAX_TOP;
    const unsigned* ci = cand_idx + (size_t)blockIdx.y * nw * LOGPROB_MAX_TOP;
    const int n_cand = nw * n;
    const int chunk = (n_cand + L2_WAVES - 1) / L2_WAVES;
    const int c0 = wave * chunk, c1 = min(c0 + chunk, n_cand);
    {
      float v[L2_C];
      unsigned id[L2_C];
#pragma unroll
      for (int j = 0; j < L2_C; ++j) {
        const int i = c0 + j * 64 + lane;
        const bool ok = i < c1;
        v[j] = ok ? cv[ok ? i : 0] : -INFINITY;
        id[j] = ok ? ci[ok ? i : 0] : NO_IDX;
        if (id[j] == NO_IDX) v[j] = -INFINITY;
      }
      wave_topk_rounds<L2_C>(v, id, n, [&](int r, float val, unsigned idx) {
        if (lane == 0) {
          s_val[wave * n + r] = val;
          s_idx[wave * n + r] = idx;
        }
      });
    }
    __syncthreads();
    if (wave == 0) {
      float v[L2_MERGE_C];
      unsigned id[L2_MERGE_C];
#pragma unroll
      for (int j = 0; j < L2_MERGE_C; ++j) {
        const int i = j * 64 + lane;
        const bool ok = i < L2_WAVES * n;
        v[j] = ok ? s_val[ok ? i : 0] : -INFINITY;
        id[j] = ok ? s_idx[ok ? i : 0] : NO_IDX;
        if (id[j] == NO_IDX) v[j] = -INFINITY;
      }
      wave_topk_rounds<L2_MERGE_C>(v, id, n, [&](int r, float val, unsigned idx) {
        if (lane == 0) {
          reinterpret_cast<unsigned*>(o)[LOGPROB_OUT_IDS + r] = idx;
          o[LOGPROB_OUT_LPS + r] = idx == NO_IDX ? -INFINITY : (val - M) - logS;
        }
      });
    }
  }
  if (wave == 0 && lane >= n && lane < LOGPROB_MAX_TOP) {   // entries past n_top: no token
    reinterpret_cast<unsigned*>(o)[LOGPROB_OUT_IDS + lane] = NO_IDX;
    o[LOGPROB_OUT_LPS + lane] = -INFINITY;
  }
  if (wave == 1) {
    if (lane == 0) {
      const uint32_t tok = tokens[t[LOGPROB_ROW_TOK]];
      o[LOGPROB_OUT_LP] = tok < (uint32_t)V ? (x[tok] - M) - logS : __uint_as_float(0x7fc00000u);
      reinterpret_cast<int32_t*>(o)[LOGPROB_OUT_NTOP] = n;
      o[LOGPROB_OUT_M] = M;
      o[LOGPROB_OUT_LOGS] = logS;
    }
    // a row the host samples: the raw logits of its candidates, so that lp of whichever it picks needs no second trip
    const int slot = t[LOGPROB_ROW_CSLOT];
    if (slot >= 0) {
      const unsigned idx = reinterpret_cast<const unsigned*>(sample_out + (size_t)slot * SAMPLE_OUT_WORDS + 66)[lane];
      o[LOGPROB_OUT_RAW + lane] = idx < (unsigned)V ? x[idx] : __uint_as_float(0x7fc00000u);
    }
  }
}

}  // namespace

int logprob_stage1_waves(int V) { return logprob_stage1_waves_dev(V); }
// the stage-1 candidates of a row within what stage 2 holds in registers (16 waves x 64 lanes x 12)
bool logprob_shape_ok(int V) { return V > 0 && (int64_t)logprob_stage1_waves(V) * LOGPROB_MAX_TOP <= L2_WAVES * 64 * L2_C; }

void launch_logprob_rows(const float* logits, int64_t ld, int V, int rows, const int32_t* tab, const uint32_t* tokens, float* cand_val,
                         unsigned* cand_idx, float* part_m, float* part_s, const float* sample_out, float* out, int stage, hipStream_t st) {
  if (rows <= 0) return;
  const int nw = logprob_stage1_waves(V);
  if (stage == 0)
    hipLaunchKernelGGL(logprob_rows_stage1_kernel, dim3((nw + L1_WAVES_PER_BLOCK - 1) / L1_WAVES_PER_BLOCK, rows),
                       dim3(64 * L1_WAVES_PER_BLOCK), 0, st, logits, ld, V, tab, cand_val, cand_idx, part_m, part_s);
  else
    hipLaunchKernelGGL(logprob_rows_stage2_kernel, dim3(1, rows), dim3(64 * L2_WAVES), 0, st, logits, ld, V, tab, tokens, cand_val, cand_idx,
                       part_m, part_s, sample_out, out);
}

}  // namespace aha
