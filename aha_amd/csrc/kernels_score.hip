// Log-probabilities of GIVEN tokens (aha_token_score, include/aha_hip.h): the lm_head GEMM whose epilogue reduces each row's V logits to
// five numbers on chip.  No logit reaches global memory.
//
//   x[r, i] = bf16(sum_k h[r, k] W[i, k])  (f32 accumulate, read back as f32: the "bf16 Linear output" GEMV_LOGITS and the prefill head produce)
//   M = max_i x,  S = sum_i exp(x_i - M),  logprob = (x_t - M) - log S,  top_id = first i with x_i = M,  top_logprob = -log S
//
// score_rows_kernel: grid = row blocks x vocabulary slices (plan_score_rows).  A workgroup of eight waves (2 x 4, 64 rows x 32 columns each)
// owns 128 rows of h and a contiguous run of 128-column tiles of W and walks them in one persistent loop:
//   * Main loop: the ring of the 128^2 GEMM (kernels_gemm.hip gemm_glds_ring_kernel): four LDS stages of [h tile 16 KiB | W tile 16 KiB] in the
//     XOR-swizzled 8-row pieces LDS-DMA writes, v_mfma_f32_16x16x32_bf16 on fragments read half a K tile ahead, one counted vmcnt wait and one
//     raw barrier per K step.  Here the ring runs over the FLAT sequence of (column tile, K tile) pairs: while the last K tiles of a column
//     tile are multiplied the first ones of the next are already being staged (the staging cursor runs three K tiles ahead of the MFMAs across
//     tile boundaries), so the pipeline is filled once per workgroup, not once per tile.  The h row block is re-staged from L2 for every tile.
//   * Epilogue, in registers: MFMA is issued W fragment x h fragment, so a lane holds, per 16-row fragment mi, 8 logits of ONE row (row
//     mi * 16 + (lane & 15), columns ni * 16 + (lane >> 4) * 4 + 0..3).  Each lane keeps a running (m, s, best value, best index, x_t) for its
//     four rows across all column tiles of the slice -- 20 registers -- and folds a tile in with no cross-lane traffic: round to bf16 and
//     widen, mask columns >= V to -inf, tile maximum, s = s exp(m - m') + sum exp(x - m') (v_exp_f32), first index of a new maximum, and the
//     target's logit from the same rounded value when its column is the lane's.  A lane visits its columns in ascending order, so "first
//     index" is a strict comparison.
//   * End of slice, once: the four lanes of a row (lane ^ 16, lane ^ 32) merge with v_permlane32_swap / v_permlane16_swap, the four column
//     waves of a row through 10 KiB of the (drained) LDS ring, in a fixed order, and the workgroup writes one five-word partial per row.
// score_rows_merge_kernel: one thread per row merges the row's partials in slice order and writes its aha_token_score.
// Every merge is the same function of the same operands in the same order on every run: no atomics, the same bits every time.
#include <math.h>

#include <mutex>

#include "common.h"
#include "gemm256_body.h"
#include "kernels.h"

namespace aha {
namespace {

constexpr int SC_BM = 128, SC_BN = 128;            // rows of a row block, columns of a column tile
constexpr int SC_WN = 4, SC_NW = 8, SC_NI = 2;     // column waves, waves, 16-column fragments per wave
constexpr int SC_NST = 4;                          // LDS stages
constexpr int SC_STAGE = 2 * TILE_BYTES;           // [h tile | W tile]
constexpr int SC_LDS = SC_NST * SC_STAGE;          // 128 KiB: one workgroup per CU
constexpr int SC_LPT = 4;                          // LDS-DMA loads per wave and K tile (two 8-row pieces of h, two of W)
constexpr int SC_WORDS = 5;                        // a partial: m, s, best value, best index, x_t
constexpr int SC_CUS = 256;                        // MI355X

struct ScoreArgs {
  const bf16_t* h;
  int64_t ldh;
  const bf16_t* W;
  const int32_t* targets;
  float* part;   // (R, n_slices, SC_WORDS)
  int R, V, K;
  int n_rb, n_slices, tiles_per_slice;
};

struct ScoreState {
  float m, s, bv;
  uint32_t bi;
  float xt;
};

__device__ __forceinline__ float exp_diff(float d) { return __builtin_amdgcn_exp2f(d * 1.4426950408889634f); }   // exp(d), d <= 0; exactly 1 at 0

// the state of the union of two column sets (a's and b's operands in this order)
__device__ __forceinline__ ScoreState score_merge(const ScoreState& a, const ScoreState& b) {
  ScoreState r;
  r.m = fmaxf(a.m, b.m);
  const float ms = r.m == -INFINITY ? 0.f : r.m;   // (two empty sets: no -inf - -inf)
  r.s = a.s * exp_diff(a.m - ms) + b.s * exp_diff(b.m - ms);
  const bool ta = a.bv > b.bv || (a.bv == b.bv && a.bi <= b.bi);   // value descending, index ascending
  r.bv = ta ? a.bv : b.bv;
  r.bi = ta ? a.bi : b.bi;
  r.xt = fmaxf(a.xt, b.xt);   // -inf wherever the target's column is not
  return r;
}

// Both lanes of a pair see (value of the lower lane, value of the upper lane): the same operands in the same order, the same result.
template <bool SWAP32>
__device__ __forceinline__ ScoreState score_merge_lanes(const ScoreState& v) {
  auto sw = [](uint32_t u, uint32_t& lo, uint32_t& hi) __attribute__((always_inline)) {
    const auto r = SWAP32 ? __builtin_amdgcn_permlane32_swap(u, u, false, false) : __builtin_amdgcn_permlane16_swap(u, u, false, false);
    lo = r[0], hi = r[1];
  };
  uint32_t lo[SC_WORDS], hi[SC_WORDS];
  sw(__float_as_uint(v.m), lo[0], hi[0]);
  sw(__float_as_uint(v.s), lo[1], hi[1]);
  sw(__float_as_uint(v.bv), lo[2], hi[2]);
  sw(v.bi, lo[3], hi[3]);
  sw(__float_as_uint(v.xt), lo[4], hi[4]);
  const ScoreState a = {__uint_as_float(lo[0]), __uint_as_float(lo[1]), __uint_as_float(lo[2]), lo[3], __uint_as_float(lo[4])};
  const ScoreState b = {__uint_as_float(hi[0]), __uint_as_float(hi[1]), __uint_as_float(hi[2]), hi[3], __uint_as_float(hi[4])};
  return score_merge(a, b);
}

// One column tile's accumulators into the lane's four row states.  col0: the lane's first column of the tile (tile + wave + lane group);
// MASK: the tile reaches past V.
template <bool MASK>
__device__ __forceinline__ void score_fold(const f32x4_t (&acc)[SC_NI][4], ScoreState (&stt)[4], const int (&tgt)[4], int col0, int V) {
#pragma unroll
  for (int mi = 0; mi < 4; ++mi) {
    float x[SC_NI * 4];
    ScoreState& q = stt[mi];
#pragma unroll
    for (int ni = 0; ni < SC_NI; ++ni)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int col = col0 + ni * 16 + j;
        float v = rbf(acc[ni][mi][j]);   // Linear output -> bf16, read as f32
        if (MASK && col >= V) v = -INFINITY;
        if (col == tgt[mi]) q.xt = v;    // (targets are < V)
        x[ni * 4 + j] = v;
      }
    float tmax = x[0];
#pragma unroll
    for (int e = 1; e < SC_NI * 4; ++e) tmax = fmaxf(tmax, x[e]);
    // a new maximum: its first column among the lane's eight (ascending in e); selects, not branches
    const bool up = tmax > q.bv;
    uint32_t first = q.bi;
#pragma unroll
    for (int e = SC_NI * 4 - 1; e >= 0; --e) first = (up && x[e] == tmax) ? (uint32_t)(col0 + (e >> 2) * 16 + (e & 3)) : first;
    q.bi = first;
    q.bv = up ? tmax : q.bv;
    const float mn = fmaxf(q.m, tmax), ms = mn == -INFINITY ? 0.f : mn;
    float s = q.s * exp_diff(q.m - ms);
#pragma unroll
    for (int e = 0; e < SC_NI * 4; ++e) s += exp_diff(x[e] - ms);
    q.s = s;
    q.m = mn;
  }
}

__global__ __launch_bounds__(SC_NW * 64) __attribute__((amdgpu_waves_per_eu(2))) void score_rows_kernel(ScoreArgs a) {
  char* const smem = gemm_smem;   // SC_NST x [h tile | W tile]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, G = lane >> 4, c = lane & 15;
  const int wm = wave / SC_WN, wn = wave % SC_WN;
  const int rb = (int)blockIdx.x % a.n_rb, slice = (int)blockIdx.x / a.n_rb;   // the row blocks of a slice run side by side: they share its W tiles in L2
  const int m0 = rb * SC_BM;
  const int ntn = (a.V + SC_BN - 1) / SC_BN;
  const int t0 = slice * a.tiles_per_slice, t1 = min(ntn, t0 + a.tiles_per_slice);   // t0 < t1 by the plan
  const int nk = a.K / BK;

  int tgt[4];
#pragma unroll
  for (int mi = 0; mi < 4; ++mi) {
    const int row = m0 + wm * 64 + mi * 16 + c;
    tgt[mi] = row < a.R ? a.targets[row] : -1;
  }
  // staging: piece j of a tile = image rows (j * 8 + wave) * 8 .. + 8; lane L lands on row + (L >> 3), physical slot L & 7, and fetches the
  // logical k slot (L & 7) ^ ((row >> 1) & 7).  Rows past R / V re-read the last valid row (their results are masked or never written).
  const bf16_t* ga[2];
  const bf16_t* gw[2];
  int prow[2], pk[2];
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    prow[j] = (j * SC_NW + wave) * 8 + (lane >> 3);
    pk[j] = ((lane & 7) ^ ((prow[j] >> 1) & 7)) * 8;
    ga[j] = a.h + (int64_t)min(m0 + prow[j], a.R - 1) * a.ldh + pk[j];
  }
  auto set_w = [&](int t) __attribute__((always_inline)) {
#pragma unroll
    for (int j = 0; j < 2; ++j) gw[j] = a.W + (int64_t)min(t * SC_BN + prow[j], a.V - 1) * a.K + pk[j];
  };
  // the staging cursor: (column tile, K tile) of the next stage to request; past the slice's end it stays on the last pair (valid memory,
  // a stage nobody reads) so that every K step requests SC_LPT pieces and the counted waits stay uniform
  int s_t = t0, s_kt = 0;
  set_w(s_t);
  auto stage_piece = [&](int st_, int j) __attribute__((always_inline)) {
    char* sa = smem + st_ * SC_STAGE;
    char* sw = sa + TILE_BYTES;
    __builtin_amdgcn_global_load_lds((glb_ptr_t)(ga[j] + s_kt * BK), (lds_ptr_t)(sa + (j * SC_NW + wave) * 1024), 16, 0, 0);
    __builtin_amdgcn_global_load_lds((glb_ptr_t)(gw[j] + s_kt * BK), (lds_ptr_t)(sw + (j * SC_NW + wave) * 1024), 16, 0, 0);
  };
  auto advance = [&]() __attribute__((always_inline)) {
    if (++s_kt == nk) {
      if (s_t + 1 < t1) {
        s_kt = 0;
        set_w(++s_t);
      } else {
        s_kt = nk - 1;
      }
    }
  };
  auto read_frags = [&](int st_, int ks, bf16x8_t (&af)[4], bf16x8_t (&wf)[SC_NI]) __attribute__((always_inline)) {
    const char* sa = smem + st_ * SC_STAGE;
    const char* sw = sa + TILE_BYTES;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      af[i] = as_frag(*reinterpret_cast<const u32x4_t*>(sa + swz(wm * 64 + i * 16 + c, ks * 4 + G)));
      if (i < SC_NI) wf[i] = as_frag(*reinterpret_cast<const u32x4_t*>(sw + swz(wn * (SC_NI * 16) + i * 16 + c, ks * 4 + G)));
    }
  };
#define AHA_SCORE_BAR()                          \
  do {                                           \
    __builtin_amdgcn_sched_barrier(0);           \
    __builtin_amdgcn_s_barrier();                \
    __builtin_amdgcn_sched_barrier(0);           \
  } while (0)
  // the targets arrive before the first LDS-DMA request: nothing but ring pieces is in the vmcnt queue of the loop
#pragma unroll
  for (int mi = 0; mi < 4; ++mi) asm volatile("" : "+v"(tgt[mi]));
  __builtin_amdgcn_sched_barrier(0);
#pragma unroll
  for (int t = 0; t < SC_NST - 1; ++t) {
    stage_piece(t, 0);
    stage_piece(t, 1);
    advance();
  }
  ScoreState stt[4];
#pragma unroll
  for (int mi = 0; mi < 4; ++mi) stt[mi] = ScoreState{-INFINITY, 0.f, -INFINITY, 0xFFFFFFFFu, -INFINITY};

  bf16x8_t a0[4], w0[SC_NI], a1[4], w1[SC_NI];
  {
    constexpr int KEEP0 = SC_LPT * (SC_NST - 2);   // the first K tile has landed
    __builtin_amdgcn_s_waitcnt(0x0F70 | (KEEP0 & 15) | ((KEEP0 >> 4) << 14));
    AHA_SCORE_BAR();
    read_frags(0, 0, a0, w0);
  }
  int st = 0, st_new = SC_NST - 1;
  for (int t = t0; t < t1; ++t) {
    f32x4_t acc[SC_NI][4];   // [ni][mi]
#pragma unroll
    for (int i = 0; i < SC_NI; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[i][j] = f32x4_t{0.f, 0.f, 0.f, 0.f};
    for (int kt = 0; kt < nk; ++kt) {
      const int st_next = (st + 1 == SC_NST) ? 0 : st + 1;
      // k 0-31 of the K tile from (a0, w0); (a1, w1) = k 32-63 requested behind the first MFMA group, piece 0 of the cursor's stage behind the second
#pragma unroll
      for (int ni = 0; ni < SC_NI; ++ni) {
#pragma unroll
        for (int mi = 0; mi < 4; ++mi) acc[ni][mi] = mfma16(w0[ni], a0[mi], acc[ni][mi]);
        __builtin_amdgcn_sched_barrier(0);
        if (ni == 0) read_frags(st, 1, a1, w1);
        else stage_piece(st_new, 0);
        __builtin_amdgcn_sched_barrier(0);
      }
      // this wave's pieces of the next K tile have landed (the two newer tiles and the half just requested stay in flight) and its LDS reads
      // have returned: past the barrier the next tile is whole and nobody reads the stage the cursor writes next
      constexpr int KEEP = SC_LPT * (SC_NST - 3) + SC_LPT / 2;
      __builtin_amdgcn_s_waitcnt(0x0070 | (KEEP & 15) | ((KEEP >> 4) << 14));
      AHA_SCORE_BAR();
      read_frags(st_next, 0, a0, w0);
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int ni = 0; ni < SC_NI; ++ni) {
#pragma unroll
        for (int mi = 0; mi < 4; ++mi) acc[ni][mi] = mfma16(w1[ni], a1[mi], acc[ni][mi]);
        if (ni == SC_NI - 1) {
          __builtin_amdgcn_sched_barrier(0);
          stage_piece(st_new, 1);
          __builtin_amdgcn_sched_barrier(0);
        }
      }
      advance();
      st_new = st;
      st = st_next;
    }
    const int col0 = t * SC_BN + wn * (SC_NI * 16) + G * 4;
    if ((t + 1) * SC_BN <= a.V) score_fold<false>(acc, stt, tgt, col0, a.V);
    else score_fold<true>(acc, stt, tgt, col0, a.V);
  }
  __builtin_amdgcn_s_waitcnt(0x0F70);   // the requests past the end still write their pieces: nothing in flight when the merge reuses the LDS
  AHA_SCORE_BAR();
#undef AHA_SCORE_BAR
  // the four lanes of a row (lane groups G), then the four column waves through LDS: [row][wn][word]
  float* red = reinterpret_cast<float*>(smem);
#pragma unroll
  for (int mi = 0; mi < 4; ++mi) {
    ScoreState q = score_merge_lanes<true>(stt[mi]);
    q = score_merge_lanes<false>(q);
    if (G == 0) {
      float* o = red + ((wm * 64 + mi * 16 + c) * SC_WN + wn) * SC_WORDS;
      o[0] = q.m, o[1] = q.s, o[2] = q.bv, o[3] = __uint_as_float(q.bi), o[4] = q.xt;
    }
  }
  __syncthreads();
  if (tid < SC_BM && m0 + tid < a.R) {
    auto ld = [&](int w) __attribute__((always_inline)) {
      const float* p = red + (tid * SC_WN + w) * SC_WORDS;
      return ScoreState{p[0], p[1], p[2], __float_as_uint(p[3]), p[4]};
    };
    ScoreState q = ld(0);
#pragma unroll
    for (int w = 1; w < SC_WN; ++w) q = score_merge(q, ld(w));
    float* o = a.part + ((size_t)(m0 + tid) * a.n_slices + slice) * SC_WORDS;
    o[0] = q.m, o[1] = q.s, o[2] = q.bv, o[3] = __uint_as_float(q.bi), o[4] = q.xt;
  }
}

__global__ __launch_bounds__(256) void score_rows_merge_kernel(const float* part, const int32_t* targets, int R, int n_slices, float* out) {
  const int r = blockIdx.x * 256 + threadIdx.x;
  if (r >= R) return;
  auto ld = [&](int j) __attribute__((always_inline)) {
    const float* p = part + ((size_t)r * n_slices + j) * SC_WORDS;
    return ScoreState{p[0], p[1], p[2], __float_as_uint(p[3]), p[4]};
  };
  ScoreState q = ld(0);
  for (int j = 1; j < n_slices; ++j) q = score_merge(q, ld(j));
  const float logS = logf(q.s);
  float* o = out + (size_t)r * 3;   // aha_token_score {logprob, top_id, top_logprob}
  o[0] = targets[r] < 0 ? 0.f : (q.xt - q.m) - logS;
  o[1] = __uint_as_float(q.bi);
  o[2] = -logS;
}

}  // namespace

ScorePlan plan_score_rows(int64_t R, int V, int K) {
  (void)K;
  ScorePlan p;
  p.row_blocks = (int)((R + SC_BM - 1) / SC_BM);
  const int ntn = (V + SC_BN - 1) / SC_BN;
  const int want = std::max(1, std::min(ntn, SC_CUS / std::max(1, p.row_blocks)));   // one workgroup per CU
  p.tiles_per_slice = (ntn + want - 1) / want;
  p.slices = (ntn + p.tiles_per_slice - 1) / p.tiles_per_slice;   // every slice holds a tile
  return p;
}
bool score_rows_shape_ok(int64_t R, int V, int K) {
  return R >= 1 && R < (1ll << 30) && V >= 1 && K >= BK && K % BK == 0;
}
size_t score_rows_ws_bytes(int64_t R, int V, int K) { return (size_t)R * plan_score_rows(R, V, K).slices * SC_WORDS * 4; }

void launch_score_rows(const void* h, int64_t ldh, int64_t R, const void* W, int V, int K, const int32_t* targets, void* ws, void* out,
                       hipStream_t st) {
  {   // 128 KiB of dynamic LDS: the attribute belongs to the current device's copy of the kernel
    static std::mutex mu;
    static unsigned long long done[4] = {};
    int dev = 0;
    (void)hipGetDevice(&dev);
    std::lock_guard<std::mutex> g(mu);
    if (!(dev >= 0 && dev < 256 && (done[dev >> 6] >> (dev & 63) & 1))) {
      (void)hipFuncSetAttribute(reinterpret_cast<const void*>(score_rows_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, SC_LDS);
      if (dev >= 0 && dev < 256) done[dev >> 6] |= 1ull << (dev & 63);
    }
  }
  const ScorePlan p = plan_score_rows(R, V, K);
  ScoreArgs a;
  a.h = (const bf16_t*)h, a.ldh = ldh, a.W = (const bf16_t*)W, a.targets = targets, a.part = (float*)ws;
  a.R = (int)R, a.V = V, a.K = K;
  a.n_rb = p.row_blocks, a.n_slices = p.slices, a.tiles_per_slice = p.tiles_per_slice;
  hipLaunchKernelGGL(score_rows_kernel, dim3((unsigned)(p.row_blocks * p.slices)), dim3(SC_NW * 64), SC_LDS, st, a);
  hipLaunchKernelGGL(score_rows_merge_kernel, dim3((unsigned)((R + 255) / 256)), dim3(256), 0, st, (const float*)ws, targets, (int)R, p.slices,
                     (float*)out);
}

}  // namespace aha
