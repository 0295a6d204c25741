// Batch-1 weight-streaming matvec: the kernel that bounds decode throughput.
//
//   y[n] = sum_k h[k] * W[n,k]     W (N,K) bf16 row-major (HF / candle_nn::Linear layout), h (K) bf16, f32 accumulate
//
// HBM-bound: every weight byte is read exactly once per token, so the design goal is nothing but keeping enough
// 16-byte non-temporal loads in flight per CU.  No LDS staging of W (read once, not shared between waves); the
// activation vector lives in LDS as f32 in a lane-linear image so each ds_read_b128 is conflict-free.
//   * one wave owns R consecutive rows; per 512-column chunk it issues R x U independent 1-KiB loads
//   * persistent grid-stride over row tiles; the (optional) fused RMSNorm prologue runs once per block
//   * epilogues fuse the reference's next op: residual add (qwen3/model.rs:81,86), silu(gate)*up
//     (modules.rs:81-87), f32 logits + argmax partials (generate.rs:75-84)
// Rounding points follow the reference's op boundaries: Linear output -> bf16, then each further op -> bf16.
#include <stdlib.h>

#include "gemv_body.h"

namespace aha {

namespace {

// Kernel arguments.  The values every wave needs before it can request anything (the matrix, the activation vector, the norm weights,
// the output, the shape, the grid size -- gridDim itself is an implicit kernel argument, i.e. another kernarg load) are plain leading
// parameters: 14 dwords, which gfx950 delivers in user SGPRs at wave launch (kernarg preload,
// build.py) -- a struct by value is passed by reference and its first use is a scalar load from the kernarg segment the host has just
// written, one cold round trip in front of the first request of every launch.  `aux` is the one further pointer an epilogue's first
// request needs: the residual vector, or (GEMV_SILU_MUL, which has no residual) the separate up matrix W2.  What is first used behind
// the first weight tile travels in the trailing struct and is loaded from the kernarg segment as before.  The trace pointer is tested in
// front of the first request (stamp(0)): it is null at compile time unless TRACE (AHA_GEMV_TRACE).
struct GemvTailArgs {
  float* y_f32;
  float* blk_max;
  uint32_t* blk_idx;
  void* h_out;
  unsigned long long* trace;
  int cached;
};

// PRO (gemv_body.h): 0 = the general prologue; 1 / 2 = the straight-line one, without / with norm weights (FAST only, K <= 8 / 4 * 2048).
template <int R, int U, int EPI, bool FAST, bool TRACE, int PRO>
__global__ __launch_bounds__(GEMV_THREADS) void gemv_kernel(const void* W, const void* x, const void* norm_w, void* y, const void* aux, int N,
                                                            int K, float eps, int nblk, GemvTailArgs t) {
  extern __shared__ __attribute__((aligned(16))) float xs[];  // K f32 + 8 floats reduction scratch
  GemvArgs a{};
  a.W = W; a.W2 = EPI == GEMV_SILU_MUL ? aux : nullptr; a.x = x; a.norm_w = norm_w; a.residual = EPI == GEMV_SILU_MUL ? nullptr : aux; a.y = y;
  a.y_f32 = t.y_f32; a.blk_max = t.blk_max; a.blk_idx = t.blk_idx; a.h_out = t.h_out; a.N = N; a.K = K; a.eps = eps; a.cached = t.cached;
  a.trace = TRACE ? t.trace : nullptr;
  gemv_body<R, U, EPI, FAST, PRO>(a, xs, (int)blockIdx.x, nblk);
}

struct GemvPlan { int R, U, grid; };

// Pick rows-per-wave so that there are at least ~2 tiles per CU (256 CUs), and keep R*U*NW <= 16 loads in flight.
GemvPlan plan_gemv(int N, int K, GemvEpi epi) {
  const int nchunks = (K + 511) / 512;
  const int nw = epi == GEMV_SILU_MUL ? 2 : 1;
  int R = 4;
  while (R > 1 && (N + 4 * R - 1) / (4 * R) < 1024) R >>= 1;
  if (nw == 2 && R > 2) R = 2;
  int U = 16 / (R * nw);
  if (U > nchunks) U = nchunks;
  if (U > 8) U = 8;
  if (U < 1) U = 1;
  // U must be one of the instantiated values {1,2,4,8}
  int Up = 1;
  while (Up * 2 <= U) Up *= 2;
  // persistent blocks: 3 per CU on 256 CUs (<= 160 VGPRs: 12 waves per CU).  A/B on the Qwen3-VL-8B decode step, same box:
  // 512 -> 267.7 tok/s, 640 -> 270.9, 768 -> 276.2, 1024 -> 269.6.
  int gmax = 768;
  // tuning knobs for scripts/bench_gemv.py (not used by the product path unless set)
  static const char* e_grid = getenv("AHA_GEMV_GRID");
  static const char* e_r = getenv("AHA_GEMV_R");
  static const char* e_u = getenv("AHA_GEMV_U");
  if (e_grid) gmax = atoi(e_grid);
  static const char* e_grid1 = getenv("AHA_GEMV_GRID_R1");  // separate cap for the 1-row-per-wave kernels (118 VGPRs: 4 blocks per CU fit)
  if (e_grid1 && R == 1) gmax = atoi(e_grid1);
  if (e_r) {
    R = atoi(e_r);
    if (nw == 2 && R > 2) R = 2;
  }
  if (e_u) Up = atoi(e_u);
  if (e_r || e_u) {
    if (Up > nchunks) Up = nchunks;
    int q = 1;
    while (q * 2 <= Up) q *= 2;
    Up = q;
  }
  const int ntiles = (N + 4 * R - 1) / (4 * R);
  // whole rounds (gemv_body.h) unless a knob says otherwise
  static const bool even_on = [] { const char* e = getenv("AHA_GEMV_EVEN_GRID"); return e ? atoi(e) != 0 : true; }();
  const bool even = even_on && !e_grid && !(e_grid1 && R == 1);
  const int grid = even ? gemv_whole_rounds_grid(ntiles, gmax) : ntiles < gmax ? ntiles : gmax;
  return {R, Up, grid};
}

// AHA_GEMV_CACHED overrides GemvArgs::cached (temporal weight loads: the general form only)
int cached_or_env(int cached) {
  static const char* e_cached = getenv("AHA_GEMV_CACHED");
  return e_cached ? atoi(e_cached) : cached;
}

// The forms a launch takes for a shape, for launch_gemv_epi and debug_plan_gemv alike.
// FAST (gemv_body.h): every chunk group full and in range, weights non-temporal.  PRO: gemv_pro_of.
void form_of(const GemvPlan& p, int N, int K, bool has_norm, int cached, bool* fast, int* pro) {
  static const bool fast_ok = [] { const char* e = getenv("AHA_GEMV_FAST"); return e ? atoi(e) != 0 : true; }();
  *fast = fast_ok && K % (512 * p.U) == 0 && !cached && N >= 1;
  *pro = gemv_pro_of(K, has_norm, *fast);
}

}  // namespace

int gemv_num_tiles(int N, int K) { return plan_gemv(N, K, GEMV_LOGITS).grid; }

void debug_plan_gemv(int N, int K, GemvEpi epi, bool has_norm, int* out5) {
  const GemvPlan p = plan_gemv(N, K, epi);
  bool fast;
  int pro;
  form_of(p, N, K, has_norm, cached_or_env(0), &fast, &pro);
  out5[0] = p.R; out5[1] = p.U; out5[2] = p.grid; out5[3] = fast ? 1 : 0; out5[4] = pro;
}

template <int EPI>
static void launch_gemv_epi(const GemvArgs& a, const GemvPlan& p, hipStream_t st) {
  const size_t lds = (size_t)((a.K + 511) / 512) * 512 * 4 + 64;
  dim3 grid(p.grid), block(GEMV_THREADS);
  bool fast;
  int pro;
  form_of(p, a.N, a.K, a.norm_w != nullptr, a.cached, &fast, &pro);
  const GemvTailArgs t{a.y_f32, a.blk_max, a.blk_idx, a.h_out, a.trace, a.cached};
  const void* aux = EPI == GEMV_SILU_MUL ? a.W2 : a.residual;
#define GV_(RR, UU, FF, TT, PP) \
  hipLaunchKernelGGL((gemv_kernel<RR, UU, EPI, FF, TT, PP>), grid, block, lds, st, a.W, a.x, a.norm_w, a.y, aux, a.N, a.K, a.eps, p.grid, t)
#define GV(RR, UU)                                                      \
  do {                                                                  \
    if (a.trace == nullptr) {                                           \
      if (pro == 2) GV_(RR, UU, true, false, 2); else if (pro == 1) GV_(RR, UU, true, false, 1);      \
      else if (fast) GV_(RR, UU, true, false, 0); else GV_(RR, UU, false, false, 0);                  \
    } else {                                                            \
      if (pro == 2) GV_(RR, UU, true, true, 2); else if (pro == 1) GV_(RR, UU, true, true, 1);        \
      else if (fast) GV_(RR, UU, true, true, 0); else GV_(RR, UU, false, true, 0);                    \
    }                                                                   \
  } while (0)
  if (p.R == 4) {
    if (p.U >= 4) GV(4, 4); else if (p.U == 2) GV(4, 2); else GV(4, 1);
  } else if (p.R == 2) {
    if (p.U >= 8) GV(2, 8); else if (p.U == 4) GV(2, 4); else if (p.U == 2) GV(2, 2); else GV(2, 1);
  } else {
    if (p.U >= 8) GV(1, 8); else if (p.U == 4) GV(1, 4); else if (p.U == 2) GV(1, 2); else GV(1, 1);
  }
#undef GV
#undef GV_
}

void launch_gemv(const GemvArgs& a_in, GemvEpi epi, hipStream_t st) {
  GemvArgs a = a_in;
  a.cached = cached_or_env(a.cached);
  const GemvPlan p = plan_gemv(a.N, a.K, epi);
  switch (epi) {
    case GEMV_STORE: launch_gemv_epi<GEMV_STORE>(a, p, st); break;
    case GEMV_RESIDUAL: launch_gemv_epi<GEMV_RESIDUAL>(a, p, st); break;
    case GEMV_SILU_MUL: launch_gemv_epi<GEMV_SILU_MUL>(a, p, st); break;
    case GEMV_LOGITS: launch_gemv_epi<GEMV_LOGITS>(a, p, st); break;
    case GEMV_PARTIAL_F32: launch_gemv_epi<GEMV_PARTIAL_F32>(a, p, st); break;
  }
}

}  // namespace aha
