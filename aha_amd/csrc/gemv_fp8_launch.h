// Host side of the batch-1 matvec from MXFP8 / MXFP4 weights: the plan, the forms and the dispatch over the shipped instantiations, one
// text for kernels_gemv_fp8.hip and kernels_gemv_fp4.hip.  A format brings its kernel (KS::get<R, U, EPI, FAST, PRO>()) and says how many
// weight loads its plan keeps per wave and buffer.
#pragma once
#include <stdlib.h>

#include <algorithm>

#include "gemv_fp8_body.h"
#include "kernels.h"

namespace aha {

namespace {

// The kernels' parameters (kernels_gemv.hip has the reasoning): the 14 leading dwords are q, scales, x, norm_w, y, the residual vector, N and
// K; what is first used behind the first weight request travels in GemvCopyTailArgs (gemv_body.h).
struct GemvFp8Plan { int R, U, grid; };

// N: output rows (GEMV_SILU_MUL: I).  Rows per wave so that there are at least 512 tiles (two per CU), then as many chunks per item as
// keep R * U * NW = loads (16), at most 8 and at most the row's chunks (a power of two).
GemvFp8Plan plan_gemv_mx(int N, int K, GemvEpi epi, int loads) {
  const int nchunks = (K + 511) / 512;
  const int nw = epi == GEMV_SILU_MUL ? 2 : 1;
  int R = 4;
  while (R > 1 && (N + 4 * R - 1) / (4 * R) < 512) R >>= 1;
  if (nw == 2 && R > 2) R = 2;
  int U = std::min(std::min(loads / (R * nw), 8), nchunks);
  int Up = 1;
  while (Up * 2 <= U) Up *= 2;
  // persistent blocks: 3 per CU on 256 CUs, as plan_gemv (the 16-load FP8 instantiations take 160 .. 169 VGPRs: 12 waves per CU, which
  // with two buffers of 16 half-KiB requests each is the bytes in flight of the bf16 kernel's 8-load plans)
  const int gmax = 768;
  const int ntiles = (N + 4 * R - 1) / (4 * R);
  const int grid = gemv_whole_rounds_grid(ntiles, gmax);   // whole rounds, as plan_gemv
  return {R, Up, std::max(grid, 1)};
}

// the forms a launch takes for a shape: FAST = every chunk group full; PRO = the straight-line prologue
void form_of(const GemvFp8Plan& p, int K, bool has_norm, bool* fast, int* pro) {
  *fast = K % (512 * p.U) == 0;
  *pro = gemv_pro_of(K, has_norm, *fast);
}

void debug_plan_out(const GemvFp8Plan& p, int K, bool has_norm, int* out5) {
  bool fast;
  int pro;
  form_of(p, K, has_norm, &fast, &pro);
  out5[0] = p.R; out5[1] = p.U; out5[2] = p.grid; out5[3] = fast ? 1 : 0; out5[4] = pro;
}

template <class KS, int EPI>
void launch_mx_epi(const GemvArgs& a, const GemvFp8Plan& p, hipStream_t st) {
  const size_t lds = (size_t)((a.K + 511) / 512) * 512 * 4 + 64;
  dim3 grid(p.grid), block(GEMV_THREADS);
  bool fast;
  int pro;
  form_of(p, a.K, a.norm_w != nullptr, &fast, &pro);
  const GemvCopyTailArgs t{a.y_f32, a.blk_max, a.blk_idx, a.h_out, a.eps, p.grid};
#define GV_(RR, UU, FF, PP) \
  hipLaunchKernelGGL((KS::template get<RR, UU, EPI, FF, PP>()), grid, block, lds, st, a.W, a.scales, a.x, a.norm_w, a.y, a.residual, a.N, a.K, t)
  // U at the plan's cap (the row has at least 2 * U chunks or exactly U): every form
#define GV_FULL(RR, UU)                                                                 \
  do {                                                                                  \
    if (pro == 2) GV_(RR, UU, true, 2); else if (pro == 1) GV_(RR, UU, true, 1);        \
    else if (fast) GV_(RR, UU, true, 0); else GV_(RR, UU, false, 0);                    \
  } while (0)
  // U below the cap: the row has fewer than 2 * U chunks, so a FAST shape is K = 512 * U <= 2048 and always straight-line
#define GV_SHORT(RR, UU)                                                                \
  do {                                                                                  \
    if (pro == 2) GV_(RR, UU, true, 2); else if (pro == 1) GV_(RR, UU, true, 1);        \
    else GV_(RR, UU, false, 0);                                                         \
  } while (0)
  constexpr int NW = EPI == GEMV_SILU_MUL ? 2 : 1;
  if (p.R == 4) {
    if constexpr (NW == 1) {
      if (p.U >= 4) GV_FULL(4, 4); else if (p.U == 2) GV_SHORT(4, 2); else GV_SHORT(4, 1);
    }
  } else if (p.R == 2) {
    if constexpr (NW == 1) {
      if (p.U >= 8) GV_FULL(2, 8); else if (p.U == 4) GV_SHORT(2, 4); else if (p.U == 2) GV_SHORT(2, 2); else GV_SHORT(2, 1);
    } else {
      if (p.U >= 4) GV_FULL(2, 4); else if (p.U == 2) GV_SHORT(2, 2); else GV_SHORT(2, 1);
    }
  } else {
    if (p.U >= 8) GV_FULL(1, 8); else if (p.U == 4) GV_SHORT(1, 4); else if (p.U == 2) GV_SHORT(1, 2); else GV_SHORT(1, 1);
  }
#undef GV_SHORT
#undef GV_FULL
#undef GV_
}

// launch_gemv with (q, scales) in place of g.W, by plan p
template <class KS>
void launch_mx(const GemvArgs& g, const void* q, const uint32_t* scales, GemvEpi epi, const GemvFp8Plan& p, hipStream_t st) {
  GemvArgs a = g;
  a.W = q; a.scales = (const uint8_t*)scales;
  switch (epi) {
    case GEMV_STORE: launch_mx_epi<KS, GEMV_STORE>(a, p, st); break;
    case GEMV_RESIDUAL: launch_mx_epi<KS, GEMV_RESIDUAL>(a, p, st); break;
    case GEMV_SILU_MUL: launch_mx_epi<KS, GEMV_SILU_MUL>(a, p, st); break;
    case GEMV_LOGITS: launch_mx_epi<KS, GEMV_LOGITS>(a, p, st); break;
    default: abort();   // GEMV_PARTIAL_F32: sharded models have no copies
  }
}

}  // namespace

}  // namespace aha
