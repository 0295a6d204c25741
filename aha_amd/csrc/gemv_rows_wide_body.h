// The batched decode matvec for 33 .. 128 rows of x in ONE pass over the weights (kernels_gemv_rows_wide.hip instantiates it for the three
// weight forms of gemv_rows_body.h).  gemv_rows_body holds the x fragments of all its row tiles at once (xf[CW][NRT][4]: CW * NRT * 16
// VGPRs), which ends at two tiles; this body turns the loop nest round.  A wave requests the weights of its CW chunks once, converts an MX
// form's bytes to bf16 fragments once -- not once per row tile -- and keeps the CW * 2 * 4 fragments in registers (32 * CW VGPRs).  It
// then walks the row tiles: the x fragments of tile rt + 1 are requested before the MFMAs of tile rt, in the other of two register
// sets (16 * CW VGPRs each), so every wait is a counted vmcnt and no load sits under a run-time condition (a tile past the last one
// re-reads row R - 1: DESIGN section 4, compiler facts).  A tile's two accumulators (one per column tile) go to LDS as soon as its
// CW * 4 MFMA steps are done, so the accumulators take 8 VGPRs whatever the row count, and the row-tile loop is a plain uniform loop over
// ceil(R / 16) tiles in steps of two -- 48 rows run three tiles' worth of x, not four.
//
// The contract: every f32 partial ws[ks][row][n] is, bit for bit, what gemv_rows_body writes for that row in a launch of at most 32
// rows.  What fixes a partial's bits is the same text here as there: gemv_rows_plan(N, K) (the launcher), wave w of split ks owning
// chunks (ks * 4 + w) * CW .., lane group q holding k q * 32 .. of a chunk with MFMA step j at + j * 8, chunk-major then j = 0..3 into one
// accumulator per (row tile, column tile), ((w0 + w1) + w2) + w3 through LDS, zero x for rows past R and k past K.  An MFMA output row
// depends on its own A row only, so which tile a row sits in, and what rides beside it, does not show.
//
// x traffic: a block still owns GR_NB = 32 columns, so every column block re-reads its K range of x from L2 -- as much x traffic as the
// row groups this kernel replaces had, and no more.  The 64-column block (each x fragment feeding four column tiles) doubles the weight
// fragments to 64 * CW VGPRs and the LDS partials to 128 KiB at eight row tiles, one block per CU; profiles/gemv_rows_wide.md has what
// was measured and what was not.
#pragma once
#include "gemv_rows_body.h"

namespace aha {

// The x fragments of row tile rt for the wave's CW chunks: 4 * CW unconditional 16-byte loads, then zeros where the row is past R or the
// k past K.  The zeros are an AND with a mask (kkeep: all ones where k < K), not a select: the compiler sinks a load whose value a
// select may discard under that select's condition, and the loop's waits become vmcnt(0).
template <int CW>
__device__ __forceinline__ void grw_load_x(u32x4_t (&xf)[CW][4], gcchar_t X, int64_t ldx, int R, int rt, int c, const int (&kc)[CW][4],
                                           const uint32_t (&kkeep)[CW][4]) {
  const int row = rt * 16 + c;
  const gcchar_t xr = X + (int64_t)min(row, R - 1) * ldx * 2;
  const uint32_t rkeep = 0u - (uint32_t)(row < R);
#pragma unroll
  for (int i = 0; i < CW; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const u32x4_t v = *reinterpret_cast<gptr16_t>(xr + (int64_t)kc[i][j] * 2);
      const uint32_t keep = rkeep & kkeep[i][j];
      xf[i][j] = u32x4_t{v[0] & keep, v[1] & keep, v[2] & keep, v[3] & keep};
    }
}

// Row tile rt: chunk-major, then j, into one accumulator per column tile -- gemv_rows_body's chain -- and the two 16 x 16 results to the
// wave's LDS slot: lane l holds out[row (l >> 4) * 4 + e][col l & 15].
template <int CW, int NRT>
__device__ __forceinline__ void grw_tile(const u32x4_t (&xf)[CW][4], const u32x4_t (&wb)[CW][2][4], float* red, int wave, int rt, int c, int q) {
  f32x4_t acc[2] = {f32x4_t{0.f, 0.f, 0.f, 0.f}, f32x4_t{0.f, 0.f, 0.f, 0.f}};
#pragma unroll
  for (int i = 0; i < CW; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int nt = 0; nt < 2; ++nt) acc[nt] = mfma16(as_frag(xf[i][j]), as_frag(wb[i][nt][j]), acc[nt]);
#pragma unroll
  for (int nt = 0; nt < 2; ++nt)
#pragma unroll
    for (int e = 0; e < 4; ++e) red[((wave * 2 + nt) * NRT + rt) * 256 + (q * 4 + e) * 16 + c] = acc[nt][e];
}

// One wave: columns n0 .. n0 + 31 x chunks cbase .. cbase + CW - 1 for every row tile of x.  red: 4 * 2 * NRT * 256 floats of LDS, 16-byte
// aligned; NRT (4 or 8) bounds the row tiles (a.R <= NRT * 16) and sizes red, the loop runs ceil(a.R / 16) of them.
template <class WF, int CW, int NRT>
__device__ __forceinline__ void gemv_rows_wide_body(const GemvRowsArgs& a, const void* w, const uint32_t* wscales, float* red) {
  static_assert(NRT % 2 == 0, "the row-tile loop runs two tiles per iteration");
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int c = lane & 15, q = lane >> 4;
  const int n0 = blockIdx.x * GR_NB, ks = blockIdx.y;
  const int K = a.K, N = a.N, R = a.R;
  const int nchunks = (K + GR_CHUNK - 1) / GR_CHUNK;
  const int cbase = (ks * 4 + wave) * CW;
  const int ntiles = (R + 15) >> 4;
  const gcchar_t W = gp<gcchar_t>(w);
  const gcu32_t S = gp<gcu32_t>(wscales);
  const gcchar_t X = gp<gcchar_t>(a.x);
  // weight rows of this lane in the two column tiles (rows past N re-read row N-1: finite values whose outputs are never stored)
  const int64_t wr[2] = {min(n0 + c, N - 1), min(n0 + 16 + c, N - 1)};
  // the weights of the wave's chunks, requested once (waves past the end of K re-read the last chunk; their x is zero)
  u32x4_t wf[CW][2][WF::LOADS];
  uint32_t sw[CW][2];
  int kc[CW][4];
  uint32_t kkeep[CW][4];
#pragma unroll
  for (int i = 0; i < CW; ++i) {
    const int ch = cbase + i;
    const int chc = min(ch, nchunks - 1);
#pragma unroll
    for (int l = 0; l < WF::LOADS; ++l)
#pragma unroll
      for (int nt = 0; nt < 2; ++nt)
        wf[i][nt][l] = __builtin_nontemporal_load(reinterpret_cast<gptr16_t>(W + WF::addr(wr[nt], K, chc * GR_CHUNK + q * 32, l)));
    if constexpr (WF::SCALED) {
#pragma unroll
      for (int nt = 0; nt < 2; ++nt) sw[i][nt] = __builtin_nontemporal_load(S + (wr[nt] * nchunks + chc));
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      kc[i][j] = min(chc * GR_CHUNK + q * 32 + j * 8, K - 8);
      kkeep[i][j] = 0u - (uint32_t)(ch * GR_CHUNK + q * 32 + j * 8 < K);
    }
  }
  u32x4_t xa[CW][4], xb[CW][4];
  grw_load_x<CW>(xa, X, a.ldx, R, 0, c, kc, kkeep);
  // MFMA fragment j of (chunk, column tile): the form's bytes -> bf16 once, for all row tiles
  u32x4_t wb[CW][2][4];
#pragma unroll
  for (int i = 0; i < CW; ++i)
#pragma unroll
    for (int nt = 0; nt < 2; ++nt) {
      float s = 0.f;
      if constexpr (WF::SCALED) s = __uint_as_float(((sw[i][nt] >> (q * 8)) & 0xffu) << 23);   // byte q of the chunk's scale word -> 2^e
#pragma unroll
      for (int j = 0; j < 4; ++j) wb[i][nt][j] = WF::frag(wf[i][nt], j, s);
    }
  // tiles rt (set a) and rt + 1 (set b); ntiles odd: the last b tile is all rows past R, zeros that are never stored
  for (int rt = 0; rt < ntiles; rt += 2) {
    grw_load_x<CW>(xb, X, a.ldx, R, rt + 1, c, kc, kkeep);
    grw_tile<CW, NRT>(xa, wb, red, wave, rt, c, q);
    grw_load_x<CW>(xa, X, a.ldx, R, rt + 2, c, kc, kkeep);
    grw_tile<CW, NRT>(xb, wb, red, wave, rt + 1, c, q);
  }
  __syncthreads();
  // ((w0 + w1) + w2) + w3, then the f32 partial of this K split: ws[ks][row][n]
  gf_t ws = gp<gf_t>(a.ws) + (int64_t)ks * a.R * a.ldws;
  for (int nt = 0; nt < 2; ++nt)
    for (int e = tid; e < ntiles * 256; e += 256) {
      const int m = (e >> 4) & 15, n = e & 15;
      const int o = nt * NRT * 256 + e;   // (column tile nt, row tile e / 256) of a wave's slot
      float s = red[o];
#pragma unroll
      for (int wv = 1; wv < 4; ++wv) s += red[wv * 2 * NRT * 256 + o];
      const int row = (e >> 8) * 16 + m, col = n0 + nt * 16 + n;
      if (row < R && col < N) ws[(int64_t)row * a.ldws + col] = s;
    }
}

}  // namespace aha
