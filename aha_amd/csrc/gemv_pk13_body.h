// Body of the batch-1 matvec from the exact 13-bit copy of a bf16 matrix (kernels_gemv_pk13.hip has the design notes and the format):
// gemv_body (gemv_body.h) with another weight load.  Lane roles, the LDS image of the activation vector, the prologue, the tile walk, the
// two register buffers, the fma order and the epilogues' rounding points are gemv_body's, and every f32 operand is rebuilt to the bits
// lo_bf / hi_bf give on W, so that every output bit equals gemv_kernel on W.
#pragma once
#include "gemv_body.h"   // xs_index, silu_f, GEMV_THREADS, GEMV_WAVES; the host rules and GemvCopyTailArgs

namespace aha {

typedef __attribute__((ext_vector_type(2))) uint32_t pk13_u32x2_t;
typedef __attribute__((ext_vector_type(2))) uint16_t pk13_u16x2_t;

constexpr int PK13_UNIT_K = 4096;        // columns of a unit: eight 512-column chunks of one row
constexpr int PK13_UNIT_BYTES = 6656;    // 4 x 1 KiB low bytes, 2 x 1 KiB exponent codes, 512 B signs
constexpr int PK13_OFF_H = 4096, PK13_OFF_S = 6144;

__device__ __forceinline__ pk13_u32x2_t pk13_ld_nt8(const void* p) { return __builtin_nontemporal_load(reinterpret_cast<const pk13_u32x2_t*>(p)); }

// One (row, unit) in registers: 26 dwords for a lane's 64 weights.
struct Pk13Unit {
  u32x4_t a[4];      // low bytes: piece p holds chunks 2p, 2p + 1, a dword = elements 0..3 or 4..7 of a chunk
  u32x4_t h[2];      // exponent codes: dword c & 3 of piece c >> 2 = chunk c, byte i = h[element i] | h[element i + 4] << 4
  pk13_u32x2_t s;    // signs: dword c >> 2, bit ((c & 3) * 2 + (e >> 2)) + 8 * (e & 3)
};

// Four weights' high bytes s | E >> 1 from their codes x (one per byte, 0..15), the sign word sd and group g = (c & 3) * 2 + (e >> 2):
// a code of 0 stays 0 (E >> 1 == 0), any other becomes bh + code -- one packed 16-bit multiply-add of the non-zero mask, no carry between
// bytes because bh + 15 <= 127.
__device__ __forceinline__ uint32_t pk13_high4(uint32_t x, uint32_t sd, pk13_u16x2_t bh2, int g) {
  const uint32_t nz = ((x + 0x0f0f0f0fu) >> 4) & 0x01010101u;
  const pk13_u16x2_t r = __builtin_bit_cast(pk13_u16x2_t, nz) * bh2 + __builtin_bit_cast(pk13_u16x2_t, x);
  return __builtin_bit_cast(uint32_t, r) | ((sd << (7 - g)) & 0x80808080u);
}

// f32 with high byte hb[e] and second byte lo[e]: the bf16 bits of element e, shifted up 16
template <int E>
__device__ __forceinline__ float pk13_f32(uint32_t hb, uint32_t lo) {
  return __uint_as_float(__builtin_amdgcn_perm(hb, lo, 0x04000c0cu + 0x01010000u * E));
}

// a.W: the copy: rows in the order of W, (K / 4096) units of PK13_UNIT_BYTES per row; GEMV_SILU_MUL: the fused matrix (2N rows); a.bh: the
// matrix's exponent base (GemvArgs, kernels.h); K % 4096 == 0.

// Exception rows (the twin kernel, EXC): rows of W that hold a finite weight below the matrix's window.  The copy has an arbitrary code at
// such a weight, so the wave that owns such a row runs the bf16 kernel's chain over the row of W itself, in front of its main loop, and at
// the end of the row its epilogue takes that sum in place of the one the copy gave.
struct Pk13ExcRows {
  const void* W;             // the bf16 matrix the copy was made of
  int n;                     // rows in use
  int row[PK13_MAX_EXC];     // rows of W, in W's own order (GEMV_SILU_MUL: of the fused matrix); unused entries -1
};

// xs: LDS, (K + 16) floats (EXC: K + 32).  PRO as in gemv_body: 1 / 2 = the straight-line prologue without / with norm weights, 0 = the
// general one.  Always the FAST form: a work item is one unit of each of the wave's R (x 2 for gate / up) rows, nothing is predicated.
template <int R, int EPI, int PRO, bool EXC = false>
__device__ __forceinline__ void gemv_pk13_body(const GemvArgs& a, float* xs, const int bid, const int nblk, const Pk13ExcRows& ex = Pk13ExcRows{}) {
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);   // wave-uniform: the row pointers live in SGPRs
  const int K = a.K, N = a.N;
  const int nchunks = K >> 9;
  float* red = xs + (nchunks << 9);

  constexpr int ROWS_PER_TILE = GEMV_WAVES * R;
  constexpr int NW = (EPI == GEMV_SILU_MUL) ? 2 : 1;
  const int n_out = N;
  const int ntiles = (n_out + ROWS_PER_TILE - 1) / ROWS_PER_TILE;
  const int gpt = K >> 12;                                  // units per row = work items per tile
  const int my_tiles = (ntiles - bid + nblk - 1) / nblk;
  const int ngroups = my_tiles * gpt;
  const uint8_t* P = (const uint8_t*)a.W;
  const size_t prow = (size_t)gpt * PK13_UNIT_BYTES;        // bytes per row
  const pk13_u16x2_t bh2 = {(uint16_t)a.bh, (uint16_t)a.bh};

  // 7 * R * NW loads per item, in the order consume needs them (returns are in order within a wave)
  auto issue = [&](int gi, Pk13Unit (&buf)[NW][R], bf16_t (&resv)[R]) {
    const int tile = bid + (gi / gpt) * nblk;
    const int unit = gi % gpt;
    const int row0 = tile * ROWS_PER_TILE + wave * R;
    if (EPI == GEMV_RESIDUAL) {
#pragma unroll
      for (int r = 0; r < R; ++r) resv[r] = ((const bf16_t*)a.residual)[min(row0 + r, n_out - 1)];
    }
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const int row = min(row0 + r, n_out - 1);  // clamp: out-of-range rows are computed but never stored
      // NW == 2: the model's fused matrix, 16-row blocks alternating gate / up
      const size_t fr = NW == 2 ? (size_t)(row >> 4) * 32 + (row & 15) : (size_t)row;
#pragma unroll
      for (int m = 0; m < NW; ++m) {
        const uint8_t* up = P + (fr + 16 * m) * prow + (size_t)unit * PK13_UNIT_BYTES;
        Pk13Unit& b = buf[m][r];
        b.s = pk13_ld_nt8(up + PK13_OFF_S + lane * 8);
        b.h[0] = ld_nt16(up + PK13_OFF_H + lane * 16);
        b.a[0] = ld_nt16(up + lane * 16);
        b.a[1] = ld_nt16(up + 1024 + lane * 16);
        b.h[1] = ld_nt16(up + PK13_OFF_H + 1024 + lane * 16);
        b.a[2] = ld_nt16(up + 2048 + lane * 16);
        b.a[3] = ld_nt16(up + 3072 + lane * 16);
      }
    }
  };

  // The prologue is gemv_body's (stand-alone form): its inputs are requested first, the first work item right behind them, and in the
  // straight-line forms nothing is loaded under a run-time condition, so every wait in front of the barrier that ends the prologue is a
  // counted one that leaves the first request in flight.
  constexpr int XPRE = 8;
  constexpr bool SL = PRO != 0, SL_NORM = PRO == 2;
  constexpr int XSL = SL_NORM ? 4 : XPRE;
  const bool pre = SL || (nchunks << 6) <= XPRE * GEMV_THREADS;
  u32x4_t xpre[XPRE], npre[XPRE];
  Pk13Unit bufA[NW][R], bufB[NW][R];
  bf16_t resA[R], resB[R];
  if (SL) {
    const int vlast = (K >> 3) - 1;
#pragma unroll
    for (int j = 0; j < XSL; ++j) {
      const int v = min(tid + j * GEMV_THREADS, vlast);
      xpre[j] = ld16((const bf16_t*)a.x + v * 8);
      if (SL_NORM) npre[j] = ld16((const bf16_t*)a.norm_w + v * 8);
    }
    __builtin_amdgcn_sched_barrier(0);
    issue(0, bufA, resA);
    __builtin_amdgcn_sched_barrier(0);
  } else {
    if (pre) {
#pragma unroll
      for (int j = 0; j < XPRE; ++j) {
        const int v = tid + j * GEMV_THREADS;
        xpre[j] = u32x4_t{0u, 0u, 0u, 0u};
        npre[j] = u32x4_t{0u, 0u, 0u, 0u};
        if (v * 8 < K) {
          xpre[j] = ld16((const bf16_t*)a.x + v * 8);
          if (a.norm_w != nullptr) npre[j] = ld16((const bf16_t*)a.norm_w + v * 8);
        }
      }
    }
    issue(0, bufA, resA);   // the grid never exceeds the tile count: every block has a first item
  }

  // ---- prologue: h = x, or h = bf16(RMSNorm(x) * norm_w) ----------------------------------------------------------
  {
    const bf16_t* x = (const bf16_t*)a.x;
    const bf16_t* nw = (const bf16_t*)a.norm_w;
    float ss = 0.f;
    auto stage = [&](int v, u32x4_t xv) {
      float f[8];
#pragma unroll
      for (int j = 0; j < 4; ++j) { f[2 * j] = lo_bf(xv[j]); f[2 * j + 1] = hi_bf(xv[j]); }
#pragma unroll
      for (int j = 0; j < 8; ++j) ss += f[j] * f[j];
      const int base = xs_index(v * 8);
      *reinterpret_cast<float4*>(xs + base) = make_float4(f[0], f[1], f[2], f[3]);
      *reinterpret_cast<float4*>(xs + base + 256) = make_float4(f[4], f[5], f[6], f[7]);
    };
    if (pre) {
#pragma unroll
      for (int it = 0; it < (SL ? XSL : XPRE); ++it) {
        const int v = tid + it * GEMV_THREADS;
        if (v < (nchunks << 6)) stage(v, xpre[it]);
      }
    } else {
      for (int v = tid; v < (nchunks << 6); v += GEMV_THREADS) stage(v, ld16(x + v * 8));
    }
    if (SL ? SL_NORM : nw != nullptr) {
      ss = wave_sum(ss);
      if (lane == 0) red[wave] = ss;
      __syncthreads();
      const float tot = red[0] + red[1] + red[2] + red[3];
      const float rinv = 1.0f / sqrtf(tot / (float)K + a.eps);
      auto norm = [&](int v, u32x4_t wv) {
        const int base = xs_index(v * 8);
        float4 lo = *reinterpret_cast<float4*>(xs + base), hi = *reinterpret_cast<float4*>(xs + base + 256);
        lo.x = rbf(lo.x * rinv * lo_bf(wv[0])); lo.y = rbf(lo.y * rinv * hi_bf(wv[0]));
        lo.z = rbf(lo.z * rinv * lo_bf(wv[1])); lo.w = rbf(lo.w * rinv * hi_bf(wv[1]));
        hi.x = rbf(hi.x * rinv * lo_bf(wv[2])); hi.y = rbf(hi.y * rinv * hi_bf(wv[2]));
        hi.z = rbf(hi.z * rinv * lo_bf(wv[3])); hi.w = rbf(hi.w * rinv * hi_bf(wv[3]));
        *reinterpret_cast<float4*>(xs + base) = lo;
        *reinterpret_cast<float4*>(xs + base + 256) = hi;
        if (a.h_out != nullptr && bid == 0) {
          u32x4_t o;
          o[0] = pack_bf(lo.x, lo.y); o[1] = pack_bf(lo.z, lo.w); o[2] = pack_bf(hi.x, hi.y); o[3] = pack_bf(hi.z, hi.w);
          *reinterpret_cast<u32x4_t*>((bf16_t*)a.h_out + v * 8) = o;
        }
      };
      if (pre) {
#pragma unroll
        for (int it = 0; it < (SL ? XSL : XPRE); ++it) {
          const int v = tid + it * GEMV_THREADS;
          if (v < (K >> 3)) norm(v, npre[it]);
        }
      } else {
        for (int v = tid; v < (K >> 3); v += GEMV_THREADS) norm(v, ld16(nw + v * 8));
      }
    }
    __syncthreads();
  }
  // nothing of the first item's decoding in front of that barrier: it depends on no LDS value, and a scheduler that hoists it puts the
  // wait for the weights into the prologue
  __builtin_amdgcn_sched_barrier(0);

  // ---- main: consume item g while item g+1 is in flight ------------------------------------------------------------
  float tile_best = -INFINITY;
  uint32_t tile_best_i = 0xffffffffu;
  float acc[NW][R];
#pragma unroll
  for (int m = 0; m < NW; ++m)
#pragma unroll
    for (int r = 0; r < R; ++r) acc[m][r] = 0.f;

  // EXC: the sums of the exception rows this wave owns, from W itself and in front of the main loop: a lane's chain over the row, chunks
  // 0 .. nchunks - 1, with gemv_body's loads, operands and fma order, then the wave sum every row ends with -- the bits the bf16 kernel
  // hands to its epilogue.  They wait in LDS (exc[i] for list entry i, read back by the wave that wrote it) until the row's epilogue
  // takes them in place of what the copy gave.  Here and not at the row end: the first buffer is in flight and nothing else is live, while
  // a chain inside consume() splits the blocks the scheduler sees and cost the gate / up and logits forms their third wave per SIMD
  // (195 VGPRs).  The sched_barriers keep the eight loads of a unit together and the LDS vectors to one chunk at a time.
  float* exc = red + 16;
  if (EXC) {
    for (int i = 0; i < ex.n; ++i) {
      int wr = -1;
#pragma unroll
      for (int j = 0; j < PK13_MAX_EXC; ++j) wr = j == i ? ex.row[j] : wr;
      const int orow = NW == 2 ? (wr >> 5) * 16 + (wr & 15) : wr;          // the output row it belongs to
      const int otile = orow / ROWS_PER_TILE;
      if (otile % nblk != bid || (orow % ROWS_PER_TILE) / R != wave) continue;
      const bf16_t* wp = (const bf16_t*)ex.W + (size_t)wr * K + lane * 8;
      float s = 0.f;
#pragma unroll 1
      for (int u = 0; u < gpt; ++u) {
        u32x4_t w[8];
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int c = 0; c < 8; ++c) w[c] = ld16(wp + ((u * 8 + c) << 9));
#pragma unroll
        for (int c = 0; c < 8; ++c) {
          __builtin_amdgcn_sched_barrier(0);
          const float4 xlo = *reinterpret_cast<const float4*>(xs + ((u * 8 + c) << 9) + (lane << 2));
          const float4 xhi = *reinterpret_cast<const float4*>(xs + ((u * 8 + c) << 9) + 256 + (lane << 2));
          s = fmaf(xlo.x, lo_bf(w[c][0]), s); s = fmaf(xlo.y, hi_bf(w[c][0]), s);
          s = fmaf(xlo.z, lo_bf(w[c][1]), s); s = fmaf(xlo.w, hi_bf(w[c][1]), s);
          s = fmaf(xhi.x, lo_bf(w[c][2]), s); s = fmaf(xhi.y, hi_bf(w[c][2]), s);
          s = fmaf(xhi.z, lo_bf(w[c][3]), s); s = fmaf(xhi.w, hi_bf(w[c][3]), s);
        }
        __builtin_amdgcn_sched_barrier(0);
      }
      s = wave_sum(s);
      if (lane == 0) exc[i] = s;
    }
    __builtin_amdgcn_sched_barrier(0);
  }

  auto consume = [&](int gi, Pk13Unit (&buf)[NW][R], bf16_t (&resv)[R]) {
    const int c0 = (gi % gpt) * 8;
#pragma unroll
    for (int c = 0; c < 8; ++c) {
      const float4 xlo = *reinterpret_cast<const float4*>(xs + ((c0 + c) << 9) + (lane << 2));
      const float4 xhi = *reinterpret_cast<const float4*>(xs + ((c0 + c) << 9) + 256 + (lane << 2));
#pragma unroll
      for (int m = 0; m < NW; ++m)
#pragma unroll
        for (int r = 0; r < R; ++r) {
          const Pk13Unit& b = buf[m][r];
          const uint32_t hd = b.h[c >> 2][c & 3], sd = b.s[c >> 2];
          const uint32_t lo0 = b.a[c >> 1][(c & 1) * 2], lo1 = b.a[c >> 1][(c & 1) * 2 + 1];
          const uint32_t h0 = pk13_high4(hd & 0x0f0f0f0fu, sd, bh2, (c & 3) * 2);
          const uint32_t h1 = pk13_high4((hd >> 4) & 0x0f0f0f0fu, sd, bh2, (c & 3) * 2 + 1);
          float s = acc[m][r];
          // gemv_body's order: elements 0..7 ascending, the activation as the first operand
          s = fmaf(xlo.x, pk13_f32<0>(h0, lo0), s); s = fmaf(xlo.y, pk13_f32<1>(h0, lo0), s);
          s = fmaf(xlo.z, pk13_f32<2>(h0, lo0), s); s = fmaf(xlo.w, pk13_f32<3>(h0, lo0), s);
          s = fmaf(xhi.x, pk13_f32<0>(h1, lo1), s); s = fmaf(xhi.y, pk13_f32<1>(h1, lo1), s);
          s = fmaf(xhi.z, pk13_f32<2>(h1, lo1), s); s = fmaf(xhi.w, pk13_f32<3>(h1, lo1), s);
          acc[m][r] = s;
        }
    }
    if (gi % gpt != gpt - 1) return;
    const int tile = bid + (gi / gpt) * nblk;
    const int row0 = tile * ROWS_PER_TILE + wave * R;
#pragma unroll
    for (int m = 0; m < NW; ++m)
#pragma unroll
      for (int r = 0; r < R; ++r) acc[m][r] = wave_sum(acc[m][r]);
    if (EXC) {
      // the row of W behind each sum is wave-uniform and the list sits in SGPRs: scalar compares, and one LDS word under a branch that is
      // taken for at most PK13_MAX_EXC rows of the matrix (a clamped row may read a word nobody wrote: it is never stored)
#pragma unroll
      for (int r = 0; r < R; ++r) {
        const int row = min(row0 + r, n_out - 1);
        const int fr = NW == 2 ? (row >> 4) * 32 + (row & 15) : row;
#pragma unroll
        for (int m = 0; m < NW; ++m) {
          int hit = -1;
#pragma unroll
          for (int i = 0; i < PK13_MAX_EXC; ++i) hit = ex.row[i] == fr + 16 * m ? i : hit;
          if (__builtin_expect(hit >= 0, 0)) acc[m][r] = exc[hit];
        }
      }
    }
    if (lane == 0) {
#pragma unroll
      for (int r = 0; r < R; ++r) {
        const int row = row0 + r;
        if (row < n_out) {
          const float lin = rbf(acc[0][r]);
          if (EPI == GEMV_STORE) {
            ((bf16_t*)a.y)[row] = f2bf(lin);
          } else if (EPI == GEMV_RESIDUAL) {
            ((bf16_t*)a.y)[row] = f2bf(bf2f(resv[r]) + lin);
          } else if (EPI == GEMV_SILU_MUL) {
            const float g = rbf(silu_f(lin));
            const float up = rbf(acc[NW - 1][r]);
            ((bf16_t*)a.y)[row] = f2bf(g * up);
          } else {  // GEMV_LOGITS
            a.y_f32[row] = lin;
            if (lin > tile_best || (lin == tile_best && (uint32_t)row < tile_best_i)) { tile_best = lin; tile_best_i = row; }
          }
        }
      }
    }
#pragma unroll
    for (int m = 0; m < NW; ++m)
#pragma unroll
      for (int r = 0; r < R; ++r) acc[m][r] = 0.f;
  };

  int g = 0;
  for (; g + 2 < ngroups; g += 2) {   // steady state: both refills unconditional
    __builtin_amdgcn_sched_barrier(0);
    issue(g + 1, bufB, resB);
    __builtin_amdgcn_sched_barrier(0);
    consume(g, bufA, resA);
    __builtin_amdgcn_sched_barrier(0);
    issue(g + 2, bufA, resA);
    __builtin_amdgcn_sched_barrier(0);
    consume(g + 1, bufB, resB);
  }
  if (g + 1 < ngroups) {
    __builtin_amdgcn_sched_barrier(0);
    issue(g + 1, bufB, resB);
    __builtin_amdgcn_sched_barrier(0);
    consume(g, bufA, resA);
    consume(g + 1, bufB, resB);
  } else if (g < ngroups) {
    consume(g, bufA, resA);
  }
  if (EPI == GEMV_LOGITS) {
    // per-block argmax partial: 4 wave leaders -> slot bid
    __syncthreads();
    if (lane == 0) { red[wave] = tile_best; reinterpret_cast<uint32_t*>(red)[4 + wave] = tile_best_i; }
    __syncthreads();
    if (tid == 0) {
      float bv = red[0];
      uint32_t bi = reinterpret_cast<uint32_t*>(red)[4];
      for (int w = 1; w < 4; ++w) {
        const float v = red[w];
        const uint32_t i = reinterpret_cast<uint32_t*>(red)[4 + w];
        if (v > bv || (v == bv && i < bi)) { bv = v; bi = i; }
      }
      a.blk_max[bid] = bv;
      a.blk_idx[bid] = bi;
    }
  }
}

}  // namespace aha
