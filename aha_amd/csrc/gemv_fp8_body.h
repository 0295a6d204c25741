// Body of the batch-1 matvec from MXFP8 and MXFP4 weights (kernels_gemv_fp8.hip has the design notes, kernels_gemv_fp4.hip the FP4 form's):
// gemv_body (gemv_body.h) with the weight operand read as one E4M3 byte or one E2M1 nibble per element plus one E8M0 scale byte per 32 k.
// Lane roles, the LDS image of the activation vector, the prologue, the tile walk, the two register buffers, the fma order and the
// epilogues' rounding points are gemv_body's, so that every output bit equals gemv_kernel on W' = q * 2^e.  One text for both formats: the
// weight form WF (below) names what differs, a lane's load and its conversion.
#pragma once
#include "gemv_body.h"   // xs_index, silu_f, GEMV_THREADS, GEMV_WAVES; the host rules and GemvCopyTailArgs

namespace aha {

typedef __attribute__((ext_vector_type(2))) uint32_t u32x2_t;

// streamed-once 8-byte / 1-byte loads: the weight bytes and their scales are the only non-temporal loads of the kernel
__device__ __forceinline__ u32x2_t ld_nt8(const void* p) { return __builtin_nontemporal_load(reinterpret_cast<const u32x2_t*>(p)); }
// (returned as the byte it is: widening it where it is loaded puts a wait for it -- an `and 0xff` -- in front of the prologue)
__device__ __forceinline__ uint8_t ld_nt1(const void* p) { return __builtin_nontemporal_load(reinterpret_cast<const uint8_t*>(p)); }

// ld_nt8's 4-byte twin: a lane's 8 E2M1 codes of a chunk
__device__ __forceinline__ uint32_t ld_nt4(const void* p) { return __builtin_nontemporal_load(reinterpret_cast<const uint32_t*>(p)); }

// Weight forms.  Per 512-k chunk a lane owns k = chunk * 512 + lane * 8 .. + 7 in either: load_t is what load() fetches for them from
// the row at row(); convert() gives the 8 f32 operands, pairs in ascending k, with the block's scale 2^e folded in
// by the hardware -- exact in f32 and bit for bit what lo_bf / hi_bf give on W' (a zero code keeps its sign; 2^e is never 0 or inf).
struct GemvWFp8 {   // 8 E4M3 bytes
  typedef u32x2_t load_t;
  static __device__ __forceinline__ const uint8_t* row(const uint8_t* Q, size_t r, int K) { return Q + r * K; }
  static __device__ __forceinline__ load_t load(const uint8_t* qp, int k) { return ld_nt8(qp + k); }
  static __device__ __forceinline__ load_t zero() { return u32x2_t{0u, 0u}; }
  static __device__ __forceinline__ void convert(const load_t w, const float sf, f32x2_t (&o)[4]) {
    o[0] = __builtin_amdgcn_cvt_scalef32_pk_f32_fp8(w[0], sf, false);
    o[1] = __builtin_amdgcn_cvt_scalef32_pk_f32_fp8(w[0], sf, true);
    o[2] = __builtin_amdgcn_cvt_scalef32_pk_f32_fp8(w[1], sf, false);
    o[3] = __builtin_amdgcn_cvt_scalef32_pk_f32_fp8(w[1], sf, true);
  }
};
struct GemvWFp4 {   // 8 E2M1 codes in 4 bytes, the even k of a byte in bits 0..3 (kernels.h "MXFP4 weight copies")
  typedef uint32_t load_t;
  static __device__ __forceinline__ const uint8_t* row(const uint8_t* Q, size_t r, int K) { return Q + r * (K >> 1); }
  static __device__ __forceinline__ load_t load(const uint8_t* qp, int k) { return ld_nt4(qp + (k >> 1)); }
  static __device__ __forceinline__ load_t zero() { return 0u; }
  static __device__ __forceinline__ void convert(const load_t w, const float sf, f32x2_t (&o)[4]) {
    o[0] = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(w, sf, 0);
    o[1] = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(w, sf, 1);
    o[2] = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(w, sf, 2);
    o[3] = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(w, sf, 3);
  }
};

// a.W: (N, K) E4M3 bytes or (N, K / 2) E2M1 pairs, row-major; GEMV_SILU_MUL: the fused matrix, 16-row blocks alternating gate / up (2N rows);
// a.scales: their scale bytes (GemvArgs, kernels.h).
// xs: LDS, (ceil(K/512)*512 + 16) floats.  PRO as in gemv_body: 1 / 2 = the straight-line prologue without / with norm weights (FAST only).
template <class WF, int R, int U, int EPI, bool FAST, int PRO>
__device__ __forceinline__ void gemv_fp8_body(const GemvArgs& a, float* xs, const int bid, const int nblk) {
  const int tid = threadIdx.x, lane = tid & 63;
  // wave-uniform on purpose: a wave's row pointers then live in SGPRs and every weight / scale load is the scalar-base form with the lane's
  // byte offset in one VGPR, instead of a 64-bit address pair per load
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int K = a.K, N = a.N;
  const int nchunks = (K + 511) >> 9;  // K % 32 == 0; the tail of the last chunk is zero-filled
  float* red = xs + (nchunks << 9);

  constexpr int ROWS_PER_TILE = GEMV_WAVES * R;
  constexpr int NW = (EPI == GEMV_SILU_MUL) ? 2 : 1;
  const int n_out = N;
  const int ntiles = (n_out + ROWS_PER_TILE - 1) / ROWS_PER_TILE;
  const int gpt = (nchunks + U - 1) / U;
  const int my_tiles = (ntiles - bid + nblk - 1) / nblk;
  const int ngroups = my_tiles * gpt;
  const uint8_t* Q = (const uint8_t*)a.W;
  const uint8_t* S = a.scales;
  const size_t srow = (size_t)((K + 127) >> 7) << 2;   // scale bytes per row
  typedef typename WF::load_t load_t;

  // Per 512-k chunk a lane owns k = chunk * 512 + lane * 8 .. + 7: 8 (FP4: 4) consecutive bytes of the row, one load; four lanes share an
  // MX block, whose scale is byte chunk * 16 + (lane >> 2) of the row's scales.  R*U*NW weight loads + as many scale-byte loads per item.
  auto issue = [&](int gi, load_t (&buf)[U][NW][R], uint8_t (&sc)[U][NW][R], bf16_t (&resv)[R]) {
    const int tile = bid + (gi / gpt) * nblk;
    const int c0 = (gi % gpt) * U;
    const int row0 = tile * ROWS_PER_TILE + wave * R;
    if (FAST && EPI == GEMV_RESIDUAL) {
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
        const uint8_t* qp = WF::row(Q, fr + 16 * m, K);
        const uint8_t* sp = S + (fr + 16 * m) * srow;
#pragma unroll
        for (int u = 0; u < U; ++u) {
          const int k = ((c0 + u) << 9) + lane * 8;
          const int sb = ((c0 + u) << 4) + (lane >> 2);
          if (FAST) {
            buf[u][m][r] = WF::load(qp, k);
            sc[u][m][r] = ld_nt1(sp + sb);
            continue;
          }
          const bool ok = k < K;   // K % 32 == 0: the lane's 8 k are inside K or past it as a whole (a chunk past the last one: past it)
          buf[u][m][r] = ok ? WF::load(qp, k) : WF::zero();
          sc[u][m][r] = ok ? ld_nt1(sp + sb) : (uint8_t)127;
        }
      }
    }
  };

  // The prologue is gemv_body's (stand-alone form): its inputs are requested first, the first weight tile right behind them, and in the
  // straight-line forms nothing is loaded under a run-time condition, so every wait in front of the barrier that ends the prologue is a
  // counted one that leaves the first request -- weight bytes and scale bytes -- in flight.
  constexpr int XPRE = 8;
  constexpr bool SL = PRO != 0, SL_NORM = PRO == 2;
  constexpr int XSL = SL_NORM ? 4 : XPRE;
  static_assert(!SL || FAST, "the straight-line prologue is a form of the FAST kernel");
  const bool pre = SL || (nchunks << 6) <= XPRE * GEMV_THREADS;
  u32x4_t xpre[XPRE], npre[XPRE];
  load_t bufA[U][NW][R], bufB[U][NW][R];
  uint8_t scA[U][NW][R], scB[U][NW][R];
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
    issue(0, bufA, scA, resA);
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
    if (ngroups > 0) issue(0, bufA, scA, resA);
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
      for (int v = tid; v < (nchunks << 6); v += GEMV_THREADS) {
        u32x4_t xv = {0u, 0u, 0u, 0u};
        if (v * 8 < K) xv = ld16(x + v * 8);
        stage(v, xv);
      }
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
  // nothing of the first tile's consumption in front of that barrier: the conversions depend on no LDS value, and a scheduler that hoists
  // them puts the wait for the weights into the prologue
  __builtin_amdgcn_sched_barrier(0);

  // ---- main: consume item g while item g+1 is in flight ------------------------------------------------------------
  float tile_best = -INFINITY;
  uint32_t tile_best_i = 0xffffffffu;
  float acc[NW][R];
#pragma unroll
  for (int m = 0; m < NW; ++m)
#pragma unroll
    for (int r = 0; r < R; ++r) acc[m][r] = 0.f;

  auto consume = [&](int gi, load_t (&buf)[U][NW][R], uint8_t (&sc)[U][NW][R], bf16_t (&resv)[R]) {
    const int c0 = (gi % gpt) * U;
#pragma unroll
    for (int u = 0; u < U; ++u) {
      if (FAST || c0 + u < nchunks) {
        const float4 xlo = *reinterpret_cast<const float4*>(xs + ((c0 + u) << 9) + (lane << 2));
        const float4 xhi = *reinterpret_cast<const float4*>(xs + ((c0 + u) << 9) + 256 + (lane << 2));
#pragma unroll
        for (int m = 0; m < NW; ++m)
#pragma unroll
          for (int r = 0; r < R; ++r) {
            // code * 2^e
            const float sf = __uint_as_float((uint32_t)sc[u][m][r] << 23);
            f32x2_t w[4];
            WF::convert(buf[u][m][r], sf, w);
            float s = acc[m][r];
            // gemv_body's order: elements 0..7 ascending, the activation as the first operand
            s = fmaf(xlo.x, w[0][0], s); s = fmaf(xlo.y, w[0][1], s);
            s = fmaf(xlo.z, w[1][0], s); s = fmaf(xlo.w, w[1][1], s);
            s = fmaf(xhi.x, w[2][0], s); s = fmaf(xhi.y, w[2][1], s);
            s = fmaf(xhi.z, w[3][0], s); s = fmaf(xhi.w, w[3][1], s);
            acc[m][r] = s;
          }
      }
    }
    if (gi % gpt != gpt - 1) return;
    const int tile = bid + (gi / gpt) * nblk;
    const int row0 = tile * ROWS_PER_TILE + wave * R;
#pragma unroll
    for (int m = 0; m < NW; ++m)
#pragma unroll
      for (int r = 0; r < R; ++r) acc[m][r] = wave_sum(acc[m][r]);
    if (lane == 0) {
#pragma unroll
      for (int r = 0; r < R; ++r) {
        const int row = row0 + r;
        if (row < n_out) {
          const float lin = rbf(acc[0][r]);
          if (EPI == GEMV_STORE) {
            ((bf16_t*)a.y)[row] = f2bf(lin);
          } else if (EPI == GEMV_RESIDUAL) {
            ((bf16_t*)a.y)[row] = f2bf(bf2f(FAST ? resv[r] : ((const bf16_t*)a.residual)[row]) + lin);
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

  if (FAST) {
    int g = 0;
    for (; g + 2 < ngroups; g += 2) {   // steady state: both refills unconditional
      __builtin_amdgcn_sched_barrier(0);
      issue(g + 1, bufB, scB, resB);
      __builtin_amdgcn_sched_barrier(0);
      consume(g, bufA, scA, resA);
      __builtin_amdgcn_sched_barrier(0);
      issue(g + 2, bufA, scA, resA);
      __builtin_amdgcn_sched_barrier(0);
      consume(g + 1, bufB, scB, resB);
    }
    if (g + 1 < ngroups) {
      __builtin_amdgcn_sched_barrier(0);
      issue(g + 1, bufB, scB, resB);
      __builtin_amdgcn_sched_barrier(0);
      consume(g, bufA, scA, resA);
      consume(g + 1, bufB, scB, resB);
    } else if (g < ngroups) {
      consume(g, bufA, scA, resA);
    }
  } else {
    for (int g = 0; g < ngroups; g += 2) {
      if (g + 1 < ngroups) issue(g + 1, bufB, scB, resB);
      consume(g, bufA, scA, resA);
      if (g + 2 < ngroups) issue(g + 2, bufA, scA, resA);
      if (g + 1 < ngroups) consume(g + 1, bufB, scB, resB);
    }
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
