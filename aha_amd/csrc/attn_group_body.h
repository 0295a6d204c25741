// Body of the group decode attention kernel (attn_decode_group_kernel, kernels_attn_group.hip): up to ATTN_GROUP_ROWS rows of ONE sequence
// at consecutive cache lengths -- the rows of a draft-and-verify step -- in one pass over the sequence's KV pages.
#pragma once
#include "attn_common.h"
#include "attn_decode_body.h"   // ATTN_DECODE_NW, ATTN_DECODE_MO_ROW, split_sum16

namespace aha {

// Work split.  Block (kv head, split, group), four waves = four KV units, pages unit, unit + nunits, ... with unit = split * 4 + wave and
// nunits = nsplit * 4: the single-row kernel's page-to-unit mapping for the group's (common) nsplit.  A page's K and V fragments are
// requested ONCE per wave and serve T q tiles of 16 MFMA columns.  Column c of tile tl holds head c % g of group row tl * rpt + c / g with
// rpt = 16 / g rows per tile (columns from rpt * g on stay idle: no row's heads straddle two tiles).  Where attn_decode_fused_body has one
// row in g of its 16 columns, a tile here has rpt rows in rpt * g.
//
// A row's bits are those of attn_decode_fused_body<false> on the row alone, because every step of a column is that body's step:
//   * an MFMA output column depends on its own B column only (QK^T: the q column; P.V: the p column), the softmax is per lane plus
//     group_max / group_sum over the four lanes of a column;
//   * a lane keeps m, l and the mask bound L_old of ITS column's row per tile; the pages are masked by `t0 + t < L_old`.  A page that
//     lies behind the row's L_old altogether (it exists for a later row of the group) is the body's fully masked tile: m_new = m, alpha =
//     e^0 = 1, every p = 0 -- m, l, o keep their bits -- and with m = -inf it is alpha = e^-inf = 0 on o = 0, l = 0.  So a unit without a
//     valid token for a column publishes m = -inf, l = 0, o = 0, as the single-row kernel's page-less unit does;
//   * the row's own token is taken by unit 0 behind the page loop from LDS (k normed and roped, v raw, per row), the same scalar step;
//   * the in-block merge, the published partials (at the ROW's index of part_o / part_ml) and the final merge -- the register path up to
//     16 splits, the LDS path above -- are the body's expressions per (row, head).
// Arrival: one counter per (group, kv head), the first member row's (GEN_ROW_CTRROW, GEN_ROW_CTR).  The host advances ctr_acc of every
// row by layers * nsplit (gen_write_row, model.hip); the last arriver adds nsplit to the other members' counters, which nobody reads
// inside the launch, so after every layer each row's counter stands where its own single-row launch would have left it.
//
// Request structure: the body's.  Prologue inputs first (every wave's (T * 16 + 16) / 4 norm + rope items -- the q columns, then the rows'
// k heads -- and a 16-byte piece of v per thread, all unconditional with clamped row indices), the unit's first page right behind them, the
// arithmetic under the page fetch; in the loop K(next) is requested behind the LAST tile's QK^T and V(next) behind the last tile's P.V.
// Tiles beyond the group's rows are skipped by a wave-uniform branch that holds arithmetic and LDS traffic only.
constexpr int ATTN_GROUP_T = 4;       // q tiles per workgroup
constexpr int ATTN_GROUP_ROWS = 16;   // rows of a group at most (1 + SPEC_MAX_DRAFT)

// rows one block serves for group size g = nh / kvh
__host__ __device__ constexpr int attn_group_cap(int g) { return (16 / g) * ATTN_GROUP_T < ATTN_GROUP_ROWS ? (16 / g) * ATTN_GROUP_T : ATTN_GROUP_ROWS; }

constexpr int ATTN_GROUP_LDS = ATTN_GROUP_T * 16 * 128 * 2 + 2 * ATTN_GROUP_ROWS * 128 * 2 + ATTN_DECODE_NW * 16 * ATTN_DECODE_MO_ROW * 4 +
                               2 * ATTN_DECODE_NW * 16 * 4 + ATTN_GROUP_ROWS * 4 + 16;   // bytes

template <int T>
__device__ __forceinline__ void attn_decode_group_body(const AttnDecodeBatchArgs& b, const int32_t* __restrict__ gt, int part_rows, char* smem,
                                                       const int kvhd, const int split) {
  constexpr int NW = ATTN_DECODE_NW, NT = NW * 64, NC = T * 16, RMAX = ATTN_GROUP_ROWS;
  constexpr int ROUNDS = (NC + RMAX) / NW;   // norm + rope items per wave: the q columns, then the rows' k heads
  constexpr int MO_ROW = ATTN_DECODE_MO_ROW, MO_WAVE = 16 * MO_ROW;
  bf16_t* qs = reinterpret_cast<bf16_t*>(smem);                 // [NC][128]
  bf16_t* ksn = qs + NC * 128;                                  // [RMAX][128]
  bf16_t* vsn = ksn + RMAX * 128;                               // [RMAX][128]
  float* mo = reinterpret_cast<float*>(vsn + RMAX * 128);       // per wave O of ONE tile [NW][q 16][MO_ROW]
  float* mm = mo + NW * MO_WAVE;                                // [NW][16]
  float* mlz = mm + NW * 16;                                    // [NW][16]
  int* rows_lds = reinterpret_cast<int*>(mlz + NW * 16);        // [RMAX] row index of group row j
  int* s_last = rows_lds + RMAX;
  const int tid = (int)threadIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int lane = tid & 63, G = lane >> 4, c = lane & 15;
  const int g = b.nh / b.kvh, rpt = 16 / g;

  // the group's entry: scalars of its first row, then the members' row indices and counter blocks
  const int nrows = __builtin_amdgcn_readfirstlane(gt[ATTN_GROUP_COUNT]);
  const int nsplit = __builtin_amdgcn_readfirstlane(gt[ATTN_GROUP_NSPLIT]);
  if (split >= nsplit) return;
  const int page0 = __builtin_amdgcn_readfirstlane(gt[ATTN_GROUP_PAGE0]);
  const int kv_len0 = __builtin_amdgcn_readfirstlane(gt[ATTN_GROUP_KVLEN]);
  const int nt = (nrows + rpt - 1) / rpt;   // tiles in use
  const int nunits = nsplit * NW, unit = split * NW + wave;
  const int Lold0 = kv_len0 - 1;                         // group row j: kv_len0 + j tokens after its append, Lold0 + j in the pages before it
  const int npages = (Lold0 + nrows - 1 + KV_PAGE_TOKENS - 1) / KV_PAGE_TOKENS;   // of the LAST row
  const int rowv = gt[ATTN_GROUP_ROW0 + min(c, nrows - 1)];   // lane (., c): the row index of group row c (clamped)
  auto row_of = [&](int j) { return __builtin_amdgcn_readlane(rowv, j); };   // j wave-uniform, < nrows

  // ---- requests, in the order their data is needed ------------------------------------------------------------------
  const bf16_t* qkv = (const bf16_t*)b.qkv;
  const int qkv_ld = (b.nh + 2 * b.kvh) * 128;
  bf16_t px0[ROUNDS], px1[ROUNDS];
  float pcs[ROUNDS], psn[ROUNDS];
  const bf16_t qw0 = ((const bf16_t*)b.q_norm_w)[lane], qw1 = ((const bf16_t*)b.q_norm_w)[lane + 64];
  const bf16_t kw0 = ((const bf16_t*)b.k_norm_w)[lane], kw1 = ((const bf16_t*)b.k_norm_w)[lane + 64];
  // Item `col` of a wave (wave-uniform): col < NC: q column col, else the k head of group row col - NC.  Lane i holds what q column i is
  // -- (group row, clamped) | head << 8 | in use << 16 -- so a round reads its item's with one v_readlane and the only division by g is
  // the lane's own.
  static_assert(NC <= 64, "a lane per q column");
  const int cdiv = c / g, cmod = c - cdiv * g;
  const int crow = (lane >> 4) * rpt + cdiv;
  const int cinfo = min(crow, nrows - 1) | (cmod << 8) | ((c < rpt * g && crow < nrows) ? 1 << 16 : 0);
  int item_ok[ROUNDS];
#pragma unroll
  for (int rd = 0; rd < ROUNDS; ++rd) {
    const int col = rd * NW + wave;
    int jr, head;
    if (rd * NW < NC) {
      const int info = __builtin_amdgcn_readlane(cinfo, col);
      jr = info & 0xff, head = kvhd * g + ((info >> 8) & 0xff), item_ok[rd] = info >> 16;
    } else {
      jr = min(col - NC, nrows - 1), head = b.nh + kvhd, item_ok[rd] = col - NC < nrows;
    }
    const int r = row_of(jr);
    // 32-bit per-lane offsets on the two scalar bases (attn_group_shape_ok bounds them): 2 * ROUNDS wave-uniform 64-bit addresses would
    // not fit next to what the loop keeps in scalar registers
    int xo = r * qkv_ld + head * 128 + lane, ro = r * 128 + lane;
    asm volatile("" : "+v"(xo), "+v"(ro));
    px0[rd] = qkv[xo], px1[rd] = qkv[xo + 64];
    pcs[rd] = b.rope[ro], psn[rd] = b.rope[ro + 64];
  }
  // v of group row tid / 16 (clamped), dims (tid % 16) * 8 ..: one 16-byte piece per thread
  const int vj = tid >> 4;
  const u32x4_t vnew =
      *reinterpret_cast<const u32x4_t*>(qkv + gt[ATTN_GROUP_ROW0 + min(vj, nrows - 1)] * qkv_ld + (b.nh + b.kvh + kvhd) * 128 + (tid & 15) * 8);

  u32x4_t kf[4][4], vf[8][2];
  typedef const __attribute__((address_space(1))) char* gchar_t;
  const uint32_t l_off = (uint32_t)lane * 16;
  auto load_k = [&](uint64_t base) {
    gchar_t kb = reinterpret_cast<gchar_t>(base + (uint64_t)kvhd * KV_PAGE_TOKENS * 256);
#pragma unroll
    for (int sub = 0; sub < 4; ++sub)
#pragma unroll
      for (int k4 = 0; k4 < 4; ++k4) {
        kf[sub][k4] = __builtin_nontemporal_load(reinterpret_cast<gptr16_t>(kb + (sub * 4 + k4) * 1024 + l_off));
        __builtin_amdgcn_sched_barrier(0);   // issue order = the order QK^T consumes them
      }
  };
  auto load_v = [&](uint64_t base) {
    gchar_t vb = reinterpret_cast<gchar_t>(base + (uint64_t)b.kvh * KV_PAGE_TOKENS * 256 + (uint64_t)kvhd * 128 * (KV_PAGE_TOKENS * 2));
#pragma unroll
    for (int ds = 0; ds < 8; ++ds)
#pragma unroll
      for (int kk = 0; kk < 2; ++kk)
        vf[ds][kk] = __builtin_nontemporal_load(reinterpret_cast<gptr16_t>(vb + (ds * 2 + kk) * 1024 + l_off));
  };
  // this unit's page pointers, lane i the i-th of them; beyond the last page the pointer of an existing one (clamped index)
  uint64_t my_pages = 0;
  const int page_clamp = max(npages - 1, 0);
  const uint64_t* page_ptrs = b.page_ptrs + page0;
  auto fetch_page_ptrs = [&](int first_it) {
    const int pg = unit + (first_it + lane) * nunits;
    my_pages = (uint64_t)(page_ptrs[min(pg, page_clamp)] + b.layer_off);
  };
  auto page_base = [&](int i) {
    const uint32_t lo = __builtin_amdgcn_readlane((uint32_t)my_pages, i & 63), hi = __builtin_amdgcn_readlane((uint32_t)(my_pages >> 32), i & 63);
    return ((uint64_t)hi << 32) | lo;
  };
  fetch_page_ptrs(0);
  int page = unit, it = 0;
  {
    const uint64_t b0 = page_base(0);   // unconditional: a unit without a page requests the clamped one and never looks at it
    __builtin_amdgcn_sched_barrier(0);
    load_k(b0);
    __builtin_amdgcn_sched_barrier(0);
    load_v(b0);
    __builtin_amdgcn_sched_barrier(0);
  }

  // ---- prologue: norm + rope of the rows' q heads and k heads, v raw (attn_decode_fused_body's norm_rope, expression by expression) ----
  {
    auto norm_rope = [&](bf16_t bx0, bf16_t bx1, bf16_t bw0, bf16_t bw1, float cs, float sn, bf16_t* dst) {
      float x0 = bf2f(bx0), x1 = bf2f(bx1);
      const float ss = wave_sum(fmaf(x0, x0, x1 * x1));
      const float rinv = 1.0f / sqrtf(ss / 128.0f + b.eps);
      x0 = rbf(x0 * rinv * bf2f(bw0));
      x1 = rbf(x1 * rinv * bf2f(bw1));
      const bf16_t y0 = f2bf(rbf(x0 * cs) + rbf(-x1 * sn));
      const bf16_t y1 = f2bf(rbf(x1 * cs) + rbf(x0 * sn));
      dst[lane] = y0;
      dst[lane + 64] = y1;
    };
#pragma unroll
    for (int rd = 0; rd < ROUNDS; ++rd) {
      const int col = rd * NW + wave;
      if (!item_ok[rd]) continue;   // wave-uniform; guards arithmetic and LDS writes only
      if (col < NC) norm_rope(px0[rd], px1[rd], qw0, qw1, pcs[rd], psn[rd], qs + col * 128);
      else norm_rope(px0[rd], px1[rd], kw0, kw1, pcs[rd], psn[rd], ksn + (col - NC) * 128);
    }
    if (vj < nrows) *reinterpret_cast<u32x4_t*>(vsn + vj * 128 + (tid & 15) * 8) = vnew;
    if (tid < RMAX) rows_lds[tid] = rowv;   // lanes 0 .. 15 of wave 0: c == tid
    __syncthreads();
  }

  // per tile: the lane's column -> (group row, valid), its mask bound and running (m, l)
  int Lold[T], jrow[T];
  bool cok[T];
  float m[T], l[T];
  f32x4_t o[T][8];
#pragma unroll
  for (int tl = 0; tl < T; ++tl) {
    const int j = tl * rpt + cdiv;
    cok[tl] = c < rpt * g && j < nrows;
    jrow[tl] = min(j, nrows - 1);
    Lold[tl] = cok[tl] ? Lold0 + j : 0;   // an idle column masks every token
    m[tl] = -INFINITY, l[tl] = 0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i) o[tl][i] = f32x4_t{0.f, 0.f, 0.f, 0.f};
  }

  auto do_page = [&](auto more_tag) {
    constexpr bool MORE = decltype(more_tag)::value;
    uint64_t nb = 0;
    if (MORE) {
      ++it;
      if ((it & 63) == 0) fetch_page_ptrs(it);
      nb = page_base(it);
    }
    const int t0 = page * KV_PAGE_TOKENS;
#pragma unroll
    for (int tl = 0; tl < T; ++tl) {
      f32x4_t st[4];
      if (tl < nt) {
#pragma unroll
        for (int sub = 0; sub < 4; ++sub) st[sub] = f32x4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int k4 = 0; k4 < 4; ++k4) {
          u32x4_t v = *reinterpret_cast<const u32x4_t*>(qs + (tl * 16 + c) * 128 + k4 * 32 + G * 8);
          if (!cok[tl]) v = u32x4_t{0u, 0u, 0u, 0u};
          const bf16x8_t qf = as_frag(v);
#pragma unroll
          for (int sub = 0; sub < 4; ++sub) st[sub] = mfma16(as_frag(kf[sub][k4]), qf, st[sub]);
        }
      }
      if (tl == T - 1) {
        __builtin_amdgcn_sched_barrier(0);
        if (MORE) load_k(nb);   // K of the unit's next page, behind the last tile's QK^T
        __builtin_amdgcn_sched_barrier(0);
      }
      if (tl < nt) {
        float alpha;
        bf16x8_t pf[2];
        const int Lo = Lold[tl];
        softmax_tile(st, b.scale, [&](int t) { return t0 + t < Lo; }, G, m[tl], l[tl], alpha, pf);
#pragma unroll
        for (int ds = 0; ds < 8; ++ds) {
          o[tl][ds] *= alpha;
#pragma unroll
          for (int kk = 0; kk < 2; ++kk) o[tl][ds] = mfma16(as_frag(vf[ds][kk]), pf[kk], o[tl][ds]);
        }
      }
      if (tl == T - 1) {
        __builtin_amdgcn_sched_barrier(0);
        if (MORE) load_v(nb);   // V of the next page, behind the last tile's P.V
        __builtin_amdgcn_sched_barrier(0);
      }
    }
    page += nunits;
  };
  if (page < npages) {
    while (page + nunits < npages) do_page(std::true_type{});
    do_page(std::false_type{});
  }

  // ---- every row's own token (unit 0): attn_decode_fused_body's scalar step, k / v of the column's row from LDS ----------------------
#pragma unroll
  for (int tl = 0; tl < T; ++tl) {
    if (tl >= nt) continue;
    if (unit == 0) {
      float dot = 0.f;
      const u32x4_t* qr = reinterpret_cast<const u32x4_t*>(qs + (tl * 16 + c) * 128 + G * 32);
      const u32x4_t* kr = reinterpret_cast<const u32x4_t*>(ksn + jrow[tl] * 128 + G * 32);
      u32x4_t qv[4], kv4[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        qv[j] = qr[j];
        kv4[j] = kr[j];
      }
#pragma unroll
      for (int j = 0; j < 16; ++j) {
        const uint32_t qw = qv[j >> 2][j & 3], kw = kv4[j >> 2][j & 3];
        dot = fmaf(__uint_as_float(qw << 16), __uint_as_float(kw << 16), dot);
        dot = fmaf(__uint_as_float(qw & 0xffff0000u), __uint_as_float(kw & 0xffff0000u), dot);
      }
      dot = group_sum(dot);
      const float s = rbf(rbf(dot) * b.scale);
      const float m_new = fmaxf(m[tl], s);
      const float alpha = __expf(m[tl] - m_new);
      const float p = rbf(__expf(s - m_new));
      l[tl] = l[tl] * alpha + (G == 0 ? __expf(s - m_new) : 0.f);
      m[tl] = m_new;
#pragma unroll
      for (int ds = 0; ds < 8; ++ds) {
        const uint2 vv = *reinterpret_cast<const uint2*>(vsn + jrow[tl] * 128 + ds * 16 + G * 4);
        o[tl][ds][0] = fmaf(p, __uint_as_float(vv.x << 16), o[tl][ds][0] * alpha);
        o[tl][ds][1] = fmaf(p, __uint_as_float(vv.x & 0xffff0000u), o[tl][ds][1] * alpha);
        o[tl][ds][2] = fmaf(p, __uint_as_float(vv.y << 16), o[tl][ds][2] * alpha);
        o[tl][ds][3] = fmaf(p, __uint_as_float(vv.y & 0xffff0000u), o[tl][ds][3] * alpha);
      }
    }
    l[tl] = group_sum(l[tl]);
  }

  // ---- merge the 4 waves through LDS tile after tile, one partial per (split, row, head) -----------------------------------------------
  const bool single = nsplit == 1;
  const auto rsrc_w = __builtin_amdgcn_make_buffer_rsrc(b.part_o, 0, (int)((size_t)part_rows * b.max_nsplit * b.nh * 128 * 4), 0x00020000);
  const uint32_t row_stride = (uint32_t)b.max_nsplit * b.nh * 128 * 4;   // bytes of a row's partials
#pragma unroll
  for (int tl = 0; tl < T; ++tl) {
    if (tl >= nt) continue;
    if (tl > 0) __syncthreads();   // the previous tile's merge has read the staging area
    {
      float* wo = mo + wave * MO_WAVE + c * MO_ROW + G * 4;
#pragma unroll
      for (int ds = 0; ds < 8; ++ds) *reinterpret_cast<f32x4_t*>(wo + ds * 16) = o[tl][ds];
      if (G == 0) {
        mm[wave * 16 + c] = m[tl];
        mlz[wave * 16 + c] = l[tl];
      }
    }
    __syncthreads();
    for (int item = tid; item < rpt * g * 32; item += NT) {
      const int q = item >> 5, d0 = (item & 31) * 4;
      const int j = tl * rpt + q / g;
      if (j >= nrows) continue;
      float M = -INFINITY;
#pragma unroll
      for (int w = 0; w < NW; ++w) M = fmaxf(M, mm[w * 16 + q]);
      float acc[4] = {0.f, 0.f, 0.f, 0.f}, ls = 0.f;
#pragma unroll
      for (int w = 0; w < NW; ++w) {
        const float mw = mm[w * 16 + q];
        const float wt = (mw == -INFINITY) ? 0.f : __expf(mw - M);
        const f32x4_t ov = *reinterpret_cast<const f32x4_t*>(mo + w * MO_WAVE + q * MO_ROW + d0);
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[e] = fmaf(wt, ov[e], acc[e]);
        ls = fmaf(wt, mlz[w * 16 + q], ls);
      }
      const int r = rows_lds[j], head = kvhd * g + q % g;
      if (single) {
        const float inv = 1.0f / ls;
        uint2 w2;
        w2.x = pack_bf(acc[0] * inv, acc[1] * inv);
        w2.y = pack_bf(acc[2] * inv, acc[3] * inv);
        *reinterpret_cast<uint2*>((bf16_t*)b.o + ((int64_t)r * b.nh + head) * 128 + d0) = w2;
      } else {
        const u32x4_t v = {__float_as_uint(acc[0]), __float_as_uint(acc[1]), __float_as_uint(acc[2]), __float_as_uint(acc[3])};
        __builtin_amdgcn_raw_buffer_store_b128(v, rsrc_w, (uint32_t)r * row_stride + (uint32_t)(((size_t)split * b.nh + head) * 128 + d0) * 4, 0,
                                               16 /* sc1 */);
        if (d0 == 0) {
          const unsigned long long mlp = ((unsigned long long)__float_as_uint(ls) << 32) | __float_as_uint(M);
          __hip_atomic_store(reinterpret_cast<unsigned long long*>(b.part_ml + (((int64_t)r * b.max_nsplit + split) * b.nh + head) * 2), mlp,
                             __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
      }
    }
  }
  if (single) return;

  // ---- the LAST split block of this (group, kv head) to arrive merges the splits of all its rows --------------------------------------
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (tid == 0) {
    unsigned* ctr = b.head_ctr + (int64_t)gt[ATTN_GROUP_CTRROW0] * b.kvh * 32 + 32 * kvhd;
    const unsigned prev = __hip_atomic_fetch_add(ctr, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    *s_last = (prev + 1u == (unsigned)gt[ATTN_GROUP_CTR] + (unsigned)b.ctr_step * (unsigned)nsplit) ? 1 : 0;
  }
  __syncthreads();
  if (*s_last == 0) return;
  // the other members' counters: where their own launches would have left them (nobody reads them inside this launch)
  if (tid >= 1 && tid < nrows)
    __hip_atomic_fetch_add(b.head_ctr + (int64_t)gt[ATTN_GROUP_CTRROW0 + tid] * b.kvh * 32 + 32 * kvhd, (unsigned)nsplit, __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_AGENT);
  const auto rsrc = __builtin_amdgcn_make_buffer_rsrc(b.part_o, 0, (int)((size_t)part_rows * b.max_nsplit * b.nh * 128 * 4), 0x00020000);
  const uint32_t split_stride = (uint32_t)b.nh * 128 * 4;
  const int ncols = nrows * g;   // (row, head) pairs of this kv head, column cq = j * g + hs
  if (nsplit <= 16) {
    // the 32 clamped split offsets below as vector values: hoisted as scalars they do not fit next to what this kernel keeps in scalar
    // registers (the KV8 form of attn_decode_fused_body does the same)
    int ns1 = nsplit - 1;
    asm volatile("" : "+v"(ns1));
    for (int item = tid; item < ncols * 32; item += NT) {
      const int cq = item >> 5, r = rows_lds[cq / g], head = kvhd * g + cq % g;
      const float* pml = b.part_ml + (int64_t)r * b.max_nsplit * b.nh * 2;
      float2 ml[16];
#pragma unroll
      for (int j = 0; j < 16; ++j) ml[j] = act_ldf2<true>(pml + ((size_t)min(j, ns1) * b.nh + head) * 2);
      const uint32_t off = (uint32_t)r * row_stride + (uint32_t)(head * 128 + (item & 31) * 4) * 4;
      f32x4_t pv[16];
#pragma unroll
      for (int j = 0; j < 16; ++j) {
        const u32x4_t v = __builtin_amdgcn_raw_buffer_load_b128(rsrc, off + (uint32_t)min(j, ns1) * split_stride, 0, 16 /* sc1 */);
        pv[j] = f32x4_t{__uint_as_float(v[0]), __uint_as_float(v[1]), __uint_as_float(v[2]), __uint_as_float(v[3])};
      }
      float M = -INFINITY;
#pragma unroll
      for (int j = 0; j < 16; ++j) M = fmaxf(M, ml[j].x);
      float wgt[16], wl[16];
#pragma unroll
      for (int j = 0; j < 16; ++j) {
        wgt[j] = (j < nsplit && ml[j].x != -INFINITY) ? __expf(ml[j].x - M) : 0.f;
        wl[j] = fmaf(wgt[j], ml[j].y, 0.f);
      }
      const float inv = 1.0f / split_sum16(wl);
      f32x4_t f = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int j = 0; j < 16; ++j)
#pragma unroll
        for (int e = 0; e < 4; ++e) f[e] = fmaf(wgt[j], pv[j][e], f[e]);
      uint2 w;
      w.x = pack_bf(f[0] * inv, f[1] * inv);
      w.y = pack_bf(f[2] * inv, f[3] * inv);
      *reinterpret_cast<uint2*>((bf16_t*)b.o + ((int64_t)r * b.nh + head) * 128 + (item & 31) * 4) = w;
    }
    return;
  }
  // More than 16 splits: the body's LDS path, a batch of bc columns at a time (bc * nsplit <= 1024 pairs, the body's table size)
  float* w_lds = mo;                                          // [bc][nsplit] weights
  float* inv_lds = mo + 16 * 256;                             // [bc] 1 / sum
  float2* ml_lds = reinterpret_cast<float2*>(mo + 8 * 256);   // [bc][nsplit] (max, sum)
  const int bc = min(ncols, 1024 / nsplit);
  for (int c0 = 0; c0 < ncols; c0 += bc) {
    const int nb = min(bc, ncols - c0);
    __syncthreads();   // the staging area / the previous batch's tables are free
    for (int i = tid; i < nb * nsplit; i += NT) {
      const int cq = c0 + i / nsplit, sidx = i % nsplit;
      ml_lds[i] = act_ldf2<true>(b.part_ml + (((size_t)rows_lds[cq / g] * b.max_nsplit + sidx) * b.nh + kvhd * g + cq % g) * 2);
    }
    __syncthreads();
    for (int q = wave; q < nb; q += NW) {   // one wave per (row, head)
      float M = -INFINITY;
      for (int sidx = lane; sidx < nsplit; sidx += 64) M = fmaxf(M, ml_lds[q * nsplit + sidx].x);
      M = wave_max(M);
      float ls = 0.f;
      for (int sidx = lane; sidx < nsplit; sidx += 64) {
        const float2 v = ml_lds[q * nsplit + sidx];
        const float wgt = (v.x == -INFINITY) ? 0.f : __expf(v.x - M);
        w_lds[q * nsplit + sidx] = wgt;
        ls = fmaf(wgt, v.y, ls);
      }
      ls = wave_sum(ls);
      if (lane == 0) inv_lds[q] = 1.0f / ls;
    }
    __syncthreads();
    for (int item = tid; item < nb * 32; item += NT) {
      const int q = item >> 5, cq = c0 + q, r = rows_lds[cq / g], head = kvhd * g + cq % g;
      const float* wq = w_lds + q * nsplit;
      const uint32_t off = (uint32_t)r * row_stride + (uint32_t)(head * 128 + (item & 31) * 4) * 4;
      f32x4_t f = {0.f, 0.f, 0.f, 0.f};
      for (int s0 = 0; s0 < nsplit; s0 += 16) {
        f32x4_t pv[16];
#pragma unroll
        for (int j = 0; j < 16; ++j) {
          const u32x4_t v = __builtin_amdgcn_raw_buffer_load_b128(rsrc, off + (uint32_t)min(s0 + j, nsplit - 1) * split_stride, 0, 16 /* sc1 */);
          pv[j] = f32x4_t{__uint_as_float(v[0]), __uint_as_float(v[1]), __uint_as_float(v[2]), __uint_as_float(v[3])};
        }
#pragma unroll
        for (int j = 0; j < 16; ++j) {
          const float wgt = (s0 + j < nsplit) ? wq[s0 + j] : 0.f;
#pragma unroll
          for (int e = 0; e < 4; ++e) f[e] = fmaf(wgt, pv[j][e], f[e]);
        }
      }
      const float inv = inv_lds[q];
      uint2 w;
      w.x = pack_bf(f[0] * inv, f[1] * inv);
      w.y = pack_bf(f[2] * inv, f[3] * inv);
      *reinterpret_cast<uint2*>((bf16_t*)b.o + ((int64_t)r * b.nh + head) * 128 + (item & 31) * 4) = w;
    }
  }
}

}  // namespace aha
