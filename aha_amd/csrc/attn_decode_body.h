// Body of the fused decode attention kernel (attn_decode_fused_kernel, kernels_attn.hip).
#pragma once
#include <type_traits>
#include "attn_common.h"

namespace aha {

constexpr int ATTN_DECODE_NW = 4;  // waves (= KV units) per workgroup
// Row of the per-wave staging image of the in-block merge, in floats: O of a wave is kept [q 16][d 128 (+4)].  The MFMA fragment of a
// lane is 4 consecutive d of one q: one ds_write_b128 at q * ROW + d; ROW = 132 = 4 (mod 32) spreads the 8 lanes (8 consecutive q) of a
// store's lane group over the 32 banks.  A merge thread reads 4 consecutive d of one q, 32 threads a row: ds_read_b128, 512 contiguous
// bytes per half wave.  Both conflict-free.  (The [d][q 16] image this replaces was read with all 32 lanes of a group on ONE bank.)
constexpr int ATTN_DECODE_MO_ROW = 132;
constexpr int ATTN_DECODE_FUSED_LDS = 16 * 128 * 2 + 128 * 2 + 128 * 2 + ATTN_DECODE_NW * 16 * ATTN_DECODE_MO_ROW * 4 + 2 * ATTN_DECODE_NW * 16 * 4;  // bytes

// Sum of v[0 .. 15] in the association in which wave_sum (common.h) combines lanes 0 .. 15 of a wave whose other lanes hold zero: its two
// cross-row steps add those zeros (exact), then partners 8, 4, 2, 1 apart inside the row.  The final merge of up to 16 splits derives a
// head's sum with this in every merge thread, to the bits that wave_sum over one split per lane gives.  Contraction off: no add of
// the tree may be fused with the multiply that formed its operand.
__device__ __forceinline__ float split_sum16(const float (&v)[16]) {
#pragma clang fp contract(off)
  float t[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) t[j] = v[j] + v[j + 8];
#pragma unroll
  for (int j = 0; j < 4; ++j) t[j] = t[j] + t[j + 4];
  const float c0 = t[0] + t[2], c1 = t[1] + t[3];
  return c0 + c1;
}

// ---- decode, fused: q/k RMSNorm + (M-)RoPE + KV append + split-KV attention + in-block merge --------------------
// One launch replaces qknorm_rope_kernel + attn_decode_kernel + the combine: every block redoes the (tiny) norm/rope of
// its kv head's g query heads and of the new key in LDS (QKNormAttention::forward, modules.rs:538-557), block (kvhd, 0)
// appends the new K/V to the cache page (modules.rs:558-566), all blocks attend over the OLD tokens from the pages, unit
// 0 adds the new token from LDS, the 4 waves of a block are merged through LDS, one un-normalised partial per
// (split, head) is published, and the LAST split block of the kv head to arrive merges the splits and writes the bf16
// attention output.
//
// Latency structure (batch 1: the launch is a chain of dependent round trips, not bandwidth):
//   * every length-dependent scalar (cache length, slot, rope table of the step) arrives as a kernel ARGUMENT or from a
//     table the step's first kernel wrote -- no dependent scalar loads, no sincos, in front of the first page request;
//   * the prologue's own inputs (qkv, norm weights, rope table: L2 hits) are requested first, the unit's first page
//     right behind them (returns are in order within a wave), and the norm/rope arithmetic runs under the page fetch.
//     That needs counted waits (vmcnt >= the page's 32 loads) up to the barrier that ends the prologue, and the compiler
//     only counts what is outstanding on EVERY path: so no global load sits under a run-time condition there.  Every
//     wave requests the inputs of its first AND second prologue item (clamped to the k head), every thread a v element,
//     and every wave a page: a unit without one requests an existing page (clamped index) and skips only the compute.
//     Conditions guard LDS writes only.  (Heads beyond two rounds, g >= 8, are done behind the barrier.)
//   * in the page loop K and V of a page are separate register buffers re-requested as soon as their MFMAs have
//     consumed them (K(next) right after QK^T, V(next) right after P.V), so a wave always has 16-32 KB in flight.
// smem: ATTN_DECODE_FUSED_LDS bytes, 16-byte aligned.  Returns true in the one block per kv head that wrote the output.
// APPEND = false (draft-and-verify steps, kernels_batch.hip): the new K/V is already in its slot (kv_append_rows_kernel wrote the same
// bits before this launch) and the append below is compiled out; everything else -- the new token taken from LDS, the old ones from the
// pages, the split rule -- is the same code, so a row's output bits are those of the default instantiation.
// LINEAR = true (attn_decode_fused_kernel, the single-request decode step): the pages the launch touches are an arithmetic progression,
// page i of this layer at a.lin_page0 + i * a.lin_step (both kernel arguments, in scalar registers at wave launch): every page address,
// the append's included, is scalar arithmetic and the first K/V request has no load and no wait in front of it.  LINEAR = false: the
// addresses come from the page table (a.kv.page_ptrs), one vector load whose return the first K/V request has to wait for -- and,
// returns being in order, for every prologue input requested before it.
template <bool APPEND = true, bool LINEAR = false>
__device__ __forceinline__ bool attn_decode_fused_body(const AttnDecodeFusedArgs& a, char* smem, const int kvhd, const int split,
                                                       const int nsplit) {
  constexpr int NW = ATTN_DECODE_NW, NT = NW * 64;
  bf16_t* qs = reinterpret_cast<bf16_t*>(smem);                 // [16][128]
  bf16_t* ksn = qs + 16 * 128;                                  // [128]
  bf16_t* vsn = ksn + 128;                                      // [128]
  constexpr int MO_ROW = ATTN_DECODE_MO_ROW, MO_WAVE = 16 * MO_ROW;
  float* mo = reinterpret_cast<float*>(vsn + 128);              // per wave O [NW][q 16][MO_ROW]
  float* mm = mo + NW * MO_WAVE;                                // [NW][16]
  float* mlz = mm + NW * 16;                                    // [NW][16]
  const int tid = (int)threadIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int lane = tid & 63, G = lane >> 4, c = lane & 15;
  const int g = a.nh / a.kvh;
  const int nunits = nsplit * NW, unit = split * NW + wave;
  const int L = a.kv_len_v, slot_new = a.kv_start_v;
  const int L_old = L - 1;  // tokens already in the pages; the new one is handled from LDS
  const int npages = (L_old + KV_PAGE_TOKENS - 1) / KV_PAGE_TOKENS;

  // optional timeline (AHA_ATTN_TRACE): block (kv head 0, split 0) and (kv head 0, last split), thread 0, 100 MHz stamps:
  // start, prologue done, pages done, partial published, arrival known, end
  const int tslot = (kvhd == 0 && split == 0) ? 0 : (kvhd == 0 && split == nsplit - 1 ? 1 : -1);
  auto stamp = [&](int k) {
    if (a.trace != nullptr && tslot >= 0 && tid == 0) a.trace[tslot * 6 + k] = wall_clock64();
  };
  stamp(0);

  // ---- requests, in the order their data is needed ------------------------------------------------------------------
  const bf16_t* qkv = (const bf16_t*)a.qkv;
  // first (for most waves: only) prologue item of this wave: hs < g: q head kvhd*g+hs ; hs == g: the k head
  const bool p_is_k = wave == g;
  const bool p_have = wave <= g;
  const bf16_t* p_src = p_is_k ? qkv + (int64_t)(a.nh + kvhd) * 128 : qkv + (int64_t)(kvhd * g + min(wave, g - 1)) * 128;
  const bf16_t* p_nw = (const bf16_t*)(p_is_k ? a.k_norm_w : a.q_norm_w);
  const bf16_t px0 = p_src[lane], px1 = p_src[lane + 64];
  const bf16_t pw0 = p_nw[lane], pw1 = p_nw[lane + 64];
  const float cs = a.rope[lane], sn = a.rope[64 + lane];   // bf16-representable values (rope_step_kernel)
  // second item (g >= 4: a further q head, or the k head for wave g - 4): requested by every wave, the k head where there is none
  const int hs2 = wave + NW;
  const bool p2_is_k = hs2 >= g;
  const bf16_t* p2_src = p2_is_k ? qkv + (int64_t)(a.nh + kvhd) * 128 : qkv + (int64_t)(kvhd * g + min(hs2, g - 1)) * 128;
  const bf16_t* p2_nw = (const bf16_t*)(p2_is_k ? a.k_norm_w : a.q_norm_w);
  const bf16_t p2x0 = p2_src[lane], p2x1 = p2_src[lane + 64];
  const bf16_t p2w0 = p2_nw[lane], p2w1 = p2_nw[lane + 64];
  const bf16_t vnew = qkv[(int64_t)(a.nh + a.kvh + kvhd) * 128 + (tid & 127)];   // waves 2, 3: a second copy, not stored

  u32x4_t kf[4][4], vf[8][2];
  // Addresses: wave-uniform 64-bit base (scalar registers) + ONE 32-bit per-lane offset (lane * 16), the rest immediates:
  // pages are fragment-major (common.h), every load is `global_load_dwordx4 v, v_off, s[base] offset:frag*1024` = 1 KB
  // contiguous per wave instruction.
  typedef const __attribute__((address_space(1))) char* gchar_t;
  const uint32_t l_off = (uint32_t)lane * 16;
  auto load_k = [&](uint64_t base) {
    gchar_t kb = reinterpret_cast<gchar_t>(base + (uint64_t)kvhd * KV_PAGE_TOKENS * 256);
#pragma unroll
    for (int sub = 0; sub < 4; ++sub)
#pragma unroll
      for (int k4 = 0; k4 < 4; ++k4) {
        kf[sub][k4] = __builtin_nontemporal_load(reinterpret_cast<gptr16_t>(kb + (sub * 4 + k4) * 1024 + l_off));
        // issue order = the order QK^T consumes them (left alone, the compiler requests fragment 0 fifteenth and the first MFMA waits for
        // nearly the whole of K)
        __builtin_amdgcn_sched_barrier(0);
      }
  };
  auto load_v = [&](uint64_t base) {
    gchar_t vb = reinterpret_cast<gchar_t>(base + (uint64_t)a.kvh * KV_PAGE_TOKENS * 256 + (uint64_t)kvhd * 128 * (KV_PAGE_TOKENS * 2));
#pragma unroll
    for (int ds = 0; ds < 8; ++ds)
#pragma unroll
      for (int kk = 0; kk < 2; ++kk)
        vf[ds][kk] = __builtin_nontemporal_load(reinterpret_cast<gptr16_t>(vb + (ds * 2 + kk) * 1024 + l_off));
  };
  // This unit's page pointers (pages unit, unit + nunits, ...): ONE vector load up front, lane i holding the i-th of them,
  // broadcast per iteration with v_readlane.  (A load of page_ptrs[page] inside the loop is a VECTOR load -- the kernel also
  // stores, so the compiler will not use the scalar cache -- and its wait drains the K/V requests queued behind it.)
  uint64_t my_pages = 0;
  // Lanes beyond the unit's last page hold the pointer of an existing page (clamped index; with no old token at all, L_old = 0, that
  // is page 0, the append slot's): no load under a condition, and a unit without a page has an address it may request from.
  const int page_clamp = max(npages - 1, 0);
  auto fetch_page_ptrs = [&](int first_it) {
    if (LINEAR) return;
    const int pg = unit + (first_it + lane) * nunits;
    my_pages = (uint64_t)(a.kv.page_ptrs[min(pg, page_clamp)] + a.kv.layer_off);
  };
  auto page_base = [&](int i) {
    if (LINEAR) return a.lin_page0 + (uint64_t)((int64_t)(unit + i * nunits) * a.lin_step);
    const uint32_t lo = __builtin_amdgcn_readlane((uint32_t)my_pages, i & 63), hi = __builtin_amdgcn_readlane((uint32_t)(my_pages >> 32), i & 63);
    return ((uint64_t)hi << 32) | lo;
  };
  fetch_page_ptrs(0);
  int page = unit, it = 0;
  {
    // unconditional: a unit without a page (page >= npages) requests the clamped page and never looks at what arrives
    const uint64_t b0 = LINEAR ? a.lin_page0 + (uint64_t)((int64_t)min(unit, page_clamp) * a.lin_step) : page_base(0);
    __builtin_amdgcn_sched_barrier(0);  // K strictly ahead of V (as in the loop): the loop's counted waits assume that order
    load_k(b0);
    __builtin_amdgcn_sched_barrier(0);
    load_v(b0);
    __builtin_amdgcn_sched_barrier(0);
  }

  // ---- prologue: norm + rope of the g q heads and the k head; v raw ------------------------------------------------
  {
    auto norm_rope = [&](bf16_t bx0, bf16_t bx1, bf16_t bw0, bf16_t bw1, bf16_t* dst) {
      float x0 = bf2f(bx0), x1 = bf2f(bx1);
      const float ss = wave_sum(fmaf(x0, x0, x1 * x1));  // explicit: `a*a + b*b` can be fused two ways
      const float rinv = 1.0f / sqrtf(ss / 128.0f + a.eps);
      x0 = rbf(x0 * rinv * bf2f(bw0));
      x1 = rbf(x1 * rinv * bf2f(bw1));
      const bf16_t y0 = f2bf(rbf(x0 * cs) + rbf(-x1 * sn));
      const bf16_t y1 = f2bf(rbf(x1 * cs) + rbf(x0 * sn));
      dst[lane] = y0;
      dst[lane + 64] = y1;
    };
    if (p_have) norm_rope(px0, px1, pw0, pw1, p_is_k ? ksn : qs + wave * 128);
    if (hs2 <= g) norm_rope(p2x0, p2x1, p2w0, p2w1, p2_is_k ? ksn : qs + hs2 * 128);  // more heads than waves (g >= 4): a second round
    if (tid < 128) vsn[tid] = vnew;
    __syncthreads();
    if (g >= 2 * NW) {  // further rounds (block-uniform): loads under a condition, so behind the barrier that ends the straight-line part
      for (int hs = wave + 2 * NW; hs <= g; hs += NW) {
        const bool is_k = hs == g;
        const bf16_t* src = is_k ? qkv + (int64_t)(a.nh + kvhd) * 128 : qkv + (int64_t)(kvhd * g + hs) * 128;
        const bf16_t* nw = (const bf16_t*)(is_k ? a.k_norm_w : a.q_norm_w);
        norm_rope(src[lane], src[lane + 64], nw[lane], nw[lane + 64], is_k ? ksn : qs + hs * 128);
      }
      __syncthreads();
    }
  }
  stamp(1);
  if (APPEND && split == 0) {  // append (k roped, v raw) for the following steps
    // global address space spelled out: a flat store here would make every later wait in the kernel a vmcnt(0)
    typedef __attribute__((address_space(1))) bf16_t* gbf_t;
    const int pg = slot_new / KV_PAGE_TOKENS, t = slot_new % KV_PAGE_TOKENS;
    const uint64_t base = LINEAR ? a.lin_page0 + (uint64_t)((int64_t)pg * a.lin_step) : (uint64_t)(a.kv.page_ptrs[pg] + a.kv.layer_off);
    gbf_t kd = reinterpret_cast<gbf_t>(base) + (int64_t)kvhd * KV_PAGE_TOKENS * 128;
    gbf_t vd = reinterpret_cast<gbf_t>(base) + (int64_t)a.kvh * KV_PAGE_TOKENS * 128 + (int64_t)kvhd * 128 * KV_PAGE_TOKENS;
    for (int i = tid; i < 128; i += NT) {
      kd[kpage_elem(t, i, 4)] = ksn[i];
      vd[vpage_elem(t, i)] = vsn[i];
    }
  }

  bf16x8_t qf[4];
#pragma unroll
  for (int k4 = 0; k4 < 4; ++k4) {
    u32x4_t v = *reinterpret_cast<const u32x4_t*>(qs + min(c, g - 1) * 128 + k4 * 32 + G * 8);
    if (c >= g) v = u32x4_t{0u, 0u, 0u, 0u};
    qf[k4] = as_frag(v);
  }
  float m = -INFINITY, l = 0.f;
  f32x4_t o[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) o[i] = f32x4_t{0.f, 0.f, 0.f, 0.f};

  // One page of this unit.  MORE (compile time): the unit has another page after this one -- its K is requested right
  // after QK^T and its V right after P.V, unconditionally, so the register buffers are plain loop-carried values (a
  // run-time `if (more) load` makes them phis that the compiler resolves with copies and a vmcnt(0) at the loop end).
  auto do_page = [&](auto more_tag) {
    constexpr bool MORE = decltype(more_tag)::value;
    uint64_t nb = 0;
    if (MORE) {
      ++it;
      if ((it & 63) == 0) fetch_page_ptrs(it);  // > 64 pages per unit: next batch of pointers (contexts beyond 1 M tokens)
      nb = page_base(it);
    }
    f32x4_t st[4];
#pragma unroll
    for (int sub = 0; sub < 4; ++sub) {
      st[sub] = f32x4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int k4 = 0; k4 < 4; ++k4) st[sub] = mfma16(as_frag(kf[sub][k4]), qf[k4], st[sub]);
    }
    __builtin_amdgcn_sched_barrier(0);
    if (MORE) load_k(nb);   // K of the unit's next page: in flight during softmax + P.V of this one
    __builtin_amdgcn_sched_barrier(0);
    float alpha;
    bf16x8_t pf[2];
    const int t0 = page * KV_PAGE_TOKENS;
    softmax_tile(st, a.scale, [&](int t) { return t0 + t < L_old; }, G, m, l, alpha, pf);
#pragma unroll
    for (int ds = 0; ds < 8; ++ds) {
      o[ds] *= alpha;
#pragma unroll
      for (int kk = 0; kk < 2; ++kk) o[ds] = mfma16(as_frag(vf[ds][kk]), pf[kk], o[ds]);
    }
    __builtin_amdgcn_sched_barrier(0);
    if (MORE) load_v(nb);   // V of the next page: in flight during its QK^T and softmax
    __builtin_amdgcn_sched_barrier(0);
    page += nunits;
  };
  if (page < npages) {
    while (page + nunits < npages) do_page(std::true_type{});
    do_page(std::false_type{});
  }
  stamp(2);
  if (unit == 0) {  // the new token: score from LDS, one more online-softmax step
    // the lane's 32 q and 32 k elements (64 bytes each) as four 16-byte LDS reads, the v elements below as 8-byte ones; the products
    // are summed in element order, as before
    float dot = 0.f;
    const u32x4_t* qr = reinterpret_cast<const u32x4_t*>(qs + min(c, g - 1) * 128 + G * 32);
    const u32x4_t* kr = reinterpret_cast<const u32x4_t*>(ksn + G * 32);
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
    const float s = rbf(rbf(dot) * a.scale);
    const float m_new = fmaxf(m, s);
    const float alpha = __expf(m - m_new);
    const float p = rbf(__expf(s - m_new));  // P feeds the MFMA as bf16 on the page path: same rounding here
    l = l * alpha + (G == 0 ? __expf(s - m_new) : 0.f);
    m = m_new;
#pragma unroll
    for (int ds = 0; ds < 8; ++ds) {
      const uint2 vv = *reinterpret_cast<const uint2*>(vsn + ds * 16 + G * 4);
      o[ds][0] = fmaf(p, __uint_as_float(vv.x << 16), o[ds][0] * alpha);
      o[ds][1] = fmaf(p, __uint_as_float(vv.x & 0xffff0000u), o[ds][1] * alpha);
      o[ds][2] = fmaf(p, __uint_as_float(vv.y << 16), o[ds][2] * alpha);
      o[ds][3] = fmaf(p, __uint_as_float(vv.y & 0xffff0000u), o[ds][3] * alpha);
    }
  }
  l = group_sum(l);

  // ---- merge the 4 waves through LDS, leave one partial per (split, head) ---------------------------------------------
  {
    float* wo = mo + wave * MO_WAVE + c * MO_ROW + G * 4;
#pragma unroll
    for (int ds = 0; ds < 8; ++ds) *reinterpret_cast<f32x4_t*>(wo + ds * 16) = o[ds];
    if (G == 0) {
      mm[wave * 16 + c] = m;
      mlz[wave * 16 + c] = l;
    }
  }
  __syncthreads();
  const bool single = nsplit == 1;
  // one thread per (head, 4 dims): the published partial is ONE 16-byte write-through store per thread (a dword sc1 store is
  // one fabric write each: ~6x the time per byte of a dwordx4 one)
  const auto rsrc_w = __builtin_amdgcn_make_buffer_rsrc(a.part_o, 0, (int)((size_t)nsplit * a.nh * 128 * 4), 0x00020000);
  for (int item = tid; item < g * 32; item += NT) {
    const int q = item >> 5, d0 = (item & 31) * 4;
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
    const int head = kvhd * g + q;
    if (single) {  // the whole cache went through this block: normalise and write the attention output tensor (bf16)
      const float inv = 1.0f / ls;
      uint2 w2;
      w2.x = pack_bf(acc[0] * inv, acc[1] * inv);
      w2.y = pack_bf(acc[2] * inv, acc[3] * inv);
      *reinterpret_cast<uint2*>((bf16_t*)a.o + head * 128 + d0) = w2;
    } else {
      const u32x4_t v = {__float_as_uint(acc[0]), __float_as_uint(acc[1]), __float_as_uint(acc[2]), __float_as_uint(acc[3])};
      __builtin_amdgcn_raw_buffer_store_b128(v, rsrc_w, (uint32_t)(((size_t)split * a.nh + head) * 128 + d0) * 4, 0, 16 /* sc1 */);
      if (d0 == 0) {
        const unsigned long long mlp = ((unsigned long long)__float_as_uint(ls) << 32) | __float_as_uint(M);
        __hip_atomic_store(reinterpret_cast<unsigned long long*>(a.part_ml + ((int64_t)split * a.nh + head) * 2), mlp, __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_AGENT);
      }
    }
  }
  if (single) {
    stamp(5);
    return true;
  }
  stamp(3);

  // ---- the LAST split block of this kv head to finish merges all splits of its g heads --------------------------------
  // Partials cross blocks (possibly XCDs) inside one launch: write-through (agent-scope) stores above, every wave waits for
  // their acknowledgement, then one relaxed atomic per block on the head's counter decides who arrived last; the reader
  // uses agent-scope loads (no fence needed on either side: cdna guide G16 R1, sc1 payload both sides).
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  int* s_last = reinterpret_cast<int*>(qs);  // q fragments are in registers since the page loop; LDS region is free
  if (tid == 0) {
    const unsigned prev = __hip_atomic_fetch_add(a.head_ctr + 32 * kvhd, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    *s_last = (prev + 1u == a.ctr_target) ? 1 : 0;
  }
  __syncthreads();
  stamp(4);
  if (*s_last == 0) return false;
  // The merging block is ONE workgroup, so this phase is bound by how many load instructions it issues and by dependent round
  // trips to memory (the partials were published write-through: they are in memory, not in any L2).  Hence: 16-byte
  // write-through-coherent (sc1) buffer loads, one thread per (head, 4 dims) -- nsplit wave-loads per wave instead of
  // 4 * nsplit -- and ONE round per 16 splits: the (max, sum) pairs and the thread's first 16 partial vectors are requested together.
  if (nsplit <= 16) {
    // Up to 16 splits (at 4 pages per block: contexts up to 4 k tokens): no LDS pass.  Every merge thread (head q, 4 dims) requests its
    // head's (max, sum) pairs itself -- the 32 threads of a head ask for the same 8 bytes -- right in front of its 16 partial vectors: one round trip, as
    // on the other path, but behind it no barrier, no LDS image of the pairs and no per-head wave pass: the weights are derived in
    // registers, with the values and in the association of the other path (split_sum16), while the vectors arrive.  Both paths clamp
    // the split index of the loads beyond nsplit and give those a weight of zero.
    const auto rsrc = __builtin_amdgcn_make_buffer_rsrc(a.part_o, 0, (int)((size_t)nsplit * a.nh * 128 * 4), 0x00020000);
    const uint32_t split_stride = (uint32_t)a.nh * 128 * 4;
    for (int item = tid; item < g * 32; item += NT) {
      const int head = kvhd * g + (item >> 5);
      float2 ml[16];
#pragma unroll
      for (int j = 0; j < 16; ++j) ml[j] = act_ldf2<true>(a.part_ml + ((size_t)min(j, nsplit - 1) * a.nh + head) * 2);
      const uint32_t off = (uint32_t)(head * 128 + (item & 31) * 4) * 4;
      f32x4_t pv[16];
#pragma unroll
      for (int j = 0; j < 16; ++j) {
        const u32x4_t v = __builtin_amdgcn_raw_buffer_load_b128(rsrc, off + (uint32_t)min(j, nsplit - 1) * split_stride, 0, 16 /* sc1 */);
        pv[j] = f32x4_t{__uint_as_float(v[0]), __uint_as_float(v[1]), __uint_as_float(v[2]), __uint_as_float(v[3])};
      }
      float M = -INFINITY;
#pragma unroll
      for (int j = 0; j < 16; ++j) M = fmaxf(M, ml[j].x);  // the clamped repeats change no maximum
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
      *reinterpret_cast<uint2*>((bf16_t*)a.o + (kvhd * g) * 128 + item * 4) = w;   // attention output tensor (bf16)
    }
    stamp(5);
    return true;
  }
  // More than 16 splits: the pairs of all splits of the g heads are shared through LDS; the global max, the split weights and 1/sum are
  // derived there, one wave per head, while the first 16 vectors are in flight.
  float* w_lds = mo;               // [g][nsplit] weights  (the per-wave O^T staging area is free again)
  float* inv_lds = mo + 16 * 256;  // [g] 1 / sum
  float2* ml_lds = reinterpret_cast<float2*>(mo + 8 * 256);  // [g][nsplit] (max, sum)
  const auto rsrc = __builtin_amdgcn_make_buffer_rsrc(a.part_o, 0, (int)((size_t)nsplit * a.nh * 128 * 4), 0x00020000);
  const int nvec = g * 32;                      // (head, 4-dim group) items of this kv head
  const uint32_t split_stride = (uint32_t)a.nh * 128 * 4;
  f32x4_t pv[16];
  auto load_batch = [&](int item, int s0) {     // partial vectors of splits s0 .. s0 + 15 (clamped) for `item`
    const uint32_t off = (uint32_t)((kvhd * g + (item >> 5)) * 128 + (item & 31) * 4) * 4;
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      const u32x4_t v = __builtin_amdgcn_raw_buffer_load_b128(rsrc, off + (uint32_t)min(s0 + j, nsplit - 1) * split_stride, 0, 16 /* sc1 */);
      pv[j] = f32x4_t{__uint_as_float(v[0]), __uint_as_float(v[1]), __uint_as_float(v[2]), __uint_as_float(v[3])};
    }
  };
  {
    float2 mlv[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {   // g * nsplit <= 1024 (host check): up to 4 pairs per thread
      const int i = tid + r * NT;
      const int q = min(i / nsplit, g - 1), sidx = i - (i / nsplit) * nsplit;
      mlv[r] = act_ldf2<true>(a.part_ml + ((size_t)sidx * a.nh + kvhd * g + q) * 2);
    }
    if (tid < nvec) load_batch(tid, 0);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int i = tid + r * NT;
      if (i < g * nsplit) ml_lds[i] = mlv[r];
    }
  }
  __syncthreads();
  for (int q = wave; q < g; q += NW) {  // one wave per head
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
  for (int item = tid; item < nvec; item += NT) {
    const int q = item >> 5;
    const float* wq = w_lds + q * nsplit;
    f32x4_t f = {0.f, 0.f, 0.f, 0.f};
    for (int s0 = 0; s0 < nsplit; s0 += 16) {
      if (item != tid || s0 > 0) load_batch(item, s0);
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
    *reinterpret_cast<uint2*>((bf16_t*)a.o + (kvhd * g) * 128 + item * 4) = w;   // attention output tensor (bf16)
  }
  stamp(5);
  return true;
}

}  // namespace aha
