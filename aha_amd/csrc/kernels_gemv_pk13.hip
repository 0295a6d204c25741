// Batch-1 matvec from an exact 13-bit copy of a bf16 matrix: the single-sequence decode step reads 0.8125 of the weight bytes and
// computes the same bits.
//
// The format, per matrix.  A bf16 weight is s | E(8) | m(7): high byte s | E >> 1, low byte (E & 1) | m.  The low byte is kept verbatim.
// Of the high byte the sign is kept and E >> 1 is recoded to 4 bits with one base bh per matrix: h = 0 means E >> 1 == 0 (+-0, the bf16
// subnormals and E = 1), h = 1 .. 15 means E >> 1 == bh + h.  bh = max(E >> 1 over the finite weights) - 15 (at least 0), so the window
// runs 30 binades down from the matrix maximum.  A matrix with Inf / NaN is not packed.  A finite weight below the window (a non-zero
// E >> 1 at or below bh) gets an arbitrary code and makes its row an exception row, which the twin kernel gemv_kernel_rows_pk13 computes
// from W itself; more than PK13_MAX_EXC such rows and the matrix is not packed.  Everywhere else the recoding is invertible, so the kernel
// rebuilds exactly the f32 operands lo_bf / hi_bf give on W.
//
// Layout.  Rows in the order of W; a row is K / 4096 units; a unit (one row x 4096 columns = eight 512-column chunks, a lane owning
// k = chunk * 512 + lane * 8 .. + 7 of each as in gemv_body.h) is 6656 bytes in seven lane-linear pieces:
//   low bytes   4 x 1 KiB   piece p, lane l: 16 bytes = chunk 2p elements 0..7, chunk 2p + 1 elements 0..7
//   codes       2 x 1 KiB   piece q, lane l: 4 dwords = chunks 4q .. 4q + 3; byte i of a dword = h[element i] | h[element i + 4] << 4
//   signs       512 B       lane l: 2 dwords; dword w covers chunks 4w .. 4w + 3: bit ((c & 3) * 2 + (e >> 2)) + 8 * (e & 3) = sign of element e
// so a lane's 64 weights of a unit arrive as six full-wave 16-byte non-temporal loads and one 8-byte load, and four weights' high bytes are
// rebuilt in one dword: the codes' low or high nibbles masked to bytes, a non-zero mask, one packed multiply-add by bh, the signs shifted to
// bits 7 / 15 / 23 / 31 and ORed in; one v_perm_b32 per weight then places high and low byte on top of an f32.
//
// Plan: a work item is one unit of each row of the wave (R rows, x 2 for gate / up): 7 * R * NW loads per buffer -- R = 1 for the layer
// matrices (7, gate+up 14), R = 2 for the lm_head (14).  At most 768 persistent blocks with plan_gemv's whole-rounds rule.
#include <algorithm>

#include "gemv_pk13_body.h"
#include "kernels.h"

namespace aha {

namespace {

template <int R, int EPI, int PRO>
__global__ __launch_bounds__(GEMV_THREADS) void gemv_kernel_pk13(const void* p, const void* x, const void* norm_w, void* y, const void* residual,
                                                                 int N, int K, int bh, GemvCopyTailArgs t) {
  extern __shared__ __attribute__((aligned(16))) float xs[];  // K f32 + 8 floats reduction scratch
  GemvArgs a{};
  a.W = p; a.x = x; a.norm_w = norm_w; a.residual = residual; a.y = y;
  a.y_f32 = t.y_f32; a.blk_max = t.blk_max; a.blk_idx = t.blk_idx; a.h_out = t.h_out; a.N = N; a.K = K; a.bh = bh; a.eps = t.eps;
  gemv_pk13_body<R, EPI, PRO>(a, xs, (int)blockIdx.x, t.nblk);
}

// The twin for a matrix with exception rows: the same body with their sums from W and the row-end check compiled in (EXC).  The list is
// part of the kernel arguments, so it arrives through scalar loads of the kernarg segment with everything else the prologue reads and
// stays in SGPRs.  Its LDS has 16 more floats: the sums of the exception rows, one per list entry.
template <int R, int EPI, int PRO>
__global__ __launch_bounds__(GEMV_THREADS) void gemv_kernel_rows_pk13(const void* p, const void* x, const void* norm_w, void* y, const void* residual,
                                                                      int N, int K, int bh, GemvCopyTailArgs t, Pk13ExcRows ex) {
  extern __shared__ __attribute__((aligned(16))) float xs[];  // K f32 + 8 floats reduction scratch, PK13_MAX_EXC floats at + 16
  GemvArgs a{};
  a.W = p; a.x = x; a.norm_w = norm_w; a.residual = residual; a.y = y;
  a.y_f32 = t.y_f32; a.blk_max = t.blk_max; a.blk_idx = t.blk_idx; a.h_out = t.h_out; a.N = N; a.K = K; a.bh = bh; a.eps = t.eps;
  gemv_pk13_body<R, EPI, PRO, true>(a, xs, (int)blockIdx.x, t.nblk, ex);
}

struct GemvPk13Plan { int R, grid; };

GemvPk13Plan plan_gemv_pk13(int N, GemvEpi epi) {
  const int R = epi == GEMV_LOGITS ? 2 : 1;
  const int gmax = 768;
  const int ntiles = (N + 4 * R - 1) / (4 * R);
  const int grid = gemv_whole_rounds_grid(ntiles, gmax);   // whole rounds, as plan_gemv
  return {R, std::max(grid, 1)};
}

template <int R, int EPI>
void launch_pk13_epi(const GemvArgs& a, const GemvPk13Plan& p, const Pk13ExcRows& ex, hipStream_t st) {
  const size_t lds = (size_t)a.K * 4 + 64;
  dim3 grid(p.grid), block(GEMV_THREADS);
  const GemvCopyTailArgs t{a.y_f32, a.blk_max, a.blk_idx, a.h_out, a.eps, p.grid};
  const int pro = gemv_pro_of(a.K, a.norm_w != nullptr, true);   // always the FAST form
  if (ex.n > 0) {   // the plan is the plain kernel's
#define GV_(PP) hipLaunchKernelGGL((gemv_kernel_rows_pk13<R, EPI, PP>), grid, block, lds + PK13_MAX_EXC * 4, st, a.W, a.x, a.norm_w, a.y, a.residual, a.N, a.K, a.bh, t, ex)
    if (pro == 2) GV_(2); else if (pro == 1) GV_(1); else GV_(0);
#undef GV_
    return;
  }
#define GV_(PP) hipLaunchKernelGGL((gemv_kernel_pk13<R, EPI, PP>), grid, block, lds, st, a.W, a.x, a.norm_w, a.y, a.residual, a.N, a.K, a.bh, t)
  if (pro == 2) GV_(2); else if (pro == 1) GV_(1); else GV_(0);
#undef GV_
}

// ---- the check and the pack (once per matrix, when a model is created) ------------------------------------------------------------------
__device__ __forceinline__ int pk13_e2(uint32_t bits16) { return (bits16 >> 8) & 0x7f; }

// pass 1: max of E >> 1 over the finite weights, count of Inf / NaN
__global__ __launch_bounds__(256) void pk13_max_kernel(const u32x4_t* w, int64_t nvec, Pk13Stats* out) {
  int mx = 0;
  unsigned long long bad = 0;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < nvec; i += (int64_t)gridDim.x * 256) {
    const u32x4_t v = ld_nt16(w + i);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const uint32_t b = (v[j >> 1] >> ((j & 1) * 16)) & 0xffffu;
      if ((b & 0x7f80u) == 0x7f80u) ++bad;
      else mx = max(mx, pk13_e2(b));
    }
  }
  for (int o = 32; o > 0; o >>= 1) {
    mx = max(mx, __shfl_xor(mx, o));
    bad += __shfl_xor(bad, o);
  }
  if ((threadIdx.x & 63) == 0) {
    atomicMax(&out->max_e2, mx);
    if (bad) {
      atomicAdd(&out->bad, bad);
      atomicAdd(&out->nonfinite, bad);
    }
  }
}

// pass 2: count of finite weights below the window of pass 1's maximum, and the rows that hold one: a set of at most PK13_MAX_EXC rows
// (stored + 1, 0 = free slot), filled by compare-and-swap in the order the rows are met; a row that finds no slot sets `over`.  Such weights
// are a handful per matrix where the copy is of any use, and once the set is full a plain read of `over` ends the matter.
__global__ __launch_bounds__(256) void pk13_window_kernel(const u32x4_t* w, int64_t nvec, int K, Pk13Stats* out) {
  const int bh = pk13_base(out->max_e2);
  unsigned long long bad = 0;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < nvec; i += (int64_t)gridDim.x * 256) {
    const u32x4_t v = ld_nt16(w + i);
    bool below = false;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const uint32_t b = (v[j >> 1] >> ((j & 1) * 16)) & 0xffffu;
      const int e2 = pk13_e2(b);
      if ((b & 0x7f80u) != 0x7f80u && e2 != 0 && e2 <= bh) {
        ++bad;
        below = true;
      }
    }
    if (below && *(volatile int*)&out->over == 0) {
      const int key = (int)(i * 8 / K) + 1;      // K % 8 == 0: a vector lies in one row
      int s = 0;
      for (; s < PK13_MAX_EXC; ++s) {
        int cur = *(volatile int*)&out->row1[s];
        if (cur == 0) cur = atomicCAS(&out->row1[s], 0, key);
        if (cur == 0 || cur == key) break;
      }
      if (s == PK13_MAX_EXC) atomicExch(&out->over, 1);
    }
  }
  for (int o = 32; o > 0; o >>= 1) bad += __shfl_xor(bad, o);
  if ((threadIdx.x & 63) == 0 && bad) atomicAdd(&out->bad, bad);
}

// thread = (unit, lane): reads the lane's 8 k of the unit's eight chunks, writes its seven pieces
__global__ __launch_bounds__(256) void pk13_pack_kernel(const bf16_t* w, int64_t nunits, int bh, uint8_t* out) {
  const int lane = threadIdx.x & 63;
  const int64_t unit = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (unit >= nunits) return;
  const bf16_t* src = w + unit * PK13_UNIT_K + lane * 8;   // units of a row are consecutive: unit u starts at element u * 4096
  uint8_t* dst = out + unit * PK13_UNIT_BYTES;
  u32x4_t a[4], h[2];
  uint32_t s[2] = {0u, 0u};
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    const u32x4_t v = ld16(src + c * 512);
    uint32_t lo[2] = {0u, 0u}, hd = 0u;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const uint32_t b = (v[e >> 1] >> ((e & 1) * 16)) & 0xffffu;
      const int e2 = pk13_e2(b);
      const uint32_t code = e2 == 0 ? 0u : (uint32_t)(e2 - bh) & 15u;
      lo[e >> 2] |= (b & 0xffu) << (8 * (e & 3));
      hd |= code << (8 * (e & 3) + 4 * (e >> 2));
      s[c >> 2] |= (b >> 15) << ((c & 3) * 2 + (e >> 2) + 8 * (e & 3));
    }
    a[c >> 1][(c & 1) * 2] = lo[0];
    a[c >> 1][(c & 1) * 2 + 1] = lo[1];
    h[c >> 2][c & 3] = hd;
  }
#pragma unroll
  for (int p = 0; p < 4; ++p) *reinterpret_cast<u32x4_t*>(dst + p * 1024 + lane * 16) = a[p];
#pragma unroll
  for (int q = 0; q < 2; ++q) *reinterpret_cast<u32x4_t*>(dst + PK13_OFF_H + q * 1024 + lane * 16) = h[q];
  *reinterpret_cast<pk13_u32x2_t*>(dst + PK13_OFF_S + lane * 8) = pk13_u32x2_t{s[0], s[1]};
}

}  // namespace

size_t pk13_bytes(int N, int K) { return (size_t)N * (K / PK13_UNIT_K) * PK13_UNIT_BYTES; }

void launch_pk13_stats(const void* w, int N, int K, Pk13Stats* stats, hipStream_t st) {
  const int64_t nvec = (int64_t)N * K / 8;
  const int grid = (int)std::min<int64_t>((nvec + 255) / 256, 4096);
  hipLaunchKernelGGL(pk13_max_kernel, dim3(grid), dim3(256), 0, st, (const u32x4_t*)w, nvec, stats);
  hipLaunchKernelGGL(pk13_window_kernel, dim3(grid), dim3(256), 0, st, (const u32x4_t*)w, nvec, K, stats);
}

int pk13_exception_rows(const Pk13Stats& s, int* rows) {
  if (s.over) return PK13_MAX_EXC + 1;
  int n = 0;
  for (int i = 0; i < PK13_MAX_EXC; ++i)
    if (s.row1[i] > 0) rows[n++] = s.row1[i] - 1;
  std::sort(rows, rows + n);
  for (int i = n; i < PK13_MAX_EXC; ++i) rows[i] = -1;
  return n;
}

void launch_pk13_pack(const void* w, int N, int K, int bh, void* out, hipStream_t st) {
  const int64_t nunits = (int64_t)N * (K / PK13_UNIT_K);
  hipLaunchKernelGGL(pk13_pack_kernel, dim3((unsigned)((nunits + 3) / 4)), dim3(256), 0, st, (const bf16_t*)w, nunits, bh, (uint8_t*)out);
}

// The shapes the kernel takes: whole units, an activation vector that fits the LDS image
bool gemv_pk13_shape_ok(int N, int K) { return N >= 1 && K >= PK13_UNIT_K && K % PK13_UNIT_K == 0 && K <= 32768; }

// Which matrices the model hands to this kernel by default: those of at least 2^25 elements in whole units.  Measured per matrix on an
// MI355X, 20 alternating launches per form (scripts/bench_gemv.py FORMS=pk13; the rule: packed p90 below bf16 p10; profiles/weights_pk13.md):
// of Qwen3-8B's decode matrices gate+up (100.7 M elements: 39.0 -> 33.9 us), down_proj (50.3 M: 22.7 -> 21.2) and lm_head (622 M: 227 -> 197)
// win; qkv (25.2 M: 16.0 -> 15.9, the ranges overlap) and o_proj (16.8 M: 12.9 -> 13.7) do not -- two rounds of tiles per block, where the
// decoding of the last round is not hidden behind loads -- and stay on bf16.  Nothing between 25.2 M and 50.3 M elements was measured except
// that 2^25 itself is where the two-layer test model's gate+up sits; the line is drawn there.  N: matrix rows (gate+up: 2I).
bool gemv_pk13_by_plan(int N, int K, GemvEpi epi) {
  (void)epi;
  return gemv_pk13_shape_ok(N, K) && (int64_t)N * K >= ((int64_t)1 << 25);
}

int gemv_pk13_num_tiles(int N, int K) { (void)K; return plan_gemv_pk13(N, GEMV_LOGITS).grid; }

void debug_plan_gemv_pk13(int N, int K, GemvEpi epi, bool has_norm, int* out5) {
  const GemvPk13Plan p = plan_gemv_pk13(N, epi);
  out5[0] = p.R; out5[1] = 8; out5[2] = p.grid; out5[3] = 1; out5[4] = gemv_pro_of(K, has_norm, true);
}

void launch_gemv_pk13(const GemvArgs& g, const void* packed, int bh, const int* rows, int nrows, GemvEpi epi, hipStream_t st) {
  if (!gemv_pk13_shape_ok(g.N, g.K)) abort();   // the callers check the shape
  const int mat_rows = (epi == GEMV_SILU_MUL ? 2 : 1) * g.N;
  if (nrows < 0 || nrows > PK13_MAX_EXC || (nrows > 0 && (g.W == nullptr || rows == nullptr))) abort();
  Pk13ExcRows ex{};
  ex.W = g.W;
  ex.n = nrows;
  for (int i = 0; i < PK13_MAX_EXC; ++i) {
    ex.row[i] = i < nrows ? rows[i] : -1;
    if (i < nrows && (rows[i] < 0 || rows[i] >= mat_rows)) abort();   // the kernel reads row rows[i] of W
  }
  GemvArgs a = g;
  a.W = packed; a.bh = bh;
  const GemvPk13Plan p = plan_gemv_pk13(g.N, epi);
  switch (epi) {
    case GEMV_STORE: launch_pk13_epi<1, GEMV_STORE>(a, p, ex, st); break;
    case GEMV_RESIDUAL: launch_pk13_epi<1, GEMV_RESIDUAL>(a, p, ex, st); break;
    case GEMV_SILU_MUL: launch_pk13_epi<1, GEMV_SILU_MUL>(a, p, ex, st); break;
    case GEMV_LOGITS: launch_pk13_epi<2, GEMV_LOGITS>(a, p, ex, st); break;
    default: abort();   // GEMV_PARTIAL_F32: sharded models have no copies
  }
}

void launch_gemv_pk13(const GemvArgs& g, const void* packed, int bh, GemvEpi epi, hipStream_t st) {
  launch_gemv_pk13(g, packed, bh, nullptr, 0, epi, st);
}

}  // namespace aha
