// Batched decode matvec, 33 .. 128 rows of x in one pass over the weights (kernels.h "multi-sequence decode").
//
//   gemv_rows_wide_kernel         gemv_rows_wide_body (gemv_rows_wide_body.h) with the GemvRowsBf16 weight form
//   gemv_rows_wide_mxfp8_kernel   ... with GemvRowsMxfp8
//   gemv_rows_wide_mxfp4_kernel   ... with GemvRowsMxfp4
//
// each for <CW, NRT> in {1, 2} x {4, 8}: chunks per wave from gemv_rows_plan, up to 64 or up to 128 rows.  They write the f32 slabs
// gemv_rows_kernel writes -- every partial the bits a launch of at most 32 rows gives that row (tests/test_gemv_rows_wide_gpu.py) -- so a
// call ends in the unchanged gemv_rows_merge_kernel.  gemv_rows_wide_plan is the host rule that says how many rows a pass takes.
#include "gemv_rows_wide_body.h"

namespace aha {

namespace {

template <int CW, int NRT>
__global__ __launch_bounds__(256, 2) void gemv_rows_wide_kernel(GemvRowsArgs a) {
  __shared__ __attribute__((aligned(16))) float red[4 * 2 * NRT * 256];
  gemv_rows_wide_body<GemvRowsBf16, CW, NRT>(a, a.W, nullptr, red);
}

template <int CW, int NRT>
__global__ __launch_bounds__(256, 2) void gemv_rows_wide_mxfp8_kernel(GemvRowsArgs a, const void* wq, const uint32_t* wscales) {
  __shared__ __attribute__((aligned(16))) float red[4 * 2 * NRT * 256];
  gemv_rows_wide_body<GemvRowsMxfp8, CW, NRT>(a, wq, wscales, red);
}

template <int CW, int NRT>
__global__ __launch_bounds__(256, 2) void gemv_rows_wide_mxfp4_kernel(GemvRowsArgs a, const void* wq, const uint32_t* wscales) {
  __shared__ __attribute__((aligned(16))) float red[4 * 2 * NRT * 256];
  gemv_rows_wide_body<GemvRowsMxfp4, CW, NRT>(a, wq, wscales, red);
}

// The two launches of a wide call: launch_gemv_rows_form's, with kern[CW - 1][more than 64 rows].
template <class... Extra>
void launch_wide_form(void (*const (&kern)[2][2])(GemvRowsArgs, Extra...), GemvRowsArgs a, GemvEpi epi, hipStream_t st, Extra... extra) {
  if (a.R <= 0 || a.R > GEMV_ROWS_WIDE_MAX || a.N <= 0 || a.K <= 0) return;
  a.ldws = a.N;
  int cw, nks;
  gemv_rows_plan(a.N, a.K, &cw, &nks);
  const dim3 grid((unsigned)((a.N + GR_NB - 1) / GR_NB), (unsigned)nks);
  hipLaunchKernelGGL(kern[cw - 1][a.R > 64], grid, dim3(256), 0, st, a, extra...);
  launch_gemv_rows_merge(a, epi, nks, st);
}

}  // namespace

// Rows per pass of a step of R rows over a matrix (N, K) held in `form` (0 bf16, 1 MXFP8, 2 MXFP4): 32 = groups on gemv_rows_kernel, 64 or
// 128 = gemv_rows_wide_kernel<cw, 4 | 8>.  The K-split plan is gemv_rows_plan(N, K) whatever this returns.  The rule is
// profiles/gemv_rows_wide.md's: a (matrix class, form, row bucket) is wide only where one wide pass measured below the group launches it
// replaces.
int gemv_rows_wide_plan(int N, int K, int R, int form) {
  (void)N, (void)K, (void)form;
  if (R <= 32) return 32;
  return R <= 64 ? 64 : GEMV_ROWS_WIDE_MAX;
}

void launch_gemv_rows_wide(const GemvRowsArgs& a, GemvEpi epi, hipStream_t st) {
  static constexpr void (*kern[2][2])(GemvRowsArgs) = {{gemv_rows_wide_kernel<1, 4>, gemv_rows_wide_kernel<1, 8>},
                                                       {gemv_rows_wide_kernel<2, 4>, gemv_rows_wide_kernel<2, 8>}};
  launch_wide_form(kern, a, epi, st);
}

void launch_gemv_rows_wide_mxfp8(const GemvRowsArgs& a, const void* wq, const uint32_t* wscales, GemvEpi epi, hipStream_t st) {
  static constexpr void (*kern[2][2])(GemvRowsArgs, const void*, const uint32_t*) = {
      {gemv_rows_wide_mxfp8_kernel<1, 4>, gemv_rows_wide_mxfp8_kernel<1, 8>}, {gemv_rows_wide_mxfp8_kernel<2, 4>, gemv_rows_wide_mxfp8_kernel<2, 8>}};
  launch_wide_form(kern, a, epi, st, wq, wscales);
}

void launch_gemv_rows_wide_mxfp4(const GemvRowsArgs& a, const void* wq, const uint32_t* wscales, GemvEpi epi, hipStream_t st) {
  static constexpr void (*kern[2][2])(GemvRowsArgs, const void*, const uint32_t*) = {
      {gemv_rows_wide_mxfp4_kernel<1, 4>, gemv_rows_wide_mxfp4_kernel<1, 8>}, {gemv_rows_wide_mxfp4_kernel<2, 4>, gemv_rows_wide_mxfp4_kernel<2, 8>}};
  launch_wide_form(kern, a, epi, st, wq, wscales);
}

}  // namespace aha
