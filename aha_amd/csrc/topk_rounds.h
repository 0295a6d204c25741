// Exact top-k selection over register-resident candidates, shared by the sampling candidates (kernels_sample.hip) and the
// log-probability pass (kernels_logprob.hip): k rounds of (wave max, lowest index among the maxima), ordered by (value desc, index asc).
#pragma once
#include "common.h"

namespace aha {
namespace {

__device__ __forceinline__ unsigned wave_min_u32(unsigned v) {
  {
    const auto r = __builtin_amdgcn_permlane32_swap(v, v, false, false);
    v = min(r[0], r[1]);
  }
  {
    const auto r = __builtin_amdgcn_permlane16_swap(v, v, false, false);
    v = min(r[0], r[1]);
  }
  v = min(v, (unsigned)__builtin_amdgcn_update_dpp(0, v, 0x128, 0xf, 0xf, false));
  v = min(v, (unsigned)__builtin_amdgcn_update_dpp(0, v, 0x124, 0xf, 0xf, false));
  v = min(v, (unsigned)__builtin_amdgcn_update_dpp(0, v, 0x122, 0xf, 0xf, false));
  v = min(v, (unsigned)__builtin_amdgcn_update_dpp(0, v, 0x121, 0xf, 0xf, false));
  return v;
}

constexpr unsigned NO_IDX = 0xffffffffu;

// k rounds over the C candidates each lane holds in registers.  emit(r, value, index) is called by every lane with the
// wave-uniform winner of round r (index NO_IDX once the candidates are exhausted).
template <int C, typename Emit>
__device__ __forceinline__ void wave_topk_rounds(float (&v)[C], unsigned (&id)[C], int k, Emit emit) {
  for (int r = 0; r < k; ++r) {
    float lm = v[0];
    unsigned li = id[0];
#pragma unroll
    for (int j = 1; j < C; ++j) {
      const bool better = v[j] > lm || (v[j] == lm && id[j] < li);
      lm = better ? v[j] : lm;
      li = better ? id[j] : li;
    }
    const float wm = wave_max(lm);
    const unsigned wi = wave_min_u32(lm == wm ? li : NO_IDX);
    emit(r, wm, wi);
#pragma unroll
    for (int j = 0; j < C; ++j) {
      const bool hit = id[j] == wi && wi != NO_IDX;
      v[j] = hit ? -INFINITY : v[j];
      id[j] = hit ? NO_IDX : id[j];
    }
  }
}

}  // namespace
}  // namespace aha
