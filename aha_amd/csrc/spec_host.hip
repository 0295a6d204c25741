// Draft proposer of aha_hip_generate_batch_spec (host only; mirrored by aha_amd/speculative.py, tests/test_generate_spec_cpu.py holds the
// two equal).  c = prompt || generated, n = |c|, t generated tokens, D = max_draft; the first rule with a non-empty draft wins:
//   1. aligned prediction   generated[0:t] == p[0:t]                                  -> p[t : t + D]
//   2. n-gram in p          k = ngram_max .. ngram_min, s = c[n-k:n], EARLIEST i with p[i:i+k] == s and i + k < |p|   -> p[i+k : i+k+D]
//   3. prompt lookup        the same k loop over c, LATEST i < n - k with c[i:i+k] == s -> c[i+k : min(i+k+D, n)]
// A wrong draft costs rows, never tokens: the verify step keeps only what greedy decoding confirms (model.hip spec_decode_loop).
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <string>

#include "model.h"

namespace aha {

int spec_config_check(const aha_spec_config* spec, const char* who) {
  if (!spec) {
    set_error(std::string(who) + ": null spec");
    return AHA_ERR_INVALID;
  }
  if (spec->max_draft < 0 || spec->max_draft > 15) {
    set_error(std::string(who) + ": max_draft must be in 0..15");
    return AHA_ERR_INVALID;
  }
  if (spec->ngram_min < 1 || spec->ngram_max < spec->ngram_min || spec->ngram_max > 8) {
    set_error(std::string(who) + ": n-gram bounds must satisfy 1 <= ngram_min <= ngram_max <= 8");
    return AHA_ERR_INVALID;
  }
  return AHA_OK;
}

void spec_propose(const aha_spec_config& spec, const uint32_t* c, size_t n, size_t n_prompt, const uint32_t* p, size_t np, uint32_t* out,
                  size_t* n_draft) {
  const size_t D = (size_t)spec.max_draft;
  *n_draft = 0;
  if (D == 0) return;
  auto take = [&](const uint32_t* src, size_t from, size_t end) {
    const size_t k = std::min(D, end - from);
    memcpy(out, src + from, k * sizeof(uint32_t));
    *n_draft = k;
  };
  auto same = [](const uint32_t* a, const uint32_t* b, size_t k) { return memcmp(a, b, k * sizeof(uint32_t)) == 0; };
  const size_t t = n - n_prompt;
  if (p && np > 0) {
    if (t < np && same(c + n_prompt, p, t)) return take(p, t, np);
    for (size_t k = (size_t)spec.ngram_max; k >= (size_t)spec.ngram_min; --k) {
      if (k > n || k >= np) continue;
      const uint32_t* s = c + n - k;
      for (size_t i = 0; i + k < np; ++i)
        if (same(p + i, s, k)) return take(p, i + k, np);
    }
  }
  for (size_t k = (size_t)spec.ngram_max; k >= (size_t)spec.ngram_min; --k) {
    if (k >= n) continue;
    const uint32_t* s = c + n - k;
    for (size_t i = n - k; i-- > 0;)
      if (same(c + i, s, k)) return take(c, i + k, n);
  }
}

}  // namespace aha
