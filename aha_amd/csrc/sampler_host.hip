// The deterministic half of the reference's non-greedy sampler, host code: a C++ restatement of aha_amd/sampling.py
// (get_logit_processor, penalty_context, LogitsProcessor.weights_from_candidates / weights_from_logits, draw_from_candidates), which
// is its specification.  The draw is aha_hip_rng_weighted_index (sampler_rng.hip): one next_u32 per sampled token, none for ArgMax.
//
// Every probability is an f32 operation in the order candle / sampling.py perform it (f32 (x - max) * (1/T as f32), expf, / sumexp).
// Sums are sequential from 0, as candle's `iter().sum::<f32>()` and softmax loop are; sampling.py's numpy sums are pairwise, so the
// two can differ in the last bits of a sum -- enough to move a token only when a draw or a top-p threshold sits within that distance.
// Plain C++: no device code, no HIP calls.
#include <math.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <new>
#include <numeric>
#include <vector>

#include "model.h"
#include "sampler.h"

#pragma clang fp contract(off)

struct aha_sampler {
  aha::HostSampler s;
};

namespace aha {
namespace {

// LogitsProcessor::sample_topp on `prs` walked in `order`: once the running f32 sum has reached top_p the rest is zeroed (the one
// that crosses is kept).
void topp_mask(std::vector<float>& prs, const std::vector<uint32_t>& order, double top_p) {
  const float tp = (float)top_p;
  float cumsum = 0.f;
  for (uint32_t i : order) {
    if (cumsum >= tp)
      prs[i] = 0.f;
    else
      cumsum = cumsum + prs[i];
  }
}

// descending probability, equal probabilities in position order (candle's stable `sort_by`)
std::vector<uint32_t> desc_stable(const std::vector<float>& prs) {
  std::vector<uint32_t> o(prs.size());
  std::iota(o.begin(), o.end(), 0u);
  std::stable_sort(o.begin(), o.end(), [&](uint32_t a, uint32_t b) { return prs[a] > prs[b]; });
  return o;
}

float sum_f32(const float* x, size_t n) {
  float s = 0.f;
  for (size_t i = 0; i < n; ++i) s = s + x[i];
  return s;
}

// weights_from_candidates: false = the candidates do not decide (TopP nucleus wider than the list, or cut on its last entry)
bool weights_from_candidates(const HostSampler& s, const float* vals, const uint32_t* idx, int k, float mx, float sumexp,
                             std::vector<float>& w) {
  const float inv_t = (float)(1.0 / s.temperature);
  w.resize(k);
  for (int i = 0; i < k; ++i) w[i] = expf((vals[i] - mx) * inv_t) / sumexp;
  if (s.kind == SAMPLE_TOPK) return true;
  if (s.kind == SAMPLE_TOPK_TOPP) {
    const float sum_p = sum_f32(w.data(), w.size());
    if (!(s.p <= 0.0 || s.p >= (double)sum_p)) topp_mask(w, desc_stable(w), s.p);
    return true;
  }
  // SAMPLE_TOPP: the plain top-p walk breaks equal probabilities by vocabulary position
  if (sum_f32(w.data(), w.size()) < (float)s.p) return false;
  std::vector<uint32_t> o(k);
  std::iota(o.begin(), o.end(), 0u);
  std::sort(o.begin(), o.end(), [&](uint32_t a, uint32_t b) { return w[a] != w[b] ? w[a] > w[b] : idx[a] < idx[b]; });
  topp_mask(w, o, s.p);
  return !(w[k - 1] > 0.f);
}

int draw(HostSampler& s, const float* w, size_t n, uint32_t* pos) {
  const int rc = aha_hip_rng_weighted_index(s.rng.get(), w, n, pos);
  if (rc == AHA_OK) ++s.words;
  return rc;
}

// draw_from_candidates: TopK / TopKThenTopP draw in candidate order; TopP in vocabulary order (sample_multinomial over the full vector)
int draw_from_candidates(HostSampler& s, const std::vector<float>& w, const uint32_t* idx, uint32_t* token) {
  uint32_t pos = 0;
  if (s.kind != SAMPLE_TOPP) {
    if (int rc = draw(s, w.data(), w.size(), &pos)) return rc;
    *token = idx[pos];
    return AHA_OK;
  }
  std::vector<uint32_t> o(w.size());
  std::iota(o.begin(), o.end(), 0u);
  std::stable_sort(o.begin(), o.end(), [&](uint32_t a, uint32_t b) { return idx[a] < idx[b]; });
  std::vector<float> wo(w.size());
  for (size_t i = 0; i < o.size(); ++i) wo[i] = w[o[i]];
  if (int rc = draw(s, wo.data(), wo.size(), &pos)) return rc;
  *token = idx[o[pos]];
  return AHA_OK;
}

// weights_from_logits + the draw, on penalised logits
int pick_from_logits(HostSampler& s, const std::vector<float>& x0, uint32_t* token) {
  const size_t V = x0.size();
  if (s.kind == SAMPLE_ARGMAX) {   // first maximal index; no draw
    *token = (uint32_t)(std::max_element(x0.begin(), x0.end()) - x0.begin());
    return AHA_OK;
  }
  const float inv_t = (float)(1.0 / s.temperature);
  std::vector<float> prs(V);
  float mx = -INFINITY;
  for (size_t i = 0; i < V; ++i) {
    prs[i] = x0[i] * inv_t;
    mx = std::max(mx, prs[i]);
  }
  for (size_t i = 0; i < V; ++i) prs[i] = expf(prs[i] - mx);
  const float sum = sum_f32(prs.data(), V);
  for (size_t i = 0; i < V; ++i) prs[i] = prs[i] / sum;
  uint32_t pos = 0;
  const bool by_id = s.kind == SAMPLE_ALL || s.kind == SAMPLE_TOPP || (size_t)s.k >= V;
  if (by_id) {
    if (s.kind == SAMPLE_TOPK_TOPP || (s.kind == SAMPLE_TOPP && !(s.p <= 0.0 || s.p >= 1.0))) topp_mask(prs, desc_stable(prs), s.p);
    if (int rc = draw(s, prs.data(), V, &pos)) return rc;
    *token = pos;
    return AHA_OK;
  }
  // the k largest probabilities; equal probabilities: higher logit, then lower index (sampling.py's lexsort)
  std::vector<uint32_t> keep(V);
  std::iota(keep.begin(), keep.end(), 0u);
  std::partial_sort(keep.begin(), keep.begin() + s.k, keep.end(), [&](uint32_t a, uint32_t b) {
    if (prs[a] != prs[b]) return prs[a] > prs[b];
    if (x0[a] != x0[b]) return x0[a] > x0[b];
    return a < b;
  });
  keep.resize(s.k);
  std::vector<float> sub(s.k);
  for (int64_t i = 0; i < s.k; ++i) sub[i] = prs[keep[i]];
  if (s.kind == SAMPLE_TOPK_TOPP && !(s.p <= 0.0 || s.p >= (double)sum_f32(sub.data(), sub.size()))) topp_mask(sub, desc_stable(sub), s.p);
  if (int rc = draw(s, sub.data(), sub.size(), &pos)) return rc;
  *token = keep[pos];
  return AHA_OK;
}

}  // namespace

int sampling_params_check(const aha_sampling_params& p, std::string* why) {
  if (isnan(p.temperature)) return *why = "temperature is NaN", AHA_ERR_INVALID;
  if ((p.flags & AHA_SAMPLE_HAS_TOP_P) && isnan(p.top_p)) return *why = "top_p is NaN", AHA_ERR_INVALID;
  if ((p.flags & AHA_SAMPLE_HAS_TOP_K) && p.top_k < 1) return *why = "top_k must be >= 1", AHA_ERR_INVALID;
  if (p.repeat_last_n < 0) return *why = "repeat_last_n must be >= 0", AHA_ERR_INVALID;
  if (!(p.repeat_penalty > 0.f)) return *why = "repeat_penalty must be > 0", AHA_ERR_INVALID;
  return AHA_OK;
}

int logit_adjust_check(const aha_logit_adjust* a, size_t vocab_size, std::string* why) {
  if (!a) return AHA_OK;
  if (!isfinite(a->presence_penalty) || !isfinite(a->frequency_penalty)) return *why = "presence / frequency penalty must be finite", AHA_ERR_INVALID;
  if (a->n_bias > AHA_MAX_LOGIT_BIAS) return *why = "n_bias above AHA_MAX_LOGIT_BIAS", AHA_ERR_INVALID;
  if (a->n_bias && (!a->bias_ids || !a->bias_vals)) return *why = "null bias_ids / bias_vals with n_bias > 0", AHA_ERR_INVALID;
  std::vector<uint32_t> ids(a->bias_ids, a->bias_ids + a->n_bias);
  std::sort(ids.begin(), ids.end());
  if (std::adjacent_find(ids.begin(), ids.end()) != ids.end()) return *why = "duplicate bias id", AHA_ERR_INVALID;
  size_t n_ninf = 0;
  for (size_t i = 0; i < a->n_bias; ++i) {
    const float b = a->bias_vals[i];
    if (isnan(b) || b == INFINITY) return *why = "bias must be finite or -inf", AHA_ERR_INVALID;
    if (vocab_size && a->bias_ids[i] >= vocab_size) return *why = "bias id " + std::to_string(a->bias_ids[i]) + " >= vocab_size", AHA_ERR_INVALID;
    n_ninf += b == -INFINITY;
  }
  if (vocab_size && n_ninf >= vocab_size) return *why = "-inf bias on every id of the vocabulary", AHA_ERR_INVALID;
  return AHA_OK;
}

void sampler_set_adjust(HostSampler& s, const aha_logit_adjust* a) {
  LogitAdjust& A = s.adj;
  A = LogitAdjust{};
  if (!logit_adjust_active(a)) return;
  A.active = true;
  A.presence = a->presence_penalty;
  A.frequency = a->frequency_penalty;
  std::vector<uint32_t> o(a->n_bias);
  std::iota(o.begin(), o.end(), 0u);
  std::sort(o.begin(), o.end(), [&](uint32_t x, uint32_t y) { return a->bias_ids[x] < a->bias_ids[y]; });
  for (uint32_t i : o)
    if (a->bias_vals[i] != 0.f) A.bias_ids.push_back(a->bias_ids[i]), A.bias_vals.push_back(a->bias_vals[i]);
}

void sampler_adjust_sync(HostSampler& s, const uint32_t* generated, size_t n_generated, size_t vocab_size) {
  LogitAdjust& A = s.adj;
  if (!A.active) return;
  if (n_generated < A.n_counted) A.counts.clear(), A.n_counted = 0;   // an external driver started over
  for (; A.n_counted < n_generated; ++A.n_counted) {
    const uint32_t t = generated[A.n_counted];
    if (t >= vocab_size) continue;
    auto it = std::lower_bound(A.counts.begin(), A.counts.end(), std::make_pair(t, 0u));
    if (it != A.counts.end() && it->first == t) ++it->second;
    else A.counts.insert(it, std::make_pair(t, 1u));
  }
}

size_t sampler_adjust_list(const HostSampler& s, uint32_t* ids_out, float* vals_out) {
  const LogitAdjust& A = s.adj;
  if (!A.active) return 0;
  size_t n = 0, b = 0, c = 0;
  const size_t nb = A.bias_ids.size(), nc = A.counts.size();
  while (b < nb || c < nc) {
    const uint32_t ib = b < nb ? A.bias_ids[b] : 0xffffffffu, ic = c < nc ? A.counts[c].first : 0xffffffffu;
    const uint32_t id = std::min(ib, ic);
    double a = 0.0;
    if (b < nb && ib == id) a = (double)A.bias_vals[b++];
    if (c < nc && ic == id) a = a - (double)A.frequency * (double)A.counts[c++].second - (double)A.presence;
    ids_out[n] = id;
    vals_out[n++] = (float)a;
  }
  return n;
}

bool token_mask_any(const uint32_t* words, size_t vocab_size) {
  const size_t full = vocab_size / 32, rest = vocab_size % 32;
  for (size_t i = 0; i < full; ++i)
    if (words[i]) return true;
  return rest && (words[full] & ((1u << rest) - 1u));
}

int host_sampler_init(HostSampler& s, const aha_sampling_params& p) {
  std::string why;
  if (sampling_params_check(p, &why)) {
    set_error("sampling params: " + why);
    return AHA_ERR_INVALID;
  }
  aha_rng* r = nullptr;
  if (int rc = aha_hip_rng_create(p.seed, &r)) return rc;
  s.rng.reset(r);
  s.words = 0;
  s.adj = LogitAdjust{};
  s.mask = nullptr, s.mask_words = 0, s.mask_own.clear();
  // get_logit_processor (sample.rs:7-38): a temperature below 1e-7 means ArgMax whatever top_k / top_p say
  const bool has_t = !(p.temperature < 1e-7f), has_p = p.flags & AHA_SAMPLE_HAS_TOP_P, has_k = p.flags & AHA_SAMPLE_HAS_TOP_K;
  s.temperature = (double)p.temperature;
  s.p = has_p ? (double)p.top_p : 1.0;
  s.k = has_k ? p.top_k : 0;
  if (!has_t)
    s.kind = SAMPLE_ARGMAX;
  else if (!has_k)
    s.kind = has_p ? SAMPLE_TOPP : SAMPLE_ALL;
  else
    s.kind = has_p ? SAMPLE_TOPK_TOPP : SAMPLE_TOPK;
  s.repeat_penalty = p.repeat_penalty;
  s.repeat_last_n = p.repeat_last_n;
  return AHA_OK;
}

void sampler_penalty_context(const HostSampler& s, size_t n_generated, float* penalty, size_t* n_context) {
  const size_t n = (s.repeat_penalty == 1.0f || s.repeat_last_n == 0) ? 0 : std::min(n_generated, (size_t)s.repeat_last_n);
  *penalty = n ? s.repeat_penalty : 1.0f;
  *n_context = n;
}

int sampler_candidates_needed(const HostSampler& s, size_t vocab_size) {
  if (s.kind == SAMPLE_TOPK || s.kind == SAMPLE_TOPK_TOPP)
    return s.k >= 1 && s.k <= 64 && (size_t)s.k < vocab_size ? (int)s.k : 0;
  if (s.kind == SAMPLE_TOPP) return (s.p <= 0.0 || s.p >= 1.0) ? 0 : (int)std::min<size_t>(64, vocab_size);
  return 0;
}

int sampler_pick(HostSampler& s, const float* vals, const uint32_t* idx, int k, float max, float sumexp, const float* logits,
                 size_t vocab_size, const uint32_t* generated, size_t n_generated, uint32_t* token_out) {
  if (vals && idx && k >= 1) {
    if (s.kind == SAMPLE_ARGMAX) {   // arg-max of the penalised logits = the first candidate
      *token_out = idx[0];
      return AHA_OK;
    }
    const int need = sampler_candidates_needed(s, vocab_size);
    std::vector<float> w;
    if (need > 0 && k >= need && weights_from_candidates(s, vals, idx, need, max, sumexp, w))
      return draw_from_candidates(s, w, idx, token_out);
  }
  if (!logits) return AHA_SAMPLE_NEED_LOGITS;
  float pen;
  size_t n_ctx;
  sampler_penalty_context(s, n_generated, &pen, &n_ctx);
  std::vector<float> x(logits, logits + vocab_size);
  if (pen != 1.0f) {   // apply_repeat_penalty: every distinct id once, from its untouched value
    std::vector<uint32_t> ids(generated + n_generated - n_ctx, generated + n_generated);
    std::sort(ids.begin(), ids.end());
    ids.erase(std::unique(ids.begin(), ids.end()), ids.end());
    for (uint32_t t : ids)
      if (t < vocab_size) x[t] = x[t] >= 0.f ? x[t] / pen : x[t] * pen;
  }
  if (s.adj.active) {   // the addends, after the penalty: one f32 add per listed id
    sampler_adjust_sync(s, generated, n_generated, vocab_size);
    std::vector<uint32_t> ids(sampler_adjust_bound(s));
    std::vector<float> a(ids.size());
    const size_t n = sampler_adjust_list(s, ids.data(), a.data());
    for (size_t i = 0; i < n; ++i)
      if (ids[i] < vocab_size) x[ids[i]] = x[ids[i]] + a[i];
  }
  if (s.mask) {   // the allowed-token mask, after the addends: -inf on every id whose bit is clear
    if (s.mask_words != token_mask_words(vocab_size)) {
      set_error("sampler_pick: the mask has " + std::to_string(s.mask_words) + " words, a vocabulary of " + std::to_string(vocab_size) +
                " needs " + std::to_string(token_mask_words(vocab_size)));
      return AHA_ERR_INVALID;
    }
    if (!token_mask_any(s.mask, vocab_size)) {
      set_error("sampler_pick: the mask allows no id below vocab_size");
      return AHA_ERR_INVALID;
    }
    for (size_t i = 0; i < vocab_size; ++i)
      if (!((s.mask[i >> 5] >> (i & 31)) & 1u)) x[i] = -INFINITY;
  }
  return pick_from_logits(s, x, token_out);
}

}  // namespace aha

using namespace aha;

extern "C" {

int aha_hip_sampler_create(const aha_sampling_params* params, aha_sampler** out) {
  if (!params || !out) {
    set_error("sampler_create: null argument");
    return AHA_ERR_INVALID;
  }
  aha_sampler* s = new (std::nothrow) aha_sampler();
  if (!s) return AHA_ERR_OOM;
  if (int rc = host_sampler_init(s->s, *params)) {
    delete s;
    return rc;
  }
  *out = s;
  return AHA_OK;
}

void aha_hip_sampler_destroy(aha_sampler* s) { delete s; }

int aha_hip_sampler_plan(const aha_sampler* s, size_t vocab_size, size_t n_generated, int32_t* k_out, float* temperature_out,
                         float* repeat_penalty_out, size_t* n_context_out) {
  if (!s || !k_out || vocab_size == 0) {
    set_error("sampler_plan: null sampler / k_out or vocab_size 0");
    return AHA_ERR_INVALID;
  }
  float pen;
  size_t n_ctx;
  sampler_penalty_context(s->s, n_generated, &pen, &n_ctx);
  const bool argmax = s->s.kind == SAMPLE_ARGMAX;
  // an addend is live once the adjust has a non-zero bias or a token has been generated
  const bool live = s->s.adj.active && (!s->s.adj.bias_ids.empty() || n_generated > 0);
  *k_out = argmax ? (pen != 1.0f || live || s->s.mask ? 1 : 0) : sampler_candidates_needed(s->s, vocab_size);
  if (temperature_out) *temperature_out = argmax ? 0.f : (float)s->s.temperature;
  if (repeat_penalty_out) *repeat_penalty_out = pen;
  if (n_context_out) *n_context_out = n_ctx;
  return AHA_OK;
}

int aha_hip_sampler_pick(aha_sampler* s, const float* vals, const uint32_t* idx, int32_t k, float max, float sumexp, const float* logits,
                         size_t vocab_size, const uint32_t* generated, size_t n_generated, uint32_t* token_out) {
  if (!s || !token_out || vocab_size == 0 || (n_generated && !generated) || (k > 0 && (!vals || !idx))) {
    set_error("sampler_pick: bad argument");
    return AHA_ERR_INVALID;
  }
  try {
    return sampler_pick(s->s, vals, idx, k, max, sumexp, logits, vocab_size, generated, n_generated, token_out);
  } catch (const std::bad_alloc&) {
    set_error("sampler_pick: out of host memory");
    return AHA_ERR_OOM;
  }
}

int aha_hip_sampler_set_adjust(aha_sampler* s, const aha_logit_adjust* adjust) {
  if (!s) {
    set_error("sampler_set_adjust: null sampler");
    return AHA_ERR_INVALID;
  }
  try {
    std::string why;
    if (logit_adjust_check(adjust, 0, &why)) {
      set_error("sampler_set_adjust: " + why);
      return AHA_ERR_INVALID;
    }
    sampler_set_adjust(s->s, adjust);
    return AHA_OK;
  } catch (const std::bad_alloc&) {
    set_error("sampler_set_adjust: out of host memory");
    return AHA_ERR_OOM;
  }
}

int aha_hip_sampler_adjust_list(aha_sampler* s, size_t vocab_size, const uint32_t* generated, size_t n_generated, uint32_t* ids_out,
                                float* vals_out, size_t cap, size_t* n_out) {
  if (!s || !n_out || vocab_size == 0 || (n_generated && !generated)) {
    set_error("sampler_adjust_list: bad argument");
    return AHA_ERR_INVALID;
  }
  try {
    sampler_adjust_sync(s->s, generated, n_generated, vocab_size);
    const size_t bound = sampler_adjust_bound(s->s);
    std::vector<uint32_t> ids(bound);
    std::vector<float> a(bound);
    size_t n = sampler_adjust_list(s->s, ids.data(), a.data()), k = 0;
    for (size_t i = 0; i < n; ++i)   // a bias id the vocabulary does not have (set_adjust cannot know it) is dropped
      if (ids[i] < vocab_size) ids[k] = ids[i], a[k++] = a[i];
    *n_out = k;
    if (k > cap || (k && (!ids_out || !vals_out))) {
      set_error("sampler_adjust_list: room for " + std::to_string(cap) + " entries, the list has " + std::to_string(k));
      return AHA_ERR_INVALID;
    }
    if (k) memcpy(ids_out, ids.data(), k * 4), memcpy(vals_out, a.data(), k * 4);
    return AHA_OK;
  } catch (const std::bad_alloc&) {
    set_error("sampler_adjust_list: out of host memory");
    return AHA_ERR_OOM;
  }
}

int aha_hip_sampler_set_mask(aha_sampler* s, const uint32_t* words, size_t n_words) {
  if (!s || (words && n_words == 0)) {
    set_error("sampler_set_mask: null sampler, or a mask of 0 words");
    return AHA_ERR_INVALID;
  }
  try {
    if (!words) {
      s->s.mask = nullptr, s->s.mask_words = 0, s->s.mask_own.clear();
      return AHA_OK;
    }
    if (std::all_of(words, words + n_words, [](uint32_t w) { return w == 0; })) {
      set_error("sampler_set_mask: the mask allows no id");
      return AHA_ERR_INVALID;
    }
    s->s.mask_own.assign(words, words + n_words);
    s->s.mask = s->s.mask_own.data(), s->s.mask_words = n_words;
    return AHA_OK;
  } catch (const std::bad_alloc&) {
    set_error("sampler_set_mask: out of host memory");
    return AHA_ERR_OOM;
  }
}

uint64_t aha_hip_sampler_rng_words(const aha_sampler* s) { return s ? s->s.words : 0; }

}  // extern "C"
