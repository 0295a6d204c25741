// Host sampler of the batched sampled generation (sampler_host.hip): candle's LogitsProcessor as get_logit_processor builds it
// (reference src/models/common/sample.rs:7-38), use_repeat_penalty's slicing (sample.rs:41-60) and the RNG of sampler_rng.hip.
// The C ABI wraps it as aha_sampler; model.hip keeps one per sequence.
#pragma once
#include <stdint.h>

#include <memory>
#include <string>
#include <utility>
#include <vector>

#include "../../include/aha_hip.h"

namespace aha {

enum SampleKind { SAMPLE_ARGMAX, SAMPLE_ALL, SAMPLE_TOPK, SAMPLE_TOPP, SAMPLE_TOPK_TOPP };

struct RngDeleter {
  void operator()(aha_rng* r) const { aha_hip_rng_destroy(r); }
};

// A request's aha_logit_adjust and its running state: the non-zero biases sorted by id, and the sorted (id, count) table of every
// in-vocabulary token generated so far -- one entry inserted or bumped per emitted token, never rebuilt.
struct LogitAdjust {
  bool active = false;
  float presence = 0.f, frequency = 0.f;
  std::vector<uint32_t> bias_ids;
  std::vector<float> bias_vals;
  std::vector<std::pair<uint32_t, uint32_t>> counts;
  size_t n_counted = 0;       // generated tokens already in `counts`
};

struct HostSampler {
  SampleKind kind = SAMPLE_ARGMAX;
  double temperature = 1.0;   // `temp as f64` of the request's f32
  double p = 1.0;             // `top_p as f64`
  int64_t k = 0;
  float repeat_penalty = 1.f;
  int64_t repeat_last_n = 64;
  std::unique_ptr<aha_rng, RngDeleter> rng;
  uint64_t words = 0;         // u32 handed out by rng
  LogitAdjust adj;            // host_sampler_init leaves it inactive
  // the allowed-token mask of the next pick (mask_words = ceil(V / 32) words, not owned; nullptr: none).  aha_hip_sampler_set_mask points it
  // at mask_own, batch generation and the engine at the sequence's words of the step.
  const uint32_t* mask = nullptr;
  size_t mask_words = 0;
  std::vector<uint32_t> mask_own;
};

// AHA_OK, or AHA_ERR_INVALID with *why set: NaN temperature / top_p, top_k < 1 with its flag, repeat_last_n < 0, repeat_penalty <= 0.
int sampling_params_check(const aha_sampling_params& p, std::string* why);
int host_sampler_init(HostSampler& s, const aha_sampling_params& p);
// penalty_context: the effective penalty (1 = none) and how many of the last generated ids it applies to
void sampler_penalty_context(const HostSampler& s, size_t n_generated, float* penalty, size_t* n_context);
// LogitsProcessor.candidates_needed: candidates that can decide a sampled token (0: the sampler needs the full vector)
int sampler_candidates_needed(const HostSampler& s, size_t vocab_size);
// aha_hip_sampler_pick
int sampler_pick(HostSampler& s, const float* vals, const uint32_t* idx, int k, float max, float sumexp, const float* logits,
                 size_t vocab_size, const uint32_t* generated, size_t n_generated, uint32_t* token_out);


// aha_logit_adjust: AHA_OK, or AHA_ERR_INVALID with *why set (a NaN / infinite penalty, n_bias > AHA_MAX_LOGIT_BIAS, null arrays, a
// duplicate id, a NaN / +inf bias; with vocab_size > 0 also an id >= vocab_size and -inf on every id).  a == nullptr: inactive, fine.
int logit_adjust_check(const aha_logit_adjust* a, size_t vocab_size, std::string* why);
inline bool logit_adjust_active(const aha_logit_adjust* a) {
  return a && (a->presence_penalty != 0.f || a->frequency_penalty != 0.f || a->n_bias > 0);
}
// a checked adjust (or nullptr) into the sampler: biases copied, counts emptied
void sampler_set_adjust(HostSampler& s, const aha_logit_adjust* a);
// counts brought up to generated[0 .. n_generated) (ids >= vocab_size ignored); no-op for an inactive adjust
void sampler_adjust_sync(HostSampler& s, const uint32_t* generated, size_t n_generated, size_t vocab_size);
// entries the step's addend list can have at most / the list itself, sorted by id, after sampler_adjust_sync: every id with a
// non-zero bias or a count, a_i = (float)((double)b_i - (double)frequency * c_i - (double)presence * [c_i > 0]).  Returns its length.
inline size_t sampler_adjust_bound(const HostSampler& s) { return s.adj.active ? s.adj.bias_ids.size() + s.adj.counts.size() : 0; }
size_t sampler_adjust_list(const HostSampler& s, uint32_t* ids_out, float* vals_out);


// allowed-token masks: true iff a set bit names an id < vocab_size among words[0 .. ceil(vocab_size / 32))
bool token_mask_any(const uint32_t* words, size_t vocab_size);
inline size_t token_mask_words(size_t vocab_size) { return (vocab_size + 31) / 32; }

}  // namespace aha
