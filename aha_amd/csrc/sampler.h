// Host sampler of the batched sampled generation (sampler_host.hip): candle's LogitsProcessor as get_logit_processor builds it
// (reference src/models/common/sample.rs:7-38), use_repeat_penalty's slicing (sample.rs:41-60) and the RNG of sampler_rng.hip.
// The C ABI wraps it as aha_sampler; model.hip keeps one per sequence.
#pragma once
#include <stdint.h>

#include <memory>
#include <string>

#include "../../include/aha_hip.h"

namespace aha {

enum SampleKind { SAMPLE_ARGMAX, SAMPLE_ALL, SAMPLE_TOPK, SAMPLE_TOPP, SAMPLE_TOPK_TOPP };

struct RngDeleter {
  void operator()(aha_rng* r) const { aha_hip_rng_destroy(r); }
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

}  // namespace aha
