// Qwen3-ASR host pieces (audio_tower.hip).  SURVEY.md section 8a A0-A3.
#pragma once
#include "model.h"

namespace aha {

int audio_create(aha_model* m, const aha_tensor_view* w, size_t nw);
void audio_destroy(aha_model* m);
// One audio request of a tower pass: its clip (mm: samples win over features), its ids, the row of x its ids start at; seq >= 0 names it
// in error messages.
struct AudRequest {
  const aha_mm_input* mm;
  const uint32_t* ids;
  size_t n;
  int64_t row0;
  int seq;
};
// The tower's frames per sub-pass: a request list is encoded in as many sub-passes as this cap needs, a clip never split (a longer clip is
// a sub-pass of its own).  24 000 frames = 240 s of audio; the scratch of such a pass at Qwen3-ASR-0.6B widths (480 conv channels) is
// about 2.7 GB, nearly all of it the conv stack's activations (the first conv's output alone is ~92 MB per 30 s clip).
constexpr int64_t AUD_PASS_FRAMES = 24000;
// Every check of audio_forward_requests (the tower, the clips, the placeholder counts), no device work.
int audio_check_requests(aha_model* m, const AudRequest* reqs, size_t n_reqs);
// log-mel of the sample clips -> conv stack -> encoder -> projector over every clip of the list, clip j's rows scattered into request j's
// <|audio_pad|> rows of x (row0 + position); forward_initial: one request at row 0, generate_batch_mm: the audio requests of a prefill pass
int audio_forward_requests(aha_model* m, const AudRequest* reqs, size_t n_reqs, void* x);
int64_t audio_tokens_of_frames(int64_t frames);   // get_feat_extract_output_lengths over the clip's 100-frame windows
int audio_debug_embeds(aha_model* m, float* out, size_t n);   // the last tower pass's packed audio embeddings
int logmel_standalone(const float* d_samples, const int64_t* n_samples, size_t n_clips, float* d_out, hipStream_t st);
// audio_pre.hip: resample_audio_from_vec_f32 (audio_utils.rs:590-616)
int64_t debug_resample_taps(int64_t orig, int64_t new_f, float* taps, int64_t cap, int32_t* width, int32_t* klen);
int64_t resample_output_len(int64_t length, int64_t orig_sr, int64_t target_sr);
int64_t audio_resample(aha_ctx* ctx, const float* pcm, int64_t n_frames, int channels, int orig_sr, int target_sr, float* out,
                       int64_t out_cap);

}  // namespace aha
