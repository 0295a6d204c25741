/* aha_hip.h -- C ABI of the MI355X-native backend for aha's Qwen3 / Qwen3-VL hot path.
 *
 * The reference (jhqxxx/aha v0.2.6) has no FFI or backend trait; its only seam for this path is the Rust trait
 *   InferenceModel { forward_initial, forward_step, clear_cache, stop_token_ids }
 *     -- /root/reference/src/models/common/mod.rs:25-45
 * driven by generate_generic -- /root/reference/src/models/common/generate.rs:115-159.
 * The model-level entry points below are exactly what a Rust `impl InferenceModel for HipQwen3` would bind
 * (INTEGRATION.md shows the shim).  The op-level entry points exist for unit parity tests of each kernel against
 * the oracle; they take DEVICE pointers and a hipStream_t (passed as void*).
 *
 * Conventions: every function returns 0 on success or a negative aha_status; the message of the last error on the
 * calling thread is available from aha_hip_last_error().  The library never aborts and never throws across the ABI.
 * Handles are NOT thread-safe (same contract as the reference: `&mut self`, server holds a write lock per request,
 * /root/reference/src/server/api.rs:117).  Host buffers passed in stay owned by the caller; weights are copied to HBM.
 */
#ifndef AHA_HIP_H
#define AHA_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct aha_ctx aha_ctx;
typedef struct aha_model aha_model;

enum aha_status {
  AHA_OK = 0,
  AHA_ERR_INVALID = -1,        /* bad argument / null handle */
  AHA_ERR_HIP = -2,            /* a HIP runtime call failed */
  AHA_ERR_OOM = -3,
  AHA_ERR_SHAPE = -4,          /* tensor shape does not match the model description */
  AHA_ERR_MISSING_WEIGHT = -5, /* a tensor name the reference looks up is absent */
  AHA_ERR_UNSUPPORTED = -6,
  AHA_ERR_STATE = -7           /* e.g. seqlen_offset does not equal the current cache length */
};

enum aha_dtype { AHA_BF16 = 0, AHA_F16 = 1, AHA_F32 = 2, AHA_U32 = 3, AHA_U8 = 4 };
enum aha_arch { AHA_ARCH_QWEN3 = 0, AHA_ARCH_QWEN3VL = 1, AHA_ARCH_QWEN3ASR = 2 };

/* Mirrors Qwen3Config (/root/reference/src/models/qwen3/config.rs:4-27), Qwen3VLTextConfig / Qwen3VLVisionConfig /
 * Qwen3VLConfig (/root/reference/src/models/qwen3vl/config.rs:59-133).  Vision fields are ignored for AHA_ARCH_QWEN3. */
typedef struct aha_model_desc {
  int32_t arch;
  int32_t hidden_size, intermediate_size, num_hidden_layers;
  int32_t num_attention_heads, num_key_value_heads, head_dim, vocab_size;
  float rms_norm_eps, rope_theta;
  int32_t tie_word_embeddings;
  int32_t mrope_section[3];        /* {0,0,0} => plain 1-D RoPE (rope.rs:583-612); else interleaved M-RoPE (rope.rs:454-476) */
  /* vision tower (Qwen3VLVisionConfig) */
  int32_t vis_depth, vis_hidden_size, vis_num_heads, vis_intermediate_size, vis_in_channels, vis_patch_size,
      vis_temporal_patch_size, vis_spatial_merge_size, vis_out_hidden_size, vis_num_position_embeddings;
  int32_t vis_deepstack_indexes[8];
  int32_t vis_num_deepstack;
  /* token ids (Qwen3VLConfig) */
  int32_t image_token_id, video_token_id, vision_start_token_id, vision_end_token_id;
  /* KV-cache sizing hint (tokens).  The cache is paged and grows on demand; this only pre-reserves pages. */
  int32_t kv_reserve_tokens;
  int32_t n_stop_tokens;
  uint32_t stop_tokens[8];         /* generation_config.json eos_token_id list (qwen3/generate.rs:36-43) */
  /* audio tower (Qwen3ASRAudioConfig, /root/reference/src/models/qwen3_asr/config.rs:24-96); AHA_ARCH_QWEN3ASR only */
  int32_t aud_d_model, aud_encoder_layers, aud_attention_heads, aud_ffn_dim, aud_num_mel_bins,
      aud_downsample_hidden_size, aud_output_dim, aud_n_window;
  int32_t audio_token_id;
  /* Tensor parallelism of the decoder stack (the reference has none): rank tp_rank of tp_size holds
   * num_attention_heads/tp_size q heads, num_key_value_heads/tp_size kv heads (+ their KV cache) and
   * intermediate_size/tp_size MLP columns; o_proj / down_proj produce f32 partial sums that are all-reduced (RCCL or the
   * host callback below) before the residual add.  tp_size 0 or 1 = off.  Every rank passes the FULL checkpoint tensors. */
  int32_t tp_rank, tp_size;
  /* Compute dtype the caller asks for (the `dtype: Option<DType>` of XxxGenerateModel::init resolved by get_dtype,
   * /root/reference/src/utils/mod.rs:77-115; see aha_hip_get_dtype).  AHA_BF16 (= 0, the zero-initialised default) is the
   * only dtype the kernels compute in: f16 / f32 CHECKPOINTS are accepted and cast to bf16 at load, an f16 / f32 COMPUTE
   * request is refused by aha_hip_model_create with AHA_ERR_UNSUPPORTED instead of silently running in bf16. */
  int32_t compute_dtype;
} aha_model_desc;

/* One checkpoint tensor: HF name, pointer (host memory, e.g. an mmapped safetensors file; or, when on_device != 0,
 * device memory of the same GPU -- bf16 only), dtype, shape. */
typedef struct aha_tensor_view {
  const char* name;
  const void* data;
  int32_t dtype;
  int32_t ndim;
  int64_t shape[5];
  int32_t on_device;
} aha_tensor_view;

/* MultiModalData for Qwen3-VL (/root/reference/src/models/qwen3vl/generate.rs:79-101: data_vec =
 * [pixel_values, image_grid_thw, None, None, cache_position]).  pixel_values is the processor output
 * (N_patches, C*T*P*P) in merge-window row order (/root/reference/src/models/qwen3vl/processor.rs:174-227). */
/* (Layout history: the four video fields at the end were added in library version 0.2 -- aha_hip_version(); a caller built
 * against the 0.1 header must be recompiled, the library reads all fields.  Zero-initialise the struct and set what applies.) */
typedef struct aha_mm_input {
  const void* pixel_values;     /* host, (n_patches, patch_dim) */
  int32_t pixel_dtype;          /* AHA_BF16 or AHA_F32 */
  int64_t n_patches;
  const uint32_t* image_grid_thw; /* host, (n_images, 3) */
  int32_t n_images;
  /* Qwen3-ASR (MultiModalData = [input_features], /root/reference/src/models/qwen3_asr/generate.rs:100-125): either the
   * Whisper log-mel features (num_mel_bins, n_frames) f32, or raw 16 kHz mono samples from which the library computes
   * them on the GPU (WhisperFeatureExtractor, feature_extraction_whisper.rs:93-115).  Host pointers. */
  const float* audio_features;
  int64_t n_frames;
  const float* audio_samples;
  int64_t n_samples;
  /* Qwen3-VL, image-parallel ViT: embeddings already computed (by aha_hip_vision_encode, possibly on
   * other GPUs and all-gathered): device pointer to (1 + n_deepstack, n_image_tokens, hidden) bf16.  When set,
   * pixel_values is ignored (image_grid_thw is still needed for the M-RoPE positions). */
  const void* image_embeds;
  int64_t n_image_tokens;
  /* Qwen3-VL video input (data_vec[2..3] = pixel_values_video, video_grid_thw, /root/reference/src/models/qwen3vl/model.rs:
   * 1169-1187,1299-1307): patch rows of the sampled frames in processor order (process_videos, processor.rs:253-281) and one
   * (t, h, w) grid per video, t = temporal patches (frame pairs).  Host pointers; same dtype as pixel_values.  Frame decoding
   * and the swscale resize (get_video_data, processor.rs:447-571, ffmpeg) stay on the caller's side.  With image_embeds set,
   * the precomputed rows are the images' tokens followed by the videos' tokens. */
  const void* pixel_values_video;
  int64_t n_patches_video;
  const uint32_t* video_grid_thw; /* host, (n_videos, 3) */
  int32_t n_videos;
} aha_mm_input;

/* ---- lifecycle ---------------------------------------------------------------------------------------------- */
int aha_hip_init(int device, aha_ctx** out);
void aha_hip_shutdown(aha_ctx* ctx);
const char* aha_hip_last_error(void);
const char* aha_hip_version(void);

/* get_dtype (/root/reference/src/utils/mod.rs:77-115) as a `hip` cargo feature would extend it: an explicit request wins
 * (requested = an aha_dtype, or -1 for None); otherwise the checkpoint's config.json "torch_dtype" string decides --
 * "float32"/"float" -> AHA_F32, "float16" -> AHA_F16, "bfloat16" -> AHA_BF16 (gfx950 has native bf16: the role the
 * SM >= 8.0 test plays on the reference's cuda branch; its cpu branch maps bfloat16 to F16, mod.rs:107), anything else ->
 * AHA_F32 like the reference's `_` arm.  Host-only.  aha_hip_check_dtype says whether this library can COMPUTE in a dtype:
 * AHA_OK for AHA_BF16, AHA_ERR_UNSUPPORTED (with a message) for the others. */
int aha_hip_get_dtype(int32_t requested, const char* cfg_dtype, int32_t* out);
int aha_hip_check_dtype(int32_t dtype);

/* Replaces XxxGenerateModel::init's VarBuilder::from_mmaped_safetensors + Qwen3Model::new
 * (/root/reference/src/models/qwen3/generate.rs:22-50, qwen3/model.rs:104-134). */
int aha_hip_model_create(aha_ctx* ctx, const aha_model_desc* desc, const aha_tensor_view* weights, size_t n_weights,
                         aha_model** out);
void aha_hip_model_destroy(aha_model* m);

/* Host-only: Qwen3VLModel::get_rope_index (/root/reference/src/models/qwen3vl/model.rs:901-1133) for images: the (3, n_ids)
 * M-RoPE position rows T, H, W and rope_delta = max(position) + 1 - n_ids.  Only the token ids and vis_spatial_merge_size
 * of `desc` are read.  forward_initial runs the same code on its own input; this entry point exists so the index
 * arithmetic can be tested (and reused by a host) without a GPU. */
int aha_hip_get_rope_index(const aha_model_desc* desc, const uint32_t* input_ids, size_t n_ids, const uint32_t* image_grid_thw,
                           int32_t n_images, int32_t* pos_out, int64_t* rope_delta_out);
/* The same with videos (model.rs:908-925,973-981): every (t, h, w) video grid stands for t frames of (1, h, w), one per
 * <|vision_start|><|video_pad|> run (the processor writes a timestamp and one such run per temporal patch, processor.rs:397-426). */
int aha_hip_get_rope_index_mm(const aha_model_desc* desc, const uint32_t* input_ids, size_t n_ids, const uint32_t* image_grid_thw,
                              int32_t n_images, const uint32_t* video_grid_thw, int32_t n_videos, int32_t* pos_out,
                              int64_t* rope_delta_out);

/* ---- Qwen3-Embedding / Qwen3-Reranker ------------------------------------------------
 * == Qwen3Embedding::embed_one after tokenisation (/root/reference/src/models/qwen3_embedding/mod.rs:50-64):
 * forward_hidden(input_ids, offset 0) -> last position after the final RMSNorm -> f32 -> l2_normalize
 * (common/modules.rs:1287-1294) -> out[hidden_size]; the KV cache is cleared before and after, as the reference does.
 * Qwen3Reranker::rerank (qwen3_reranker/mod.rs:23-31) is the dot product of two such vectors
 * (cosine_similarity_no_l2, modules.rs:1381-1389) -- host arithmetic on the caller's side. */
int aha_hip_embed(aha_model* m, const uint32_t* input_ids, size_t n_ids, float* out);
/* Many texts in one call: out[j * hidden_size ..] == aha_hip_embed of sequence j, within the parity bounds (the reference embeds one
 * text at a time: qwen3_embedding/mod.rs:38-64; pooling + l2_normalize common/modules.rs:1287-1294; Qwen3Reranker::rerank
 * qwen3_reranker/mod.rs:23-31 and cosine_similarity_no_l2 modules.rs:1381-1389 are dot products of such rows).  input_ids holds the
 * n_seqs sequences back to back, seq_lens[j] tokens each.  They run as packed prefills without padding -- every sequence with positions
 * 0 .. len-1 and a cache window of its own, causal attention inside it -- in passes of at most max_tokens_per_pass tokens (0: a library
 * default of 16384; a longer sequence runs alone as one pass).  The KV cache is cleared before and after.  AHA_ARCH_QWEN3 on one GPU only:
 * a tensor- or context-parallel model gets AHA_ERR_UNSUPPORTED.  n_seqs == 0 or an empty sequence: AHA_ERR_INVALID ("empty"); an
 * id >= vocab_size: AHA_ERR_INVALID ("out of range", naming the sequence and position). */
int aha_hip_embed_batch(aha_model* m, const uint32_t* input_ids, const size_t* seq_lens, size_t n_seqs, size_t max_tokens_per_pass,
                        float* out);

/* Batched greedy generation: for each of n_seqs prompts (packed in input_ids, lengths seq_lens), what generate_generic
 * (/root/reference/src/models/common/generate.rs:115-159, which serves /v1/chat/completions one prompt at a time) yields at temperature 0
 * for that prompt alone on a cleared model.  The first token is the argmax of the prefill's last-row logits and never ends a sequence;
 * up to max_new - 1 greedy tokens follow, ending at (and keeping) the first stop token.  Row j of tokens_out (n_seqs x max_new) holds
 * n_out[j] tokens; logits_out (n_seqs x vocab f32, may be NULL) receives the logits that chose each sequence's last token (the bf16
 * Linear output read as f32).  Argmax = the first maximal index.
 * Prefill runs as packed passes of at most max_tokens_per_pass rows (0: the embed_batch default); decode advances every unfinished sequence
 * in one step per token, the weights streamed once per group of <= 32 rows.  Sequence j owns ceil((len_j + max_new) / 64) pages of the
 * cache, reserved before any work (AHA_ERR_OOM if they cannot be had); the cache is cleared before and after, on success and on error.
 * AHA_ARCH_QWEN3, text-only AHA_ARCH_QWEN3VL and text-only AHA_ARCH_QWEN3ASR (the thinker) on one GPU with head_dim 128, else
 * AHA_ERR_UNSUPPORTED.  AHA_ERR_INVALID: a null
 * pointer, n_seqs == 0, an empty prompt, max_new == 0, or an id >= vocab_size (naming the sequence and position). */
int aha_hip_generate_batch(aha_model* m, const uint32_t* input_ids, const size_t* seq_lens, size_t n_seqs, size_t max_new,
                           size_t max_tokens_per_pass, uint32_t* tokens_out, size_t* n_out, float* logits_out);

/* ---- batched sampled generation ----------------------------------------------------------------------------------------
 * aha_sampling_params: the Options of GenerationContext::new (common/generate.rs:21-53) for one sequence.
 *   temperature     < 1e-7 (negative included) = no temperature (get_logit_processor, sample.rs:13: ArgMax); NaN = AHA_ERR_INVALID
 *   top_p           read only if flags & AHA_SAMPLE_HAS_TOP_P
 *   top_k           read only if flags & AHA_SAMPLE_HAS_TOP_K; must be >= 1
 *   repeat_penalty  1.0 = off (use_repeat_penalty, sample.rs:41-60); must be > 0
 *   repeat_last_n   >= 0; 0 = off
 *   seed            StdRng::seed_from_u64(seed) (the reference's default is 299792458), one stream per sequence */
#define AHA_SAMPLE_HAS_TOP_P 1u
#define AHA_SAMPLE_HAS_TOP_K 2u
typedef struct aha_sampling_params {
  float temperature;
  float top_p;
  int32_t top_k;
  float repeat_penalty;
  int32_t repeat_last_n;
  uint32_t flags;
  uint64_t seed;
} aha_sampling_params;

/* Batched generation with per-sequence samplers: row j of tokens_out (n_seqs x max_new) holds the n_out[j] tokens generate_generic
 * (generate.rs:115-159) yields for prompt j alone with GenerationContext(params[j]), given the logits this call computes.  The first token
 * is sampled from the prefill's last row with an empty penalty context and never ends a sequence; up to max_new - 1 more follow, ending
 * at (and keeping) the first stop token.  Each sequence draws from its own RNG stream.  A sequence with no temperature and penalty 1 is
 * greedy and gives exactly aha_hip_generate_batch's tokens and logits.  step_logits_out (n_seqs x max_new x vocab f32, may be NULL):
 * entry [j, t] receives the logits before the penalty that chose token t; entries past n_out[j] are left untouched.
 * Each decode step runs the candidate step of aha_hip_sample_rows once over every row that samples, copies the candidates to the host
 * and picks there (aha_hip_sampler_pick's arithmetic); only a row whose candidates cannot decide copies its full logits row.
 * Supported models, errors, page reservation and the cache clearing are those of aha_hip_generate_batch; invalid params (null, NaN
 * temperature, top_k < 1 with its flag, repeat_last_n < 0, repeat_penalty <= 0) are AHA_ERR_INVALID before any device work. */
int aha_hip_generate_batch_sampled(aha_model* m, const uint32_t* input_ids, const size_t* seq_lens, size_t n_seqs,
                                   const aha_sampling_params* params, size_t max_new, size_t max_tokens_per_pass,
                                   uint32_t* tokens_out, size_t* n_out, float* step_logits_out);

/* ---- batched generation with images and audio ---------------------------------------------------------------------------
 * aha_hip_generate_batch / _sampled for Qwen3-VL requests with images and videos and for Qwen3-ASR requests with audio.  mm: n_seqs
 * entries, each NULL (a text request) or that request's images and / or videos, or its audio clip, with forward_initial's rules (pixel
 * values in host or device memory, bf16 or f32, grids on the host; audio samples or (128, n_frames) features in host or device memory,
 * samples winning when both are set); mm == NULL: every request is text.  params: NULL = every sequence greedy, else n_seqs samplers
 * with exactly the semantics of aha_hip_generate_batch_sampled (one RNG stream per sequence).  step_logits_out: the layout of _sampled
 * (n_seqs x max_new x vocab f32, may be NULL), for greedy sequences too: entry [j, n_out[j] - 1] of a greedy sequence is
 * aha_hip_generate_batch's logits_out.
 * Row j of tokens_out holds what generate_generic (generate.rs:115-159) yields for request j alone, on a cleared model, with its
 * MultiModalData (sampled rows: given the logits this call computes).  Per request, as Qwen3VLModel::forward / Qwen3ASRThinker::forward
 * do it for one:
 *   positions      get_rope_index of its own ids and grids at offset 0 (qwen3vl/model.rs:901-1133), a text or audio request arange;
 *   visual rows    the merged tower rows masked_scatter'ed into its <|image_pad|> then <|video_pad|> rows (model.rs:1166-1190);
 *   DeepStack      feature k added to its visual rows after decoder layer k (model.rs:806-822);
 *   audio rows     its clip's audio tower rows masked_scatter'ed into its <|audio_pad|> rows (qwen3_asr/model.rs:336-361);
 *   decode         position seqlen_offset + its own rope_delta on all three rows (model.rs:1235-1264; 0 for text and audio).
 * The prefill passes follow aha_hip_generate_batch's rule (text rows, placeholders included, up to max_tokens_per_pass; a request is
 * never split); one tower pass encodes every image and video of a prefill pass, and one audio tower pass (split in sub-passes of at
 * most 240 s of audio, a clip never split) every clip of it.  The model's own rope_delta is neither read nor left behind.
 * Errors, all before any device work (the cache stays cleared), the message naming the sequence: AHA_ERR_UNSUPPORTED for images or
 * videos on a model that is not Qwen3-VL or has no vision weights, image_embeds, or audio on a model without an audio tower;
 * AHA_ERR_SHAPE for a placeholder-count, grid or n_patches mismatch; AHA_ERR_INVALID for audio of at most 400 samples or an entry
 * without samples or features on a Qwen3-ASR model; everything else as aha_hip_generate_batch / _sampled.  Text requests give tokens
 * and logits bit-identical to aha_hip_generate_batch / _sampled. */
int aha_hip_generate_batch_mm(aha_model* m, const uint32_t* input_ids, const size_t* seq_lens, size_t n_seqs,
                              const aha_mm_input* const* mm, const aha_sampling_params* params, size_t max_new,
                              size_t max_tokens_per_pass, uint32_t* tokens_out, size_t* n_out, float* step_logits_out);

/* ---- draft-and-verify greedy generation -----------------------------------------------------------------------------------
 * aha_hip_generate_batch with up to max_draft draft tokens per sequence verified in every decode step: Predicted Outputs (the request's
 * `prediction`, /root/reference/src/params/chat.rs:105, whose usage counters accepted_prediction_tokens / rejected_prediction_tokens are
 * params/shared.rs:58-63; the reference declares them and never fills them in) plus prompt-lookup drafting.  A sequence whose cache holds
 * p tokens runs its last token and its k draft tokens as k + 1 rows of the same step, at positions p .. p + k on its own pages; the longest
 * draft prefix that equals what greedy decoding chooses is kept, with the token that follows it.  tokens_out, n_out and logits_out are
 * EXACTLY those of aha_hip_generate_batch on the same arguments -- equal, not close -- for any spec and any predictions, wrong or
 * adversarial ones included: a wrong draft costs rows of a step, never a token.  Greedy only.
 *   spec         max_draft 1..15 draft tokens per sequence per step (0: speculation off, aha_hip_generate_batch's own steps);
 *                ngram_min .. ngram_max (1 <= min <= max <= 8): the suffix lengths the n-gram rules try, longest first.
 *   predictions  NULL with prediction_lens NULL, or the sequences' predicted outputs packed like input_ids, prediction_lens[j] ids each
 *                (a length may be 0: no prediction for that sequence).
 *   drafts       per sequence and step, the first non-empty of (c = prompt || generated, n = |c|, t generated tokens, D = max_draft):
 *                1. generated[0:t] == p[0:t]: p[t : t+D];  2. for k = ngram_max .. ngram_min, s = c[n-k:n], the earliest i with
 *                p[i:i+k] == s and i + k < |p|: p[i+k : i+k+D];  3. the same k loop over c, the latest i < n - k with c[i:i+k] == s:
 *                c[i+k : min(i+k+D, n)] (aha_hip_spec_propose).  A draft is cut so that t + 1 + |draft| <= max_new.
 *   row budget   every unfinished sequence has its one row; drafts are then granted in submission order until the step's rows reach the
 *                next multiple of 32 at or above the number of unfinished sequences: speculation never adds a pass over the weights.
 *   n_proposed / n_accepted (n_seqs each, may be NULL): draft tokens run / kept per sequence (a request's accepted_prediction_tokens,
 *                and rejected = proposed - accepted);  stats (may be NULL): decode steps, rows over all steps, proposed, accepted.
 * Supported models, errors, the page reservation ceil((len + max_new) / 64) and the cache clearing are aha_hip_generate_batch's.
 * AHA_ERR_INVALID before any device work, additionally: "null spec"; "max_draft must be in 0..15"; "n-gram bounds must satisfy
 * 1 <= ngram_min <= ngram_max <= 8"; "predictions and prediction_lens must both be set or both be null"; "prediction id out of
 * range" (an id >= vocab_size, naming the sequence and position). */
typedef struct aha_spec_config {
  int32_t max_draft;  /* 1..15 draft tokens per sequence per step; 0 = speculation off */
  int32_t ngram_min;  /* >= 1 */
  int32_t ngram_max;  /* >= ngram_min, <= 8 */
} aha_spec_config;

typedef struct aha_spec_stats {
  size_t decode_steps;
  size_t rows;       /* rows run over all steps */
  size_t proposed;
  size_t accepted;
} aha_spec_stats;

int aha_hip_generate_batch_spec(aha_model* m, const uint32_t* input_ids, const size_t* seq_lens, size_t n_seqs, size_t max_new,
                                size_t max_tokens_per_pass, const aha_spec_config* spec, const uint32_t* predictions,
                                const size_t* prediction_lens, uint32_t* tokens_out, size_t* n_out, float* logits_out, size_t* n_proposed,
                                size_t* n_accepted, aha_spec_stats* stats);

/* Host only: the draft the rules above yield for one sequence -- context = prompt || generated (n_context ids, the first n_prompt of them
 * the prompt), its prediction (NULL or n_prediction == 0: none).  draft_out: room for max_draft ids; *n_draft: how many were written
 * (0: no draft, the sequence runs one row).  AHA_ERR_INVALID: a bad spec (as above), a null context / draft_out / n_draft, an empty
 * context or n_prompt > n_context. */
int aha_hip_spec_propose(const aha_spec_config* spec, const uint32_t* context, size_t n_context, size_t n_prompt,
                         const uint32_t* prediction, size_t n_prediction, uint32_t* draft_out, size_t* n_draft);

/* ---- continuous batching engine --------------------------------------------------------------------------------------------
 * A stateful server loop over the generate_batch machinery, for generate_stream_generic (/root/reference/src/models/common/generate.rs:
 * 231-368, `stream: true`): requests are submitted at any time, every step returns one event per emitted token, requests can be cancelled,
 * each has its own max_new.  While an engine exists on a model, the engine owns the KV cache: the model's single-sequence entries
 * (forward_initial, forward_step, decode_greedy, clear_cache, kv_export / kv_import, debug_graph_step), embed / embed_batch and every
 * generate_batch* entry return AHA_ERR_STATE; aha_hip_engine_destroy clears the cache.  Destroy the engine before its model:
 * aha_hip_model_destroy destroys an engine left open, and that engine's handle must not be used afterwards.  One GPU, the models and head_dim of
 * aha_hip_generate_batch (else AHA_ERR_UNSUPPORTED); no environment variable changes what it does.
 *   max_running          requests admitted at once (1 .. AHA_ENGINE_MAX_RUNNING); rows past 32 take one more weight pass per step
 *   kv_pages             64-token cache pages reserved at creation; a request holds ceil((len + max_new) / 64) of them from admission to its end
 *   max_tokens_per_step  prompt rows one step prefills (0: 16384, else >= 64)
 *   prefill_chunk        rows of one chunk of a long text prompt, a multiple of 64 within max_tokens_per_step (0: max_tokens_per_step
 *                        rounded down to 64) */
#define AHA_ENGINE_MAX_RUNNING 64
typedef struct aha_engine aha_engine;
typedef struct aha_engine_config {
  size_t max_running;
  size_t kv_pages;
  size_t max_tokens_per_step;
  size_t prefill_chunk;
} aha_engine_config;
#define AHA_ENGINE_EV_FIRST 1u      /* the request's first token (from its prefill) */
#define AHA_ENGINE_EV_STOP 2u       /* a stop token: kept, the request ended */
#define AHA_ENGINE_EV_LENGTH 4u     /* the request's max_new-th token: it ended */
#define AHA_ENGINE_EV_CANCELLED 8u  /* aha_hip_engine_cancel took effect: token is AHA_ENGINE_NO_TOKEN, the request ended */
#define AHA_ENGINE_NO_TOKEN 0xffffffffu
typedef struct aha_engine_event {
  uint64_t req_id;
  uint32_t token;
  uint32_t flags;
} aha_engine_event;
typedef struct aha_engine_stats {
  size_t waiting;      /* submitted, not admitted */
  size_t running;      /* admitted: prefilling or decoding */
  size_t free_pages;
  size_t total_pages;  /* kv_pages */
} aha_engine_stats;
/* Clears the model's cache and reserves the pages.  AHA_ERR_INVALID: a null argument or a bad config (checked first, before the model is
 * looked at); AHA_ERR_STATE: the model already has an engine; AHA_ERR_OOM: the pages or buffers cannot be had. */
int aha_hip_engine_create(aha_model* m, const aha_engine_config* cfg, aha_engine** out);
void aha_hip_engine_destroy(aha_engine* e);
/* Queues one request (generate_generic's input for one prompt: ids, its MultiModalData, GenerationContext's options, max_tokens).
 * mm: NULL or the request's images / videos or audio clip, with aha_hip_generate_batch_mm's rules; the struct and what it points to stay the
 * caller's and must stay valid until the request's first-token (or cancelled) event.  params: NULL = greedy, else the sampler with the
 * semantics of aha_hip_generate_batch_sampled (its own RNG stream).  Every check happens here, before any device work, with
 * aha_hip_generate_batch_mm's codes and messages; a request that needs more than kv_pages pages is AHA_ERR_OOM.  *req_id: 1, 2, ... */
int aha_hip_engine_submit(aha_engine* e, const uint32_t* input_ids, size_t n_ids, const aha_mm_input* mm, const aha_sampling_params* params,
                          size_t max_new, uint64_t* req_id);
/* A waiting or running request ends at the next step with a CANCELLED event and gives its pages back; AHA_ERR_INVALID for an id that is
 * neither (unknown or already ended). */
int aha_hip_engine_cancel(aha_engine* e, uint64_t req_id);
/* One step.  Cancellations first; then the prefill pass: at most one prefill_chunk-row chunk of the long text prompt part-way through its
 * prefill, and waiting requests admitted in submission order while a slot and their pages are free and their prompt fits in what is left of
 * max_tokens_per_step.  Only a text prompt longer than max_tokens_per_step is chunked (when no other chunked prefill runs); a shorter
 * one that does not fit waits for the next step, so it is always prefilled whole; a request with images, video or audio is prefilled
 * whole, never chunked, alone if it is over the budget.  The prompts it completes give their first token (FIRST).  Then one
 * decode step over every request that had its first token before this step (generate_generic's loop: greedy argmax or the request's sampler,
 * stop tokens kept, STOP / LENGTH end it).  ev (cap >= max_running + pending cancellations, else AHA_ERR_INVALID): cancellations, first
 * tokens in pass order, decode tokens in submission order; *n_ev of them.  logits_out (NULL or cap x vocab f32, as the count is known only
 * afterwards): row i = the logits that chose event i's token (a cancellation's row is not written).  A request prefilled whole has the
 * tokens and logits of aha_hip_generate_batch_mm (or _sampled) for the same prefill pass composition, bit for bit; a chunked prompt's
 * equal its whole prefill within the parity bounds only.  A step that fails (a HIP or allocation error) loses its events: destroy the
 * engine then.
 * With requests of aha_hip_engine_submit_spec (below) waiting or running, cap >= aha_hip_engine_max_events(e), and: a request may emit up
 * to 1 + max_draft token events in one step; its events of one step are consecutive and in generation order, at the place its single event
 * has otherwise, among the decode tokens in submission order; STOP / LENGTH can only be on the last of them, and tokens behind a stop token
 * inside an accepted run are dropped; logits_out row i is still the logits that chose event i's token -- for a drafted token the verify
 * row that confirmed it.  Everything above stays true for an engine without such requests. */
int aha_hip_engine_step(aha_engine* e, aha_engine_event* ev, size_t cap, size_t* n_ev, float* logits_out);
int aha_hip_engine_stats(const aha_engine* e, aha_engine_stats* out);
/* Test hook: the value a slot's split-arrival counters are reset to when a request takes it (default 0; near 2^32 they wrap mid-request).
 * The counter blocks of a step's draft rows (aha_hip_engine_submit_spec) are set to it at the next step that drafts. */
int aha_hip_engine_debug_ctr_base(aha_engine* e, uint32_t base);

/* ---- draft-and-verify requests in the engine ---------------------------------------------------------------------------------
 * aha_hip_generate_batch_spec's decoding for streamed requests: where the request's `prediction` (src/params/chat.rs:105 of the reference)
 * arrives when `stream: true` (generate_stream_generic, models/common/generate.rs:231-368).  A request submitted here is greedy and may
 * run up to max_draft draft tokens as rows of its own in every decode step; its tokens, flags and logits are EXACTLY those of the same
 * request through aha_hip_engine_submit on the same submission history, for any prediction, and every other request of the engine keeps
 * its bits.  An engine without such a request launches and computes what it did before they existed.
 *   spec, prediction   aha_hip_generate_batch_spec's rules for one sequence: the drafts are aha_hip_spec_propose's over prompt || generated;
 *                      the prediction is copied at submit; NULL / 0: prompt lookup only; max_draft 0: an ordinary greedy request.
 *   scheduler          in the decode step of aha_hip_engine_step the R requests that decode have their one row each, in submission order;
 *                      extra = row_budget(R) - R, row_budget(n) the next multiple of 32 at or above n; drafts are then granted in
 *                      submission order among the requests of this entry: k = min(|propose(...)|, extra, max_new - t - 1) for a request
 *                      with t tokens so far, extra -= k -- aha_hip_generate_batch_spec's rule, with the same cut that keeps the cache
 *                      inside the request's reserved pages.  Speculation never adds a pass over the weights.  A step whose prefill gave F
 *                      first tokens grants at most row_budget(max_running) - F - R draft rows, so that the step's events fit the cap (no
 *                      cut when F = 0).  A step in which no row drafts is the step it was before: one attention launch per layer with the
 *                      fused append.  Draft rows sit behind the R mandatory rows, request by request.
 *   counters           a draft token is accepted when the verify step's greedy choice equals it; proposed = draft rows run.
 * Out of scope: samplers, logprobs (an event of such a request has n_top = -1 in aha_hip_engine_step_logprobs), logit adjustments and masks
 * on these requests (aha_hip_engine_set_mask refuses their ids with AHA_ERR_INVALID); tensor-parallel and context-parallel models (as the engine).
 * Errors, all before any device work: aha_hip_engine_submit's codes and messages, plus AHA_ERR_INVALID "null spec"; "max_draft must be in
 * 0..15"; "n-gram bounds must satisfy 1 <= ngram_min <= ngram_max <= 8"; "prediction id out of range" (an id >= vocab_size, naming its
 * position).  A request with mm is allowed, as in aha_hip_generate_batch_spec. */
int aha_hip_engine_submit_spec(aha_engine* e, const uint32_t* input_ids, size_t n_ids, const aha_mm_input* mm, size_t max_new,
                               const aha_spec_config* spec, const uint32_t* prediction, size_t n_prediction, uint64_t* req_id);
/* The cap the next aha_hip_engine_step* call needs, pending cancellations included: max_running + pending cancellations while no request
 * submitted with max_draft > 0 is waiting or running (what aha_hip_engine_step has always demanded), else row_budget(max_running) + pending
 * cancellations.  0 for a null engine. */
size_t aha_hip_engine_max_events(const aha_engine* e);
/* aha_spec_stats over the engine's life: its decode steps (those of requests that never draft included), their rows, the draft tokens
 * proposed and accepted. */
int aha_hip_engine_spec_stats(const aha_engine* e, aha_spec_stats* out);
/* The draft tokens run / kept for one request (a response's accepted_prediction_tokens, params/shared.rs:58-63; rejected = proposed -
 * accepted): for a running request, and for one that ended in the most recent step -- the engine keeps the counts of the requests a step
 * retired until the next step begins.  Any other id: AHA_ERR_INVALID. */
int aha_hip_engine_request_spec(const aha_engine* e, uint64_t req_id, size_t* n_proposed, size_t* n_accepted);

/* ---- per-token log-probabilities -----------------------------------------------------------------------------------------
 * The chat request's `logprobs` / `top_logprobs` (src/params/chat.rs:85-89 of the reference, whose responses always carry
 * `logprobs: None`): for every generated token its log-probability and the top_logprobs most likely tokens with theirs.
 * Definition.  For a step's row of V f32 logits x -- the logits the lm_head produced, the ones step_logits_out reports -- let
 * M = max_i x_i and S = sum_i exp(x_i - M).  lp(t) = (x_t - M) - log S, in f32.  The distribution is the model's own: temperature 1,
 * before the repeat penalty, independent of the request's sampler (a sampled token's logprob is that of the token the sampler picked,
 * under this distribution, computed from its raw logit).  top_logprobs = N (0 .. AHA_MAX_TOP_LOGPROBS) asks for the N tokens with the
 * largest logits, ordered by (value descending, index ascending) -- the order of aha_hip_sample_candidates, exact among equal values
 * too; if N > V the surplus entries are id 0xFFFFFFFF / logprob -inf.  A row that contains NaN, or whose every entry is -inf, is
 * unspecified.
 * Cost: two small launches per step that has a logprob row (profile classes logprob_rows_stage1 / logprob_rows_stage2) and 168 bytes
 * per token in the copy that ends the step anyway; a step without such a row takes the path it took before.
 * Out of scope: logprobs of prompt tokens (`echo`), logprobs in aha_hip_generate_batch_spec, tensor-parallel models.  `logit_bias` and
 * the presence / frequency penalties (aha_logit_adjust below) change the token choice, never these log-probabilities. */
#define AHA_MAX_TOP_LOGPROBS 20
typedef struct aha_token_logprobs {
  float    logprob;                              /* lp(emitted token) */
  int32_t  n_top;                                /* the request's top_logprobs; -1: it did not ask for logprobs, nothing else is written */
  uint32_t top_ids[AHA_MAX_TOP_LOGPROBS];        /* first n_top valid */
  float    top_logprobs[AHA_MAX_TOP_LOGPROBS];
} aha_token_logprobs;                            /* 168 bytes */

/* aha_hip_generate_batch_mm plus logprobs.  top_logprobs: HOST, n_seqs entries, -1 = none for that sequence, else 0 .. 20.
 * logprobs_out: n_seqs x max_new entries; entry [j, t] belongs to token t of sequence j (the first token included); entries past
 * n_out[j] are untouched; a sequence with -1 gets n_top = -1 in its entries and nothing else.  tokens_out, n_out and step_logits_out are
 * EXACTLY those of aha_hip_generate_batch_mm on the same arguments, for any top_logprobs; every sampler's RNG stream is consumed
 * identically.  Supported models, page reservation, cache clearing, error codes and messages are aha_hip_generate_batch_mm's;
 * additionally AHA_ERR_INVALID before any device work, naming the sequence: a null top_logprobs or logprobs_out, or an entry outside
 * -1 .. 20. */
int aha_hip_generate_batch_logprobs(aha_model* m, const uint32_t* input_ids, const size_t* seq_lens, size_t n_seqs,
                                    const aha_mm_input* const* mm, const aha_sampling_params* params, const int32_t* top_logprobs,
                                    size_t max_new, size_t max_tokens_per_pass, uint32_t* tokens_out, size_t* n_out,
                                    float* step_logits_out, aha_token_logprobs* logprobs_out);
/* aha_hip_engine_submit plus the request's top_logprobs (0 .. 20, else AHA_ERR_INVALID).  Requests of either submit function share an
 * engine and a step. */
int aha_hip_engine_submit_logprobs(aha_engine* e, const uint32_t* input_ids, size_t n_ids, const aha_mm_input* mm,
                                   const aha_sampling_params* params, size_t max_new, int32_t top_logprobs, uint64_t* req_id);
/* aha_hip_engine_step plus one entry per event: logprobs_out (NULL: exactly aha_hip_engine_step) has cap entries, entry i belongs to
 * event i.  The event of a request that did not ask for logprobs has n_top = -1, and so has a CANCELLED event.  Events, tokens and
 * logits_out are those of aha_hip_engine_step on the same submission history, bit for bit; aha_hip_engine_step itself keeps working on
 * an engine with logprob requests (it reports none and does not compute them). */
int aha_hip_engine_step_logprobs(aha_engine* e, aha_engine_event* ev, size_t cap, size_t* n_ev, float* logits_out,
                                 aha_token_logprobs* logprobs_out);

/* Host-only sampler: candle's LogitsProcessor built by get_logit_processor (sample.rs:7-38) plus use_repeat_penalty's slicing, over
 * the rand 0.9.2 StdRng of aha_hip_rng_*.  The deterministic half restates aha_amd/sampling.py (weights over the device candidates, the
 * top-p tie rule, the full-vector path); each sampled token consumes one next_u32, an ArgMax pick none.
 *   aha_hip_sampler_plan: what the device step needs after n_generated tokens: k_out candidates (0: none -- a greedy row the forward's
 *     argmax decides, or a sampler that needs the full logits vector), the temperature for the candidate step (0 for ArgMax), the
 *     effective repeat penalty and how many of the last generated ids form the penalty context.
 *   aha_hip_sampler_pick: the token from a row's candidates (vals / idx ordered by (value desc, index asc), k of them, with the
 *     full-vocabulary max and sumexp of aha_hip_sample_candidates over the penalised logits), or -- when vals is NULL or the
 *     candidates cannot decide -- from `logits` (vocab_size f32, BEFORE the penalty; the sampler applies it).  `generated` is every id
 *     generated so far (the sampler slices the penalty context).  Returns AHA_SAMPLE_NEED_LOGITS, with the RNG untouched, when it
 *     needs the full vector and logits is NULL.
 *   aha_hip_sampler_rng_words: how many u32 the sampler's stream has handed out. */
#define AHA_SAMPLE_NEED_LOGITS 1
typedef struct aha_sampler aha_sampler;
int aha_hip_sampler_create(const aha_sampling_params* params, aha_sampler** out);
void aha_hip_sampler_destroy(aha_sampler* s);
int aha_hip_sampler_plan(const aha_sampler* s, size_t vocab_size, size_t n_generated, int32_t* k_out, float* temperature_out,
                         float* repeat_penalty_out, size_t* n_context_out);
int aha_hip_sampler_pick(aha_sampler* s, const float* vals, const uint32_t* idx, int32_t k, float max, float sumexp, const float* logits,
                         size_t vocab_size, const uint32_t* generated, size_t n_generated, uint32_t* token_out);
uint64_t aha_hip_sampler_rng_words(const aha_sampler* s);

/* ---- logit_bias, presence_penalty, frequency_penalty ------------------------------------------------------------------------
 * The chat request's three remaining sampling fields (src/params/chat.rs:75-81,109-112 of the reference, which declares and never
 * reads them).  Definition, for one request with generated tokens g[0..t) and the step's V f32 logits x (what step_logits_out reports):
 *   1. y = x after the repeat penalty (unchanged: distinct ids of the last repeat_last_n generated tokens, / if >= 0 else *).
 *   2. c_i = occurrences of id i in ALL of g[0..t) (not windowed; ids >= V ignored; prompt tokens are not counted).  The addend of id i is
 *      a_i = (float)((double)b_i - (double)frequency_penalty * c_i - (double)presence_penalty * [c_i > 0]), computed on the host in f64
 *      and rounded once; b_i is the request's bias for i (0 if none).  Ids with b_i == 0 and c_i == 0 have no addend.
 *   3. z_i = y_i + a_i, one f32 add (ids without an addend: z_i = y_i).  A b_i of -inf gives z_i = -inf: the token is never chosen.
 *   4. The request's sampler runs on z wherever it ran on y: argmax (first maximal index), the candidates, their max and sumexp over
 *      the whole vocabulary, the top-p cut, the draw.  RNG consumption per token is unchanged.
 *   5. Logprobs keep their definition: the model's own distribution, from the raw x.
 * The first token has every c_i = 0: only the bias applies.  A sparse token ban is a bias of -inf.
 * An adjust is INACTIVE when both penalties are 0 and n_bias == 0; a NULL adjust pointer means inactive.  A row / step without a live
 * addend launches and copies exactly what it did before; one with addends takes the candidate step (k = 1 for ArgMax), whose stage 1
 * finds each wave's slice of the row's sorted (id, addend) list by binary search -- the list (8 bytes per entry) is uploaded with the
 * step's row table.
 * Errors, AHA_ERR_INVALID before any device work, naming the sequence: a NaN or infinite penalty, n_bias > AHA_MAX_LOGIT_BIAS, a null
 * array with n_bias > 0, a bias id >= vocab_size, a duplicate id, a NaN or +inf bias, -inf biases on every id of the vocabulary.
 * Out of scope: the single-sequence aha_hip_sample_candidates path; aha_hip_generate_batch_spec; dense allowed-token masks and
 * grammars; the repeat penalty's own context walk in stage 1, which is unchanged. */
#define AHA_MAX_LOGIT_BIAS 1024
typedef struct aha_logit_adjust {
  float presence_penalty;    /* 0 = off; finite */
  float frequency_penalty;   /* 0 = off; finite */
  const uint32_t* bias_ids;  /* n_bias distinct ids < vocab_size, any order */
  const float* bias_vals;    /* finite or -inf */
  size_t n_bias;             /* <= AHA_MAX_LOGIT_BIAS */
} aha_logit_adjust;          /* 32 bytes */
/* aha_hip_generate_batch_logprobs plus `adjust`: HOST, n_seqs entries (NULL: all inactive).  top_logprobs and logprobs_out may both be
 * NULL (no logprobs); params NULL still means greedy.  With every adjust inactive: tokens, step logits, logprobs and launches are those
 * of aha_hip_generate_batch_logprobs.  Everything else (models, pages, cache clearing, errors) is aha_hip_generate_batch_logprobs's. */
int aha_hip_generate_batch_adjusted(aha_model* m, const uint32_t* input_ids, const size_t* seq_lens, size_t n_seqs,
                                    const aha_mm_input* const* mm, const aha_sampling_params* params, const aha_logit_adjust* adjust,
                                    const int32_t* top_logprobs, size_t max_new, size_t max_tokens_per_pass, uint32_t* tokens_out,
                                    size_t* n_out, float* step_logits_out, aha_token_logprobs* logprobs_out);
/* aha_hip_engine_submit_logprobs plus the request's adjust (NULL: inactive; its arrays are copied).  top_logprobs -1: none.  Requests of
 * all three submit functions share an engine and a step; aha_hip_engine_step and aha_hip_engine_step_logprobs are unchanged. */
int aha_hip_engine_submit_adjusted(aha_engine* e, const uint32_t* input_ids, size_t n_ids, const aha_mm_input* mm,
                                   const aha_sampling_params* params, const aha_logit_adjust* adjust, size_t max_new, int32_t top_logprobs,
                                   uint64_t* req_id);
/* The host sampler with an adjust (NULL or inactive: none): it keeps a copy and the running counts, which follow the `generated`
 * arrays later calls pass.  Errors as above, except those that need a vocabulary.  aha_hip_sampler_plan then returns k_out = 1 for an
 * ArgMax sampler while an addend is live (a non-zero bias, or any generated token); aha_hip_sampler_pick adds the addends in its
 * full-vector path, after its own penalty -- candidates passed to it must come from aha_hip_sample_rows_adjusted with the step's list.
 * aha_hip_sampler_adjust_list: that list after `generated[0 .. n_generated)`, sorted by id: *n_out entries into ids_out / vals_out
 * (AHA_ERR_INVALID, with *n_out set, if cap is too small; at most n_bias + the distinct generated ids). */
int aha_hip_sampler_set_adjust(aha_sampler* s, const aha_logit_adjust* adjust);
int aha_hip_sampler_adjust_list(aha_sampler* s, size_t vocab_size, const uint32_t* generated, size_t n_generated, uint32_t* ids_out,
                                float* vals_out, size_t cap, size_t* n_out);

/* ---- guided decoding: per-step allowed-token masks ----------------------------------------------------------------------------------
 * What `response_format` / Structured Outputs (src/params/chat.rs:115-118,226 of the reference, declared and never acted on), guided
 * choice, tool-call grammars and regex constraints need from the backend: the caller owns the grammar and hands over one bit per
 * vocabulary id each step; the bits are applied inside the kernel that already reads the logits row.
 * A token mask is W = ceil(V / 32) uint32_t words.  Id i is allowed iff bit i & 31 of word i >> 5 is set.  Bits at positions >= V in the
 * last word are ignored, whatever they hold.  For one request and one step:
 *   1-3. z = the row after the repeat penalty and the addends, steps 1-3 of the logit_bias definition above, unchanged.
 *   3b.  z_i = -inf for every id i that is not allowed.
 *   4.   The request's sampler runs on that z wherever it ran on z before: argmax (first maximal index), the candidates, max and sumexp
 *        over the whole vocabulary, the top-p cut, the draw.  RNG consumption per token is unchanged.
 *   5.   Logprobs keep their definition: the model's own distribution, from the raw logits.
 * The first token is masked too.  Stop tokens are ordinary ids: the caller sets their bits when the constraint may end.
 * A request with no mask, or a step for which the callback says "no mask", takes exactly the path it takes without this section.  A
 * masked row is a candidate row (k = 1 for ArgMax), as a row with a live addend is; stage 1 of the candidate step takes one more
 * instantiation for it, in which each wave loads its 16 mask words once.  A row that falls back to its full vector gets the mask on the
 * host.  A mask with no allowed id < V is an error (AHA_ERR_INVALID); one that, together with -inf biases, leaves no finite logit is
 * unspecified, like the all--inf row of the logprob section.
 * Out of scope: grammars, regex and JSON-schema compilation (the caller's job: they feed the callback / set_mask);
 * aha_hip_generate_batch_spec; the single-sequence aha_hip_sample_candidates; tensor-parallel models.
 *
 * aha_token_mask_fn: called on the host once per live sequence per step, the first token included (n_generated == 0), after the step's
 * device work has been queued and before its candidate step is, so a grammar's work overlaps the forward pass.  `generated` are the
 * sequence's tokens so far; mask_words (n_words == W) arrives holding that sequence's previous mask, the first time all ones.  Return 1:
 * use mask_words; 0: this step is unmasked; negative: the call fails with AHA_ERR_STATE, naming the sequence and step.  A mask without an
 * allowed id: AHA_ERR_INVALID, the same way.  The cache is cleared as on every error. */
typedef int (*aha_token_mask_fn)(void* user, size_t seq, const uint32_t* generated, size_t n_generated, uint32_t* mask_words,
                                 size_t n_words);
/* aha_hip_generate_batch_adjusted plus the callback and its user pointer.  One device buffer of n_seqs x W words; a sequence's words
 * (W * 4 bytes) are uploaded only when the callback returned 1.  mask_fn NULL: exactly aha_hip_generate_batch_adjusted. */
int aha_hip_generate_batch_masked(aha_model* m, const uint32_t* input_ids, const size_t* seq_lens, size_t n_seqs,
                                  const aha_mm_input* const* mm, const aha_sampling_params* params, const aha_logit_adjust* adjust,
                                  const int32_t* top_logprobs, size_t max_new, size_t max_tokens_per_pass, aha_token_mask_fn mask_fn,
                                  void* mask_user, uint32_t* tokens_out, size_t* n_out, float* step_logits_out,
                                  aha_token_logprobs* logprobs_out);
/* aha_hip_engine_submit_adjusted plus an initial mask (mask_words NULL: none; copied), which governs the first token.
 * aha_hip_engine_set_mask: callable between steps for a waiting or running request; the mask (copied) stays until it is replaced, words
 * NULL clears it, and it acts from the next token the request samples.  AHA_ERR_INVALID before any device work: an unknown, cancelled or
 * ended id, n_words != W, no allowed id.  A request's mask lives and dies with the request: a slot taken by the next request starts
 * unmasked, a cancelled request leaves nothing behind.  aha_hip_engine_step / _step_logprobs are unchanged and, on an engine without
 * masks, so are their launches. */
int aha_hip_engine_submit_masked(aha_engine* e, const uint32_t* input_ids, size_t n_ids, const aha_mm_input* mm,
                                 const aha_sampling_params* params, const aha_logit_adjust* adjust, const uint32_t* mask_words,
                                 size_t n_mask_words, size_t max_new, int32_t top_logprobs, uint64_t* req_id);
int aha_hip_engine_set_mask(aha_engine* e, uint64_t req_id, const uint32_t* words, size_t n_words);
/* The host sampler with a mask (copied; words NULL clears it; AHA_ERR_INVALID for n_words == 0 or all-zero words).  aha_hip_sampler_plan
 * then returns k_out = 1 for an ArgMax sampler; aha_hip_sampler_pick applies the mask in its full-vector path, after the addends
 * (AHA_ERR_INVALID if n_words != ceil(vocab_size / 32) or no id < vocab_size is allowed) -- candidates passed to it must come from
 * aha_hip_sample_rows_masked with the same words. */
int aha_hip_sampler_set_mask(aha_sampler* s, const uint32_t* words, size_t n_words);

/* ---- checkpoint directory -> model (XxxGenerateModel::init minus tokenizer / chat template) --------------------------
 * aha_hip_config_parse: <dir>/config.json -> aha_model_desc, the same field mapping serde does into Qwen3Config
 *   (/root/reference/src/models/qwen3/config.rs:4-27), Qwen3VLConfig (qwen3vl/config.rs:51-133, text_config / vision_config,
 *   top-level tie_word_embeddings qwen3vl/model.rs:853) or Qwen3ASRConfig (qwen3_asr/config.rs:6-22, thinker_config.*);
 *   stop tokens from <dir>/generation_config.json eos_token_id (qwen3/generate.rs:33-36; a scalar or a list).  The
 *   architecture is taken from "model_type" / the presence of vision_config / thinker_config.  Host only (no GPU).
 * aha_hip_weights_open: mmaps every *.safetensors file in <dir> (find_type_files, utils/mod.rs:121-137 +
 *   VarBuilder::from_mmaped_safetensors, qwen3/generate.rs:30-31) and indexes the tensors; views point into the mappings
 *   and stay valid until aha_hip_weights_close.  Host only.
 * aha_hip_model_load = config_parse + weights_open + aha_hip_model_create + weights_close. */
typedef struct aha_weights aha_weights;
int aha_hip_config_parse(const char* model_dir, aha_model_desc* out);
/* The dtype string the reference's init passes to get_dtype for this checkpoint: Qwen3 config.json "torch_dtype"
 * (qwen3/config.rs:23, qwen3/generate.rs:28), Qwen3-VL "text_config.dtype" (qwen3vl/config.rs:100), Qwen3-ASR the constant
 * "bfloat16" (qwen3_asr/config.rs:186).  NUL-terminated into out (cap bytes).  A host calls
 * aha_hip_get_dtype(requested, <this>, &d) and aha_hip_check_dtype(d) before aha_hip_model_load, so that an f16 / f32
 * checkpoint without an explicit dtype is refused the way the header promises instead of silently computing in bf16. */
int aha_hip_config_torch_dtype(const char* model_dir, char* out, size_t cap);
int aha_hip_weights_open(const char* model_dir, aha_weights** out);
size_t aha_hip_weights_count(const aha_weights* w);
int aha_hip_weights_get(const aha_weights* w, size_t index, aha_tensor_view* out);
void aha_hip_weights_close(aha_weights* w);
int aha_hip_model_load(aha_ctx* ctx, const char* model_dir, size_t kv_reserve_tokens, aha_model** out);

/* ---- InferenceModel (common/mod.rs:25-45) ------------------------------------------------------------------- */
/* forward_initial(&mut self, input_ids, seqlen_offset, data) -> logits (1,1,V).
 * logits_out (V floats, host, may be NULL) receives the last position's logits as f32 exactly as the generic loop
 * reads them (generate.rs:75).  argmax_out (may be NULL) receives the first maximal index (Sampling::ArgMax). */
int aha_hip_forward_initial(aha_model* m, const uint32_t* input_ids, size_t n_ids, size_t seqlen_offset,
                            const aha_mm_input* mm, float* logits_out, uint32_t* argmax_out);
/* forward_step(&mut self, input_ids (1,1), seqlen_offset) -> logits (1,1,V). */
int aha_hip_forward_step(aha_model* m, uint32_t token, size_t seqlen_offset, float* logits_out, uint32_t* argmax_out);
/* clear_cache(&mut self) */
int aha_hip_clear_cache(aha_model* m);
/* stop_token_ids(&self) -> Vec<u32>: writes up to cap ids, returns the count (>=0) or a negative status. */
int aha_hip_stop_token_ids(const aha_model* m, uint32_t* out, size_t cap);

/* Extension (not in the reference): device-resident greedy loop = generate_generic with temperature 0
 * (generate.rs:115-159) without a host round trip per token.  Must follow a forward_initial/forward_step call;
 * first_token is the token sampled from that call.  Writes up to max_new tokens; stops after an eos id.
 * Returns the number of tokens written or a negative status. */
int aha_hip_decode_greedy(aha_model* m, uint32_t first_token, size_t seqlen_offset, size_t max_new, uint32_t* tokens_out);

/* D11, device half of sample_and_push (common/generate.rs:70-86) for the non-greedy samplers of get_logit_processor
 * (common/sample.rs:7-38: candle LogitsProcessor TopK / TopKThenTopP / TopP).  Works on the logits the last
 * forward_initial / forward_step / decode_greedy call left on the device:
 *   1. use_repeat_penalty (sample.rs:41-60 -> candle_transformers::utils::apply_repeat_penalty): every DISTINCT id of
 *      `context` (the caller passes the last repeat_last_n generated ids, sample.rs:49-53) has its logit divided by
 *      repeat_penalty if >= 0, multiplied otherwise; repeat_penalty == 1 or n_context == 0 leaves the logits unchanged;
 *   2. the k (1..64) largest penalised logits, ordered by (value descending, index ascending), into vals_out / idx_out;
 *   3. max_out / sumexp_out = max_i x_i and sum_i exp((x_i - max) / temperature) over the WHOLE vocabulary, so that
 *      exp((vals_out[j] - max) / temperature) / sumexp equals the probability candle's softmax(logits / temperature)
 *      assigns to candidate j (temperature <= 0 is treated as 1).
 * The host finishes with the top-p cut over the candidates and the weighted draw (aha_hip_rng_* below): 8k + 8 bytes leave the device per
 * token instead of the V-float logits vector.  Not in the reference as a function: it replaces the body of
 * LogitsProcessor::sample up to the random draw.  If k exceeds the vocabulary the surplus entries come back as value -inf /
 * index 0xFFFFFFFF.  Under tensor parallelism (vocab-parallel lm_head) the call is collective: every rank makes it, the
 * shards of the logits are all-reduced first. */
int aha_hip_sample_candidates(aha_model* m, const uint32_t* context, size_t n_context, float repeat_penalty, float temperature,
                              int32_t k, float* vals_out, uint32_t* idx_out, float* max_out, float* sumexp_out);

/* The V f32 logits of the last forward call, exactly what logits_out of that call would have received (fallback of the
 * candidate path: Sampling::All, or a TopP whose nucleus is wider than 64 tokens). */
int aha_hip_last_logits(aha_model* m, float* logits_out);

/* The random draw of candle's LogitsProcessor (the `rng` field and sample_multinomial of candle-transformers 0.9.2, built by
 * get_logit_processor, /root/reference/src/models/common/sample.rs:7-37 with seed 299792458, common/generate.rs:408,452, or
 * 34562, qwen3_asr/generate.rs:134), host code:
 *   aha_hip_rng_create(seed)        = rand 0.9.2 StdRng::seed_from_u64(seed)   (candle-transformers' own rand, Cargo.lock:590-606):
 *                                     PCG32 expansion of the u64 to 32 seed bytes, ChaCha12 stream, block counter 0, stream id 0
 *   aha_hip_rng_next_u32            = RngCore::next_u32 on it
 *   aha_hip_rng_weighted_index      = WeightedIndex::<f32>::new(weights)?.sample(&mut rng): ONE next_u32; index of the first running
 *                                     f32 sum greater than the uniform draw in [0, total).  AHA_ERR_INVALID for a negative / NaN
 *                                     weight or an all-zero vector (the crate's Err(..)), with the RNG left untouched.
 * [unverified] against the crates themselves (not on disk, no cargo): restated from their published algorithms, see
 * csrc/sampler_rng.hip.  For Sampling::TopK / TopKThenTopP candle draws over the k probabilities in the order
 * select_nth_unstable_by leaves them, which Rust does not specify: callers pass them ranked (probability desc, logit desc,
 * index asc), the order aha_hip_sample_candidates returns. */
typedef struct aha_rng aha_rng;
int aha_hip_rng_create(uint64_t seed, aha_rng** out);
void aha_hip_rng_destroy(aha_rng* rng);
uint32_t aha_hip_rng_next_u32(aha_rng* rng);
int aha_hip_rng_weighted_index(aha_rng* rng, const float* weights, size_t n, uint32_t* index_out);
/* Test hook: the ChaCha block function (even `rounds`) on a 16-word state -- RFC 7539 section 2.3.2 pins it at 20 rounds. */
int aha_hip_debug_chacha_block(const uint32_t* state16, int rounds, uint32_t* out16);

/* Extension for the image-parallel ViT (each GPU encodes its share of the images, embeddings are all-gathered over RCCL):
 * runs only the vision tower on `mm` (its images, then its videos) and writes (1 + n_deepstack, n_tokens, hidden) bf16 to out_dev
 * (device memory, may be NULL to query n_tokens); rows = the images' tokens followed by the videos' tokens. */
int aha_hip_vision_encode(aha_model* m, const aha_mm_input* mm, void* out_dev, int64_t* n_tokens);

/* Tensor-parallel seam.  Either (a) a host callback that must leave buf = sum over ranks of buf (count f32, device memory)
 * before it returns -- e.g. torch.distributed.all_reduce over RCCL on a tensor view of buf -- or (b) an RCCL communicator
 * owned by the library: every rank calls aha_hip_tp_unique_id on rank 0's bytes (128) and aha_hip_tp_init_rccl.  With (b)
 * the all-reduce is enqueued on the model's stream (no host synchronisation). */
typedef int (*aha_allreduce_fn)(void* buf_f32_dev, size_t count, void* user);
int aha_hip_set_allreduce(aha_model* m, aha_allreduce_fn fn, void* user);
int aha_hip_tp_unique_id(void* out128);
int aha_hip_tp_init_rccl(aha_model* m, const void* unique_id128);
/* Sequence-parallel prefill ("reduce-scatter + all-gather, sequence-parallel norms").  With it a
 * tensor-parallel prefill keeps the residual stream row-sharded (rank r owns rows [r*ceil(S/T), ...)): the f32 partial sums of
 * o_proj / down_proj are REDUCE-SCATTERED over rows (same f32 sums as the all-reduce: identical numerics), the residual add and
 * the next RMSNorm run on the owned rows only, and the normalised bf16 rows are ALL-GATHERED for the next column-parallel
 * GEMM -- (T-1)/T * (4 + 2) bytes per element and rank instead of 2 * (T-1)/T * 4 for the ring all-reduce.
 * Used automatically when the library owns an RCCL communicator (aha_hip_tp_init_rccl; the collectives it overlaps with GEMMs on its
 * communication stream run on a second communicator of the same ranks, split off at init -- AHA_TP_SIDE_COMM=0 shares the first one);
 * with the host-callback seam install:
 *   reduce_scatter(buf, count_per_rank): buf holds T * count_per_rank f32 on the device; on return rank r's slice
 *       buf[r*count_per_rank ..) must hold the sum over ranks of that slice (the other slices are undefined);
 *   all_gather(buf, bytes_per_rank): rank r's slice of buf (T * bytes_per_rank bytes) is its contribution; on return every
 *       slice must be filled on every rank.
 * Passing NULLs removes them (all-reduce path).  AHA_TP_SP=0 in the environment forces the all-reduce path. */
typedef int (*aha_reduce_scatter_fn)(void* buf_f32_dev, size_t count_per_rank, void* user);
typedef int (*aha_all_gather_fn)(void* buf_dev, size_t bytes_per_rank, void* user);
int aha_hip_set_seq_parallel(aha_model* m, aha_reduce_scatter_fn reduce_scatter, aha_all_gather_fn all_gather, void* user);
/* Context-parallel prefill (round 4; the 288-GB design of SURVEY.md section 8e row 3 "long-context text prefill": an 8B checkpoint is
 * 16 GB, so every GPU holds the FULL weights -- create the model with tp_size 1 on every rank -- and the PROMPT is sharded instead).
 * The prompt's 64-token KV pages are cut into 2 * world contiguous chunks; rank r owns chunks r and 2 * world - 1 - r (balanced causal
 * work) and runs every GEMM / norm / rope of the prefill on its own rows only; per layer the ranks all-gather that layer's K / V pages
 * (the one op that couples rows is attention).  After the call EVERY rank holds the complete KV cache and the last position's logits
 * (rank 0 owns the last row; it is broadcast), so decode continues on any rank -- rank 0 by convention -- with no hand-back.
 * Inbound bytes per rank and layer at 41 k tokens on 8 GPUs: 147 MB, against 1.76 GB for the tensor-parallel form above.
 * Every rank calls aha_hip_forward_initial with the same ids (offset 0: a fresh cache; other calls run unsharded on every rank).
 * Collective: an RCCL communicator owned by the library (aha_hip_tp_unique_id on rank 0, then aha_hip_cp_init_rccl on every rank), or
 * the host callback `all_gather` (same contract as aha_hip_set_seq_parallel's; tests).  world = 1 switches it off.
 * Prompts below AHA_CP_MIN_ROWS (default 2048) tokens or with fewer than 4 * world pages run unsharded. */
int aha_hip_set_context_parallel(aha_model* m, int32_t rank, int32_t world, aha_all_gather_fn all_gather, void* user);
int aha_hip_cp_init_rccl(aha_model* m, const void* unique_id128);
/* Host only (no GPU): the rows rank `rank` of `world` owns in a context-parallel prefill of n_tokens -- out5 = {first row and length of
 * its early chunk, first row and length of its late chunk, page slots per rank of the exchange's staging buffer}.  Returns 1 (and leaves
 * out5 alone) when such a prompt is not sharded (fewer than 4 * world pages, world outside 2..8). */
int aha_hip_debug_cp_plan(int32_t n_tokens, int32_t world, int32_t rank, int32_t* out5);
/* KV hand-back after a sharded prefill ("for single-GPU decode afterwards, all-gather KV to GPU 0";
 * north_star: decode stays single-GPU).  A tensor-parallel prefill leaves every rank with the K / V of ITS kv heads, in its own
 * pages.  aha_hip_kv_export packs them into a contiguous device buffer
 *     [layer][page][this rank's kv head][K block 16 KB | V block 16 KB]      (pages = ceil(cache_len / 64), fragment-major blocks)
 * = the byte image of the pages, so it can cross a collective (RCCL gather / all-gather, 738 MB per rank and 41 k tokens at 8B)
 * untouched; aha_hip_kv_import copies `n_heads` heads starting at head `src_head0` of such a buffer (which holds `src_heads` heads
 * per page) into heads [dst_head0, dst_head0 + n_heads) of THIS model's pages -- an un-sharded model on GPU 0 imports rank r's
 * buffer at dst_head0 = r * kv_heads / T --, maps pages for n_tokens, and sets the cache length and the Qwen3-VL rope_delta so
 * that forward_step / decode_greedy continue exactly as after a single-GPU prefill.  out_dev NULL: only the sizes are returned.
 * `in_bytes` is the size of the buffer behind in_dev: it must hold layers x ceil(n_tokens / 64) x src_heads x 32 KB, else
 * AHA_ERR_INVALID (nothing is read).  The destination must be un-sharded (tp_size 1); an import invalidates the logits an earlier
 * forward call left behind.
 * No reference counterpart (the reference has no collectives): the contract is "decode after export + import == decode after
 * the same prefill on one GPU" (tests/test_tp_gpu.py). */
int aha_hip_kv_export(aha_model* m, void* out_dev, size_t out_bytes, size_t* bytes_needed, size_t* n_tokens, int64_t* rope_delta);
int aha_hip_kv_import(aha_model* m, const void* in_dev, size_t in_bytes, int32_t src_heads, int32_t src_head0, int32_t dst_head0,
                      int32_t n_heads, size_t n_tokens, int64_t rope_delta);
/* Test hook: run the installed all-reduce (RCCL communicator or callback) once on a caller-owned f32 device buffer and
 * wait for it.  Lets a 1-GPU box exercise the RCCL wiring with a communicator of size 1. */
int aha_hip_debug_allreduce(aha_model* m, void* buf_f32_dev, size_t count);

/* ---- quantised weight copies for decode ------------------------------------------------------------------------- */
/* aha_hip_model_quantize_weights: quantise the layer matrices (wqkv, wo, wgu, wdown) of a created model to MXFP8 (see
 * aha_hip_quantize_mxfp8), in place: each bf16 matrix W is overwritten with W' = dequantised W and its (q, scales) copy is kept beside it.
 * The batched decode matvec (every aha_hip_generate_batch* entry and the engine) then streams q and the scales, 1.03125 bytes per weight
 * instead of 2, with the bits it would compute from W', and so does the single-sequence decode matvec (aha_hip_forward_step,
 * aha_hip_decode_greedy, the generate_generic loops, the last-row lm_head of aha_hip_forward_initial: gemv_mxfp8_kernel, bit-identical to
 * the bf16 kernel on W') on the matrices it measured faster on, those of 2^24 elements or more whose launch takes the kernel's FAST form (aha_hip_debug_fp8_single); prefill and
 * every other path go on reading the bf16 W'.  flags: 0, or
 * AHA_WQ_LM_HEAD to quantise lm_head too (with tied embeddings: the embedding table).  Costs 0.516 x the quantised matrices in memory.
 * AHA_ERR_INVALID: a null model, an unknown format or flag, or a weight that is not finite (or >= 1.9375 * 2^127 in magnitude), naming
 * the tensor -- every matrix is checked before any is modified.  AHA_ERR_STATE: the cache is not empty, the model has an engine, or it
 * was quantised with other arguments (the same arguments again: AHA_OK, nothing done).  AHA_ERR_UNSUPPORTED, naming the cause: a tensor-
 * or context-parallel model, a matrix whose K is not a multiple of 32, a model outside aha_hip_generate_batch's set.  AHA_ERR_OOM: the
 * copies cannot be had; the model is as it was.  Reads no environment variable.
 * format AHA_WQ_MXFP4_E2M1 does the same with MXFP4 copies (see aha_hip_quantize_mxfp4): W' = dequantised W in place, E2M1 nibbles and
 * the same scale words beside it, 0.53125 bytes per weight for the batched decode matvec (gemv_rows_mxfp4_kernel, the bits of the bf16
 * kernel on W'), +0.266 x the quantised matrices in memory, a weight refused when it is not finite or above 1.5 * 2^127 in magnitude.
 * An MXFP4 model's single-sequence decode (aha_hip_forward_step, aha_hip_decode_greedy, the generate loops, the last-row lm_head) reads
 * the same copies through a batch-1 kernel of its own (gemv_mxfp4_kernel, bit-identical to the bf16 kernel on W') on the matrices its
 * plan takes (aha_hip_debug_fp4_single; profiles/weights_fp4_single.md has what was measured) and runs the bf16 matvec on W' on the
 * others.  A model holds copies of one format: quantising with the other afterwards is AHA_ERR_STATE. */
#define AHA_WQ_NONE 0
#define AHA_WQ_MXFP8_E4M3 1
#define AHA_WQ_MXFP4_E2M1 2
#define AHA_WQ_LM_HEAD 1u
int aha_hip_model_quantize_weights(aha_model* m, int32_t format, uint32_t flags);
/* *format = AHA_WQ_NONE or the format the model was quantised with, *flags its flags (either pointer may be NULL). */
int aha_hip_model_weight_format(const aha_model* m, int32_t* format, uint32_t* flags);
/* Test hook: on = 0 makes a quantised model's batched decode run the bf16 matvec on W' instead of the FP8 one (the same bits); on = 1
 * (the default) restores it.  It holds for either format: on = 0 sends an MXFP4 model to the bf16 kernel on W' as well. */
int aha_hip_debug_fp8_rows(aha_model* m, int on);
/* The switch of the single-sequence decode matvec (the decode step's four projections and the lm_head); independent of
 * aha_hip_debug_fp8_rows, and unlike it three-valued, because here the plan may keep a shape on bf16.  on = 1 (the default): a matrix with a copy is read from it where the plan takes its shape -- the matrices for
 * which the FP8 kernel measured faster, at least 2^24 elements and K a multiple of 512 * U, the FAST form (aha_hip_debug_plan_gemv_mxfp8
 * tells; profiles/weights_fp8_single.md) -- so small models, the test suite's among them, decode on bf16 unless the switch is 2;
 * 2: every matrix with a copy; 0: none (the bf16 kernel on W').  The bits are the same in all three.  Profile class of the FP8 launches:
 * gemv_fp8 (bf16: gemv).  AHA_ERR_INVALID: a null model or another value.  FP8 copies only: an MXFP4 model ignores this switch (value 2
 * included) and has aha_hip_debug_fp4_single. */
int aha_hip_debug_fp8_single(aha_model* m, int on);
/* aha_hip_debug_fp8_single's twin for a model with MXFP4 copies; it replaces "an MXFP4 model's single-sequence path always runs the bf16
 * matvec".  on = 1 (the default): a matrix with a copy is read from it by gemv_mxfp4_kernel where that kernel's plan takes the shape
 * (aha_hip_debug_plan_gemv_mxfp4 tells; the rule and the measurements: profiles/weights_fp4_single.md); 2: every matrix with a copy;
 * 0: none (the bf16 kernel on W', what the path ran before the kernel existed).  The bits are the same in all three.  Profile class of
 * the FP4 launches: gemv_fp4, at 0.53125 bytes per weight.  Sharded models have no copies.  AHA_ERR_INVALID: a null model or another
 * value.  An MXFP8 model ignores it. */
int aha_hip_debug_fp4_single(aha_model* m, int on);
/* Exact 13-bit weight copies.  When a model is created unsharded, each of the four layer matrices and lm_head gets a copy that holds
 * every bf16 weight exactly in 13 bits (aha_hip_pack_pk13 has the format) if the matrix has at least 2^24 elements, K is a multiple of
 * 4096, every weight is finite, at most 16 rows hold a weight below the format's window (those rows are then read from the bf16 matrix,
 * aha_hip_pack_pk13_rows), and the device has the copies' bytes plus a tenth more free; otherwise that matrix, or every matrix, stays
 * without one, silently.  The single-sequence decode matvec then streams 0.8125 of the bytes and computes the same
 * bits (gemv_kernel_pk13; profiles/weights_pk13.md).  AHA_WPACK=0 in the environment, read when a model is created, makes no copies.
 * aha_hip_model_quantize_weights frees the copies: a quantised model never reads them.
 * aha_hip_debug_pk13_single: on = 1 (the default): a matrix with a copy is read from it where the plan takes its shape
 * (aha_hip_debug_plan_gemv_pk13 tells); 2: wherever a copy exists; 0: nowhere (the bf16 kernel).  The bits are the same in all three, and
 * the launches stay in profile class gemv, at 1.625 bytes per weight.  AHA_ERR_INVALID: a null model or another value.
 * aha_hip_pk13_status: one line per matrix into buf (NUL-terminated, truncated to cap), "<tensor name>\t<status>\n", status "packed",
 * "<n> weights outside the window: packed, rows <list> read from bf16", or the reason the matrix has no copy; returns the number of matrices with a copy, or a negative error. */
int aha_hip_debug_pk13_single(aha_model* m, int on);
int aha_hip_pk13_status(const aha_model* m, char* buf, size_t cap);

/* ---- introspection used by bench.py / tests ------------------------------------------------------------------ */
size_t aha_hip_cache_len(const aha_model* m);
/* Decode steps the device ran in the last aha_hip_decode_greedy call, including the ones queued past a stop token (at most
 * AHA_DECODE_RUNAHEAD - 1 = 3 by default: the host watches the tokens in pinned memory while later steps are queued). */
int64_t aha_hip_debug_steps_executed(const aha_model* m);
/* Diagnostic: microseconds per decode step at the current cache length, (a) enqueued launch by launch, (b) replayed as one captured
 * hipGraph -- identical kernel arguments in both, results discarded, the cache is cleared afterwards (scripts/bench_graph_step.py). */
int aha_hip_debug_graph_step(aha_model* m, int32_t replays, double* us_launches, double* us_graph);
/* Per-kernel-class HIP-event timing of subsequent forward calls (adds one event pair per launch).  0 = off. */
int aha_hip_set_profiling(aha_model* m, int enable);
/* name: e.g. "gemv", "gemm", "attn_decode", "attn_prefill".  Returns accumulated ms and launch count since enable. */
int aha_hip_get_profile(aha_model* m, const char* kernel_class, double* total_ms, int64_t* launches, double* bytes,
                        double* flops);
/* Debug knob for the paged-KV property tests: 1 => hand out physical pages in a scrambled order. */
int aha_hip_debug_scramble_pages(aha_model* m, int enable);
/* Which form of the fused decode attention the last single-request decode step launched: 1 = linear (page addresses formed by
 * arithmetic from two kernel arguments: the cache's pages are an arithmetic progression), 0 = page table, -1 = no step yet. */
int aha_hip_debug_attn_decode_form(const aha_model* m);
/* Copies the last hidden state before lm_head (hidden_size floats) / the image embeddings of the last
 * forward_initial (rows x out_hidden floats) to the host, for parity tests of intermediate tensors. */
int aha_hip_debug_last_hidden(aha_model* m, float* out, size_t n);
/* Test tool: fill the LDS of every CU with seeded garbage (on `stream`).  A kernel that consumes LDS it did not stage itself gives
 * run-to-run identical results when its launch is simply repeated and different ones behind different poisons
 * (tests/test_ops_gpu.py::test_kernels_do_not_consume_unstaged_lds). */
int aha_hip_debug_poison_lds(uint32_t seed, void* stream);
/* Test entry of the row-grouped GEMM behind the tensor-parallel prefill's chunked all-gather (csrc/kernels.h launch_gemm_grouped): `groups`
 * row segments of M rows each, all x W^T (N, K): segment g reads A rows [g * a_gstride, + M) (row pitch K) and writes C rows
 * [c_row0 + g * c_gstride, + M) (row pitch ldc), clipped to rows < m_total.  act: plain (0) or gate+up pairs (4). */
int aha_hip_debug_gemm_grouped(const void* A, const void* W, void* C, int32_t M, int32_t N, int32_t K, int32_t ldc, int32_t act,
                               int32_t groups, int32_t a_gstride, int32_t c_gstride, int32_t c_row0, int32_t m_total, void* stream);
/* Test hook: the prefill attention's score chain.  3 (the default since round 5; env AHA_ATTN_SMX) = the scores stay the f32 QK^T
 * accumulators through scale, mask, maximum and exponential, P is rounded to bf16 once for the P.V product; 1 / 0 = the reference's
 * eager path, which materialises `q.k^T` and `* scaling` in bf16 (modules.rs:782-783), with the scale multiply on the matrix pipe
 * (csrc/attn_common.h mfma_diag) / in the vector ALU -- the same bits as each other, the bit-faithful forms.  -1 = back to the
 * default.  Both chains are held to the same parity bounds (profiles/r05_attn_prefill.md). */
int aha_hip_debug_attn_variant(int32_t smx);
/* Test hook: the prefill attention's kernel form (env AHA_ATTN_FORM).  16 = 16 q rows per wave, two 8-wave (or 4-wave) workgroups per CU
 * (csrc/kernels_attn.hip: every score chain, every head dim); 64 = one wave per SIMD, 64 q rows per wave on 32x32x16 MFMAs, 256-row
 * workgroups (csrc/kernels_attn64.hip: f32 score chain, head_dim 128 and the ViT's 72); 65 = the same, software-pipelined inside the wave;
 * -1 = automatic (the 64-row form once its 256-row blocks fill the chip).  Same rounding points in every form; the accumulation order of
 * the two MFMA shapes differs, so outputs agree to the parity bound, not bit for bit. */
int aha_hip_debug_attn_form(int32_t form);
/* Test hook: force the GEMM tile (128, 256, 192 = 256 x 192, 2128 = 256 x 128 on the eight-wave ring kernel) and split-K factor of every
 * following GEMM launch of the process;
 * (0, 0) restores the automatic choice (csrc/kernels_gemm.hip plan_gemm).  tile 1256 / 1192: the persistent kernel on 256- /
 * 192-column tiles wherever it has an instantiation and a workspace (128^2 kernel elsewhere). */
int aha_hip_debug_gemm_plan(int32_t tile, int32_t splitk);
/* Host only (no GPU): the plan the GEMM launcher would pick for a shape -- out3 = {tile (128 | 256), split-K factor, 1 if the
 * columns run as a multiple of 256 + a tail launch}; workspace_bytes = size of the caller's split-K scratch (0 = none); has_residual
 * bit 0 = a residual is added, bit 1 = an RMSNorm of the output rides on the call (o_proj / down_proj in the layer loop).  Lets the
 * CPU tier pin the plans of the BASELINE shapes (csrc/kernels_gemm.hip plan_gemm is a cost model fitted on MI355X). */
int aha_hip_debug_plan_gemm(int32_t M, int32_t N, int32_t K, int32_t act, int32_t has_bias, int32_t has_residual, size_t workspace_bytes,
                            int32_t* out3);
/* Host only (no GPU): the segment lists the persistent GEMM kernel (csrc/kernels_gemm_sk.hip) would walk for a shape on `workers`
 * workgroups (a multiple of 8) with `tile_n` (256 | 192) column tiles: out = 8 ints per segment {m0, n0, first K tile, end K tile,
 * pieces the tile is cut into, this piece's index in K order, first chunk of the tile, counter of the tile}, grouped by worker;
 * off_out[workers + 1] = where each worker's list starts; info7 = {workers, chunks, counters, tiles cut, cut style, cuts, k steps on
 * the slowest worker x 1000}.  Returns the number of segments (at most `cap` are written) or a negative error.  The CPU tier checks
 * that every (tile, K tile) is covered exactly once for the BASELINE shapes. */
int aha_hip_debug_streamk_plan(int32_t M, int32_t N, int32_t K, int32_t tile_n, int32_t workers, size_t workspace_bytes, int32_t* out,
                               int32_t cap, int32_t* off_out, int32_t* info7);
/* Host only (no GPU): the plan aha_hip_gemv_mxfp8 / the model's single-sequence FP8 matvec picks for a matrix of N rows (epi 2: N = 2I)
 * and K columns: *R rows per wave, *U 512-k chunks per work item, *grid persistent blocks (= the (max, index) partials of epi 3), and
 * (form may be NULL) *form = 0 the general kernel, 1 FAST (every chunk group full), 2 / 3 FAST with the straight-line prologue without /
 * with norm weights (has_norm).  Names the instantiation gemv_mxfp8_kernel<R, U, epi, form != 0, max(form - 1, 0)>.  *by_plan (may be
 * NULL) = 1 if a model's single-sequence step reads a matrix of this shape from its copy by default (aha_hip_debug_fp8_single). */
int aha_hip_debug_plan_gemv_mxfp8(int32_t N, int32_t K, int32_t epi, int32_t has_norm, int32_t* R, int32_t* U, int32_t* grid, int32_t* form,
                                  int32_t* by_plan);
/* The same query for aha_hip_gemv_pk13 / the single-sequence matvec from an exact 13-bit copy; K a multiple of 4096, at most 32768.
 * *U is always 8 (a work item is one 4096-column unit per row) and *form 2 / 3, or 1 past the straight-line prologue's K; names
 * gemv_kernel_pk13<R, epi, max(form - 1, 0)>.  *by_plan as aha_hip_debug_pk13_single reads it. */
int aha_hip_debug_plan_gemv_pk13(int32_t N, int32_t K, int32_t epi, int32_t has_norm, int32_t* R, int32_t* U, int32_t* grid, int32_t* form,
                                 int32_t* by_plan);
/* The same query for aha_hip_gemv_mxfp4 / the single-sequence matvec of an MXFP4 model (there was no such plan: the path had no FP4
 * kernel): names gemv_mxfp4_kernel<R, U, epi, form != 0, max(form - 1, 0)>, *by_plan as aha_hip_debug_fp4_single reads it. */
int aha_hip_debug_plan_gemv_mxfp4(int32_t N, int32_t K, int32_t epi, int32_t has_norm, int32_t* R, int32_t* U, int32_t* grid, int32_t* form,
                                  int32_t* by_plan);
/* The same query for the bf16 matvec itself (aha_hip_gemv, aha_hip_gemv_gate_up, aha_hip_gemv_epi and the model's decode step): names
 * gemv_kernel<R, U, epi, form != 0, false, max(form - 1, 0)>, by the function the launch itself calls.  epi 0..4 (4: the un-rounded f32
 * partial sums of the tensor-parallel row split); epi 2 takes N = 2I for either weight layout, and any even N (aha_hip_gemv_gate_up has
 * no 32-row blocks).  K a multiple of 8, at most 32768. */
int aha_hip_debug_plan_gemv(int32_t N, int32_t K, int32_t epi, int32_t has_norm, int32_t* R, int32_t* U, int32_t* grid, int32_t* form);
/* Host only (no GPU): the launch aha_hip_gemv_rows / _mxfp8 / _mxfp4 and the model's multi-sequence matvec pick for a matrix of N rows
 * and K columns, by the function the launch itself calls: *cw chunks (128 k) per wave, 1 | 2, and *nks K splits (the f32 slabs the merge
 * sums).  With the row tiles (2 above 16 rows of x) it names gemv_rows_kernel<cw, 1 | 2> and its MX twins.  K a multiple of 8. */
int aha_hip_debug_plan_gemv_rows(int32_t N, int32_t K, int32_t* cw, int32_t* nks);
/* Test entry of that epilogue, which only a sharded model's row-parallel projections launch: y_f32[n] = sum_k h[k] * W[n, k], f32, not
 * rounded; h = x, or RMSNorm(x; norm_w, eps) rounded to bf16 when norm_w is not NULL.  W (N, K) bf16, x (K) bf16, device pointers. */
int aha_hip_debug_gemv_partial_f32(const void* W, const void* x, float* y_f32, int32_t N, int32_t K, const void* norm_w, float eps,
                                   void* stream);
/* CUs the persistent GEMM kernel leaves free (rounded so that its workgroup count stays a multiple of 8; 0 = use every CU; < 0 = take
 * AHA_GEMM_RESERVE_CUS from the environment).  Process-wide.  For tensor-parallel prefill: RCCL's kernels on the communication stream
 * need CUs next to a GEMM whose workgroups each fill one (csrc/model.hip gemm_row_parallel).  Must be the same on every rank only
 * for speed, not for correctness (no collective depends on it). */
int aha_hip_set_gemm_reserved_cus(int32_t n);
int aha_hip_debug_image_embeds(aha_model* m, int which /*0=merged, 1..=deepstack k*/, float* out, size_t n);

/* ---- op-level entry points (device pointers; stream = hipStream_t as void*, NULL = default stream) ---------- */
/* D3: y = x / sqrt(mean(x^2)+eps) * w over the last dim (qwen3/model.rs:79,83,186; modules.rs:512-513). bf16. */
int aha_hip_rmsnorm(const void* x, const void* w, void* y, int64_t rows, int32_t dim, float eps, void* stream);
/* D4/D8 decode: y[n] = sum_k x[k] W[n,k]  (candle_nn::Linear, batch 1).  W (N,K) bf16 row-major, x (K) bf16.
 * norm_w != NULL fuses y = Linear(RMSNorm(x; norm_w, eps)); residual != NULL fuses y = residual + Linear(..). */
int aha_hip_gemv(const void* W, const void* x, void* y, int32_t N, int32_t K, const void* norm_w, float eps,
                 const void* residual, void* stream);
/* D8 decode: y[j] = silu(gate_j . h) * (up_j . h), h = RMSNorm(x) if norm_w else x.  Wg, Wu (I,K) bf16. */
int aha_hip_gemv_gate_up(const void* Wg, const void* Wu, const void* x, void* y, int32_t I, int32_t K,
                         const void* norm_w, float eps, void* stream);
/* D4/D8/V1 prefill: C[M,N] = A[M,K] . W[N,K]^T (+bias[N]) (+residual[M,N]); bf16 in/out, f32 accumulate (MFMA).
 * act: 0 none, 1 gelu_pytorch_tanh, 2 gelu (erf), 3 silu. lda/ldw/ldc in elements. K % 32 == 0. */
int aha_hip_gemm(const void* A, const void* W, void* C, int32_t M, int32_t N, int32_t K, int32_t lda, int32_t ldw,
                 int32_t ldc, const void* bias, const void* residual, int32_t act, void* stream);
/* D5/M1: q/k RMSNorm over head_dim + rotary embedding (rope.rs:96-132) on a fused qkv activation (S, (nh+2kvh)*d).
 * pos: int32 (3,S) rows T,H,W (all equal for 1-D RoPE).  axis_map: int32[d/2], frequency slot -> row of pos.
 * Writes q_out (S, nh*d) and k_out / v_out (S, kvh*d) contiguous (op-level variant without the paged cache). */
int aha_hip_qknorm_rope(const void* qkv, const void* q_norm_w, const void* k_norm_w, const int32_t* pos,
                        const int32_t* axis_map, void* q_out, void* k_out, void* v_out, int32_t S, int32_t nh,
                        int32_t kvh, int32_t d, float eps, float theta, void* stream);
/* D6/D7 decode attention over a contiguous (kvh, L, d) K/V (op-level variant): o (nh*d) bf16. */
int aha_hip_attn_decode(const void* q, const void* k, const void* v, void* o, int32_t nh, int32_t kvh, int32_t d,
                        int32_t L, float scale, void* stream);
/* Batched decode (aha_hip_generate_batch's kernels), op level.
 * aha_hip_gemv_rows: y[R, N] = x[R, K] . W[N, K]^T for 1 <= R <= 32, the weights read once (the step's projections of
 * /root/reference/src/models/qwen3/model.rs:79-86 for R sequences).  x (R, K) bf16, K % 8 == 0.  epi 0: y (R, N) bf16; 1: y = residual +
 * Linear (both bf16 (R, N), may alias); 2: SiLU(gate) * up with W in the 16-row gate / up block layout (N = 2I), y (R, I) bf16; 3: logits
 * (R, N) f32 and argmax_out (R) u32 (device), the first maximal index.  Each output row depends only on its own input row. */
int aha_hip_gemv_rows(const void* W, const void* x, void* y, int32_t R, int32_t N, int32_t K, int32_t epi, const void* residual,
                      float* logits, uint32_t* argmax_out, void* stream);
/* MXFP8 weight copies, op level.  A bf16 matrix W (N, K), K % 32 == 0, as OCP microscaling FP8: every row in blocks of 32 consecutive k;
 * per block e = the smallest integer in [-117, 120] with max |w| <= 448 * 2^e (an all-zero block: -117), the scale byte e + 127 (E8M0)
 * and q = e4m3fn(w / 2^e), round to nearest even, one byte per element; W' = q * 2^e is exact in bf16.
 * aha_hip_quantize_mxfp8: q_out (N, K) bytes; scales_out (N, ceil(K / 128)) u32, word (n, c) = the scale bytes of row n's blocks
 * 4c .. 4c + 3, block 4c + g in bits 8g .. 8g + 7 (bytes of blocks past K: 127); w_roundtrip_out (N, K) bf16 = W', may be NULL or W
 * itself.  The weights must be finite and below 1.9375 * 2^127 in magnitude (not checked here).
 * aha_hip_gemv_rows_mxfp8: aha_hip_gemv_rows with (q, scales) in place of W, K % 32 == 0: every output bit equals
 * aha_hip_gemv_rows on W'. */
int aha_hip_quantize_mxfp8(const void* W, int32_t N, int32_t K, void* q_out, uint32_t* scales_out, void* w_roundtrip_out, void* stream);
/* Batch-1 matvec with an epilogue, op level (the single-sequence decode step's kernels).  N counts MATRIX rows; epi as in
 * aha_hip_gemv_rows: 0 y (N) bf16; 1 y = residual + Linear (may alias); 2 SiLU(gate) * up with W in the 16-row gate / up block layout
 * (N = 2I, N % 32 == 0), y (I) bf16; 3 logits (N) f32 and *argmax_out (device u32) the first maximal index.  norm_w != NULL fuses
 * h = RMSNorm(x; norm_w, eps) in front.
 * aha_hip_gemv_epi: W (N, K) bf16, K % 8 == 0, K <= 32768 -- the kernel of aha_hip_gemv.
 * aha_hip_gemv_mxfp8: (q, scales) of aha_hip_quantize_mxfp8 in place of W, K % 32 == 0, K <= 32768.  The contract is bit identity: per
 * 512-k chunk a lane reads the same 8 k as the bf16 kernel (8 E4M3 bytes and their block's scale byte), byte * 2^e is exact in f32 and
 * equals the bf16 weight of W' = q * 2^e, and the fma order, wave reduction and rounding points are the bf16 kernel's, so every output
 * bit -- and the argmax -- equals aha_hip_gemv_epi on W'.  AHA_ERR_INVALID with a message, before anything is launched: a null q,
 * scales, x or output of the epilogue, K not a multiple of 32 or above 32768, N < 1, epi outside 0..3, epi 2 with N % 32 != 0. */
int aha_hip_gemv_epi(const void* W, const void* x, void* y, int32_t N, int32_t K, int32_t epi, const void* norm_w, float eps,
                     const void* residual, float* logits, uint32_t* argmax_out, void* stream);
int aha_hip_gemv_mxfp8(const void* q, const uint32_t* scales, const void* x, void* y, int32_t N, int32_t K, int32_t epi, const void* norm_w,
                       float eps, const void* residual, float* logits, uint32_t* argmax_out, void* stream);
int aha_hip_gemv_rows_mxfp8(const void* q, const uint32_t* scales, const void* x, void* y, int32_t R, int32_t N, int32_t K, int32_t epi,
                            const void* residual, float* logits, uint32_t* argmax_out, void* stream);
/* MXFP4 weight copies, op level.  A bf16 matrix W (N, K), K % 32 == 0, as OCP microscaling FP4: every row in blocks of 32 consecutive k.
 * Elements are OCP E2M1: the magnitudes {0, 0.5, 1, 1.5, 2, 3, 4, 6}, code = sign << 3 | index.  Per block e = the smallest integer in
 * [-125, 125] with max |w| <= 6 * 2^e (an all-zero block: -125) and the scale byte is e + 127 (E8M0) -- the no-saturation convention of
 * the MXFP8 path, not the OCP text's floor(log2 max |w|) - 2.  q = the code nearest to v = w / 2^e (exact), a tie to the even code:
 * 0.25 -> 0, 0.75 -> 1, 1.25 -> 1, 1.75 -> 2, 2.5 -> 2, 3.5 -> 4, 5 -> 4.  The sign bit is kept, so the code 0x8 (-0) occurs; gfx950's
 * conversion returns -0.0 for it, as W' holds.  W' = q * 2^e has two significant bits and is 0 or at least 2^-126 in magnitude: exact
 * in bf16.  |w' - w| <= max(|w| / 4, 2^(e - 2)); quantising W' gives W' again.
 * aha_hip_quantize_mxfp4: q_out (N, K / 2) bytes, byte (n, k / 2) holds even k in bits 0..3 and odd k in bits 4..7; scales_out as for
 * aha_hip_quantize_mxfp8 -- (N, ceil(K / 128)) u32, block 4c + g in bits 8g .. 8g + 7 of word (n, c), bytes of blocks past K: 127;
 * w_roundtrip_out (N, K) bf16 = W', may be NULL or W itself.  The weights must be finite and at most 1.5 * 2^127 in magnitude (beyond
 * it a weight would round past 6 * 2^125; not checked here).
 * aha_hip_gemv_rows_mxfp4: aha_hip_gemv_rows with (q, scales) in place of W, K % 32 == 0: every output bit equals aha_hip_gemv_rows on
 * W'.  Argument checks as for aha_hip_gemv_rows_mxfp8.
 * aha_hip_gemv_mxfp4: aha_hip_gemv_mxfp8 with (q, scales) of aha_hip_quantize_mxfp4, q rows of K / 2 bytes; it replaces running
 * aha_hip_gemv_epi on W' for a matrix kept as MXFP4.  The same contract: a lane reads the same 8 k of a 512-k chunk (one dword of 8 codes
 * and their block's scale byte), code * 2^e is exact in f32 and equals the bf16 weight of W', everything else is the bf16 kernel's, so
 * every output bit -- and the argmax -- equals aha_hip_gemv_epi on W'.  The same argument checks, messages prefixed "gemv_mxfp4:". */
int aha_hip_gemv_mxfp4(const void* q, const uint32_t* scales, const void* x, void* y, int32_t N, int32_t K, int32_t epi, const void* norm_w,
                       float eps, const void* residual, float* logits, uint32_t* argmax_out, void* stream);
/* Exact 13-bit copy of a bf16 matrix W (N, K), K a multiple of 4096 (device pointers).  A bf16 weight is s | E(8) | m(7); the copy keeps
 * its low byte (E & 1) | m and its sign verbatim and recodes E >> 1 to 4 bits with one base bh per matrix: code 0 means E >> 1 == 0
 * (+-0, subnormals, E = 1), code h = 1..15 means E >> 1 == bh + h, bh = max(0, max of E >> 1 over the finite weights - 15).  Rows in the
 * order of W, K / 4096 units of 6656 bytes per row; a unit holds one row x 4096 columns as four 1-KiB pieces of low bytes, two 1-KiB
 * pieces of codes and 512 bytes of signs, each lane-linear for the matvec (kernels_gemv_pk13.hip and aha_amd/quant.py pack_pk13 spell the
 * bit positions out).  aha_hip_pack_pk13 checks W first: *bad_out = the number of weights the format cannot hold (Inf, NaN, non-zero
 * values with E >> 1 <= bh); *bh_out = bh.  out (may be NULL: check only) receives N * (K / 4096) * 6656 bytes if *bad_out == 0 and
 * is left untouched otherwise.  Synchronises the stream.
 * aha_hip_gemv_pk13: aha_hip_gemv_epi with (packed, bh) in place of W; K a multiple of 4096, at most 32768.  The contract is bit
 * identity with aha_hip_gemv_epi on W, whatever either plan picks. */
int aha_hip_pack_pk13(const void* W, int32_t N, int32_t K, void* out, int32_t* bh_out, int64_t* bad_out, void* stream);
int aha_hip_gemv_pk13(const void* packed, int32_t bh, const void* x, void* y, int32_t N, int32_t K, int32_t epi, const void* norm_w,
                      float eps, const void* residual, float* logits, uint32_t* argmax_out, void* stream);
/* Exception rows.  Finite weights below the window do not keep a matrix from being packed as long as at most 16 rows of W hold one: the
 * copy has an arbitrary code at such a weight, and the matvec computes those rows from W itself (gemv_kernel_rows_pk13), still bit for bit
 * what aha_hip_gemv_epi gives on W.  Inf / NaN keep a matrix unpacked.
 * aha_hip_pack_pk13_rows: *nonfinite_out = the number of Inf / NaN, *below_out = the number of finite weights below the window,
 * *nrows_out = the number of rows that hold one (17 stands for "more than 16"), rows_out (host, cap entries, cap 0..16) = those rows
 * ascending, as many as fit, in W's own order (for a gate / up matrix: rows of the fused 16-row-alternating matrix).  out (may be NULL)
 * receives the copy if *nonfinite_out == 0 and *nrows_out <= cap and is left untouched otherwise.  Synchronises the stream.
 * aha_hip_gemv_pk13_rows: aha_hip_gemv_pk13 with the bf16 matrix W (device) and the row list (host, nrows 0..16, each a row of W);
 * nrows == 0 is aha_hip_gemv_pk13 and needs neither.  Messages prefixed "gemv_pk13_rows:". */
int aha_hip_pack_pk13_rows(const void* W, int32_t N, int32_t K, void* out, int32_t* bh_out, int32_t* rows_out, int32_t cap, int32_t* nrows_out,
                           int64_t* below_out, int64_t* nonfinite_out, void* stream);
int aha_hip_gemv_pk13_rows(const void* packed, int32_t bh, const void* W, const int32_t* rows, int32_t nrows, const void* x, void* y, int32_t N,
                           int32_t K, int32_t epi, const void* norm_w, float eps, const void* residual, float* logits, uint32_t* argmax_out,
                           void* stream);
int aha_hip_quantize_mxfp4(const void* W, int32_t N, int32_t K, void* q_out, uint32_t* scales_out, void* w_roundtrip_out, void* stream);
int aha_hip_gemv_rows_mxfp4(const void* q, const uint32_t* scales, const void* x, void* y, int32_t R, int32_t N, int32_t K, int32_t epi,
                            const void* residual, float* logits, uint32_t* argmax_out, void* stream);
/* aha_hip_attn_decode_batch: the fused decode attention block (QKNormAttention::forward, modules.rs:538-577, without o_proj) of `rows`
 * sequences in one launch.  qkv (rows, (nh + 2kvh) * 128) bf16; q_norm_w / k_norm_w (128) bf16; rope (rows, 128) f32 cos | sin, bf16
 * values; page_ptrs: device table of page addresses (pages of kvh K blocks then kvh V blocks, 16 KB each); row r's pages are
 * page_ptrs[page0[r]], ..., its new token goes to slot kv_len[r] - 1 (page0 / kv_len: HOST arrays).  o (rows, nh * 128) bf16. */
int aha_hip_attn_decode_batch(const void* qkv, const void* q_norm_w, const void* k_norm_w, const float* rope, const uint64_t* page_ptrs,
                              const int32_t* page0, const int32_t* kv_len, int32_t rows, int32_t nh, int32_t kvh, float eps, float scale,
                              void* o, void* stream);
/* Debug: the single-sequence fused decode attention kernel (the decode step's) on one sequence whose pages are page_ptrs[0 ..]. */
int aha_hip_debug_attn_decode_fused(const void* qkv, const void* q_norm_w, const void* k_norm_w, const float* rope, const uint64_t* page_ptrs,
                                    int32_t kv_len, int32_t nh, int32_t kvh, float eps, float scale, void* o, void* stream);
/* Test entry: the attention launches of a draft-and-verify decode step on pages of the caller.  The arguments, the row table
 * (splits from the row's own length, counters zeroed, one counter block per row, ctr_step 1) and the checks are
 * aha_hip_attn_decode_batch's; several rows may name the same page0 (a sequence's last token and its drafts, kv_len ascending by one).
 * form 0: the default launch, the append inside the attention (= aha_hip_attn_decode_batch).  form 1: the KV append of every row, then
 * the attention without its append -- the pair a step with drafts queues.  form 2: the KV append alone (o may be NULL).
 * AHA_ERR_INVALID, before any device work, for what aha_hip_attn_decode_batch refuses or a form outside 0 .. 2.  Synchronises the stream. */
int aha_hip_debug_attn_decode_rows(const void* qkv, const void* q_norm_w, const void* k_norm_w, const float* rope, const uint64_t* page_ptrs,
                                   const int32_t* page0, const int32_t* kv_len, int32_t rows, int32_t nh, int32_t kvh, float eps, float scale,
                                   void* o, int32_t form, void* stream);
/* Test entry: the accept step of draft-and-verify decoding.  argmax (device, rows uint32): the step's pick of every row; row_tok (HOST,
 * rows): every row's input token (a draft row's is its draft); seq_tab (HOST): per sequence {first row, drafts} (layout 0: a sequence's
 * rows are consecutive, generate_batch_spec's step) or {own row, first draft row, drafts} (layout 1: the engine's step).  out (device,
 * n_seqs x 18 uint32): {emitted count, last confirmed row, tokens[16]} per sequence; words behind the count are unspecified.  At most 15
 * drafts of a sequence are looked at.  AHA_ERR_INVALID, before any device work, for a null pointer, rows or n_seqs < 1, a layout outside
 * 0 .. 1, a negative draft count, or a sequence whose rows (with its drafts clamped to 15) are not all inside 0 .. rows - 1.
 * Synchronises the stream. */
int aha_hip_debug_spec_accept(const uint32_t* argmax, const int32_t* row_tok, int32_t rows, const int32_t* seq_tab, int32_t n_seqs,
                              int32_t layout, uint32_t* out, void* stream);
/* aha_hip_sample_rows: aha_hip_sample_candidates for R rows of f32 logits at once (the candidate step of
 * aha_hip_generate_batch_sampled), bit-identical per row to it.  logits (device, row r at logits + r * ld, V floats) are only read;
 * k (1..64), temperature, repeat_penalty: HOST arrays of R; context / context_offsets: HOST, row r's penalty context is
 * context[context_offsets[r] .. context_offsets[r + 1]) (duplicates and ids >= V allowed, as apply_repeat_penalty).  Device outputs:
 * vals_out / idx_out (R, 64) -- the first k[r] entries of row r in (value desc, index asc) order -- and ms_out (R, 2) = {max, sumexp}. */
int aha_hip_sample_rows(const float* logits, int64_t ld, int32_t R, int32_t V, const int32_t* k, const float* temperature,
                        const float* repeat_penalty, const uint32_t* context, const size_t* context_offsets, float* vals_out,
                        uint32_t* idx_out, float* ms_out, void* stream);
/* aha_hip_logprob_rows: the log-probability pass of aha_hip_generate_batch_logprobs for R rows of f32 logits (device, row r at
 * logits + r * ld, V floats, only read).  tokens (device, R): row r's emitted token; n_top (HOST, R, each 0 .. 20); out (device, R).
 * AHA_ERR_INVALID for R < 1, V < 1, ld < V, a null pointer or an n_top outside 0 .. 20, checked before anything touches the device. */
int aha_hip_logprob_rows(const float* logits, int64_t ld, int32_t R, int32_t V, const uint32_t* tokens, const int32_t* n_top,
                         aha_token_logprobs* out, void* stream);
/* aha_hip_sample_rows plus addends: adj_ids / adj_vals / adj_offsets are HOST; row r adds adj_vals[i] (finite or -inf) to the penalised
 * logit of adj_ids[i] for i in [adj_offsets[r], adj_offsets[r + 1]) -- ids distinct and < V, in any order (AHA_ERR_INVALID otherwise).
 * A row with no entries gives bit-identical outputs to aha_hip_sample_rows; a row whose every logit ends at -inf is unspecified. */
int aha_hip_sample_rows_adjusted(const float* logits, int64_t ld, int32_t R, int32_t V, const int32_t* k, const float* temperature,
                                 const float* repeat_penalty, const uint32_t* context, const size_t* context_offsets,
                                 const uint32_t* adj_ids, const float* adj_vals, const size_t* adj_offsets, float* vals_out,
                                 uint32_t* idx_out, float* ms_out, void* stream);
/* aha_hip_sample_rows_adjusted plus allowed-token masks (the definition is in the guided-decoding section): masks is DEVICE memory,
 * n_masks x ceil(V / 32) words, only read; mask_rows is HOST, R entries: the mask index of row r, or -1 for none.  adj_offsets may be
 * NULL (no addends).  A row without a mask gives bit-identical outputs to aha_hip_sample_rows_adjusted, and so does an all-ones mask;
 * entries past the number of allowed ids have value -inf; a row left without a finite logit is unspecified. */
int aha_hip_sample_rows_masked(const float* logits, int64_t ld, int32_t R, int32_t V, const int32_t* k, const float* temperature,
                               const float* repeat_penalty, const uint32_t* context, const size_t* context_offsets, const uint32_t* adj_ids,
                               const float* adj_vals, const size_t* adj_offsets, const uint32_t* masks, const int32_t* mask_rows,
                               float* vals_out, uint32_t* idx_out, float* ms_out, void* stream);
/* D7 prefill attention, causal with q position i attending to k positions <= kv_offset + i; q (S, nh*d),
 * k/v (L, kvh*d) token-major, L = kv_offset + S.  causal = 0 gives full (ViT / audio encoder) attention.  d = 128, or 64 with
 * nh == kvh (the Qwen3-ASR audio encoder's geometry). */
int aha_hip_attn_prefill(const void* q, const void* k, const void* v, void* o, int32_t S, int32_t L, int32_t nh,
                         int32_t kvh, int32_t d, int32_t kv_offset, int32_t causal, float scale, void* stream);
/* Test entry: the packed prefill attention over independent segments (AttnPrefillArgs::seg_tab, the engine's and generate_batch's launch),
 * causal, head_dim 128, q rows as given (already normed and rotated).  segs: n_seg host pairs {len, kv0}; segment j's q / o rows follow
 * segment j - 1's, and its cache -- kv0 + len token-major rows of k / v ((rows, kvh * 128) bf16 on the device), after segment j - 1's --
 * goes to pages of its own.  Row i of segment j sees cache positions 0 .. kv0 + i.  with_kv0: pass kv0 as AttnPrefillArgs::seg_kv0
 * (multiples of 64); 0: launch without it (every kv0 must be 0).  Synchronises the stream. */
int aha_hip_debug_attn_prefill_segs(const void* q, const void* k, const void* v, void* o, int32_t nh, int32_t kvh, const int32_t* segs,
                                    int32_t n_seg, int32_t with_kv0, float scale, void* stream);
/* Test entry: the rope stage of a prefill as the model runs it, on pages of the caller.  Stage 1: launch_rope_table into rope_tab
 * ((S, 128) bf16, cos[64] | sin[64] per row; always written).  Stage 2: launch_qknorm_rope with the paged destination, in one of the forms
 * below.  Device inputs: qkv (S, (nh + 2 kvh) * 128) bf16, q_norm_w / k_norm_w (128) bf16, pos (3, S) int32, axis_map (64) int32, inv_freq
 * (64) f32 -- used as given, not derived from a theta -- and page_ptrs, n_page_ptrs byte addresses of pages (kvh K blocks then kvh V
 * blocks) in memory the caller owns.  q_out (S, nh * 128) bf16 receives the q heads unless skip_q (never null: with AHA_ROPE_ROWS=0 the
 * per-element kernel writes it regardless).  kv_start: the cache position of row 0 (forms 0 - 2).  The packed form takes HOST arrays:
 * row_slot (S): the cache slot of every row, counted over the call's pages page_ptrs[0 .. n_pages), and page_rows (2 * n_pages): per page
 * its first row and row count (1 .. 64), as plan_packed_pass lays them out.  The two must agree (row page_rows[2p] + t in slot 64 p + t): each
 * is checked against the pages and rows of the call, not against the other, so a mismatch stays inside the caller's pages but puts K and
 * V of a row in different slots.  AHA_ERR_INVALID, before any device work, for a null pointer,
 * S < 1, d != 128, an unknown form, skip_q outside what the form's kernel takes, or slots / rows outside the page table or the call.
 * Synchronises the stream. */
#define AHA_ROPE_FORM_TABLE 0         /* kv_start_host = kv_start, rope_tab set: forward_initial_impl's call (S < 16: the per-element kernel) */
#define AHA_ROPE_FORM_NO_TABLE 1      /* the same without rope_tab: cos / sin computed in place */
#define AHA_ROPE_FORM_DEVICE_START 2  /* kv_start_host = -1, kv_start read from a device int: the per-element kernel whatever S is */
#define AHA_ROPE_FORM_PACKED 3        /* row_slot / page_rows / n_pages, rope_tab set, skip_q = 1: packed_layers' call */
int aha_hip_debug_prefill_rope(const void* qkv, const void* q_norm_w, const void* k_norm_w, const int32_t* pos, const int32_t* axis_map,
                               const float* inv_freq, const uint64_t* page_ptrs, int32_t n_page_ptrs, int32_t S, int32_t nh, int32_t kvh,
                               int32_t d, float eps, int32_t form, int32_t kv_start, int32_t skip_q, const int32_t* row_slot,
                               const int32_t* page_rows, int32_t n_pages, void* rope_tab, void* q_out, void* stream);
/* Test entry: launch_attn_prefill with q-norm + RoPE of Q inside the kernel's Q load (AttnPrefillArgs::q_norm_w / q_rope_tab / q_eps), over
 * pages of the caller: qkv as above (the RAW q heads are read, row pitch (nh + 2 kvh) * 128), rope_tab as aha_hip_debug_prefill_rope left
 * it, o (rows, nh * 128) bf16.  Causal.  n_seg == 0: one sequence, rows [0, S) at cache positions kv_offset .. of kv_total tokens on
 * page_ptrs[0 ..], and with S2 > 0 a second segment of rows [S, S + S2) at kv_offset2 / kv_total2 in the same launch
 * (AttnPrefillArgs::S2).  n_seg > 0: packed, segs = n_seg HOST triples {len, page0, kv0}, segment j's rows after segment j - 1's, its cache
 * positions 0 .. kv0 + len - 1 on page_ptrs[page0 ..]; with_kv0 passes the kv0 column as AttnPrefillArgs::seg_kv0 (multiples of 64), 0
 * launches without it (every kv0 0).  AHA_ERR_UNSUPPORTED, nothing launched, when attn_prefill_takes_qfuse says no for these arguments
 * (the 64-row form); AHA_ERR_INVALID, before any device work, for a null pointer, S < 1, d != 128, nh / kvh > 16 or a cache range past
 * the page table.  Synchronises the stream. */
int aha_hip_debug_prefill_attn_qfuse(const void* qkv, const void* q_norm_w, const void* rope_tab, const uint64_t* page_ptrs,
                                     int32_t n_page_ptrs, int32_t S, int32_t nh, int32_t kvh, int32_t d, float eps, float scale,
                                     int32_t kv_offset, int32_t kv_total, int32_t S2, int32_t kv_offset2, int32_t kv_total2,
                                     const int32_t* segs, int32_t n_seg, int32_t with_kv0, void* o, void* stream);
/* Test entries of the vision and audio towers' row kernels (tests/test_tower_rows_gpu.py): each launches the production launcher unchanged
 * on buffers and page pools of the caller, and returns AHA_ERR_INVALID before any device work for a null pointer, a non-positive size, a
 * width the kernel cannot cover, or a page-pointer array shorter than the pages the call writes.  Unless stated, pointers are device memory.
 *
 * LayerNorm rows (launch_layernorm_rows): y = LayerNorm(x; w, b, eps) over rows x dim bf16; dim a multiple of 8, at most 8192. */
int aha_hip_debug_layernorm_rows(const void* x, const void* w, const void* b, void* y, int64_t rows, int32_t dim, float eps, void* stream);
/* aha_hip_gemm with a LayerNorm of the finished rows riding on the call (GemmArgs::norm_w / norm_b / norm_out / norm_eps): norm_out (M, N)
 * bf16.  The norm runs inside the split-K reduce pass where the plan has one and takes the width, else as a launch of its own.  ldc == N,
 * N <= 8192, no gate+up epilogue.  Shares aha_hip_gemm's per-device scratch; aha_hip_debug_gemm_plan selects the plan. */
int aha_hip_debug_gemm_layernorm(const void* A, const void* W, void* C, int32_t M, int32_t N, int32_t K, int32_t lda, int32_t ldw, int32_t ldc,
                                 const void* bias, const void* residual, int32_t act, const void* norm_w, const void* norm_b, void* norm_out,
                                 float eps, void* stream);
/* The ViT's learned position embedding: the tower's host construction of the bilinear corner indices and f32 weights for the HOST grids
 * grid_thw (n_grids x {t, h, w}; h, w multiples of merge) into a G x G table, then launch_pos_embed_add on x (N, D) bf16 in place with
 * table (G * G, D) bf16.  idx_out (4, N) int32 and wt_out (4, N) f32 are HOST arrays that receive the tables.  N must be the rows the grids
 * describe, D a multiple of 8.  Synchronises the stream. */
int aha_hip_debug_vit_pos_embed(const uint32_t* grid_thw, int32_t n_grids, int32_t G, int32_t merge, const void* table, void* x, int64_t N,
                                int32_t D, int32_t* idx_out, float* wt_out, void* stream);
/* The ViT's rope stage: launch_vit_rope_table into cs_tab ((N, 36, 2) f32: bf16-rounded cos, sin), then launch_vit_rope_pack, with the
 * tower's host tables for the HOST grids.  qkv (N, 3 * nh * 72) bf16, inv_freq (18) f32, page_ptrs: n_page_ptrs byte addresses of pages
 * (nh K blocks of 64 x 96, then nh V blocks of 80 x 64) in memory the caller owns, at least one page per 64 rows of every (grid, frame).
 * q_out (N, nh, 96) bf16.  rowcol_out (N, 2), page_of_out (N), slot_of_out (N) are HOST int32 arrays that receive the tables.  hd must be
 * 72.  Synchronises the stream. */
int aha_hip_debug_vit_rope(const void* qkv, const uint32_t* grid_thw, int32_t n_grids, int32_t merge, const float* inv_freq,
                           const uint64_t* page_ptrs, int32_t n_page_ptrs, int64_t N, int32_t nh, int32_t hd, float* cs_tab, void* q_out,
                           int32_t* rowcol_out, int32_t* page_of_out, int32_t* slot_of_out, void* stream);
/* launch_scatter_rows: dst[rows[i], :] = src[i, :] (add 0) or bf16(dst + src) (add 1) for i < n; rows is a HOST array of indices below
 * dst_rows, D a multiple of 8.  Synchronises the stream. */
int aha_hip_debug_scatter_rows(void* dst, const void* src, const int32_t* rows, int64_t n, int64_t dst_rows, int32_t D, int32_t add, void* stream);
/* The audio tower's staging kernels, one entry each.
 * im2col1: feat (mels, ld) f32, chunks: C HOST triples {first column of the clip, its frames F, window index}; out (C * ceil(mels / 2) *
 * ceil(win / 2), 16) bf16.  Synchronises the stream.
 * im2col_nhwc: in (B, Hin, Win, Cin) bf16 -> out (B * ceil(Hin / 2) * ceil(Win / 2), 9 * Cin), Cin a multiple of 8.
 * tokens_gather: in (B, Fq, T, Cc) bf16 -> out (B * T, Cc * Fq).
 * sinus_pe_add: x (rows, d) bf16 in place, row r at position r % T.
 * kv_pack_generic: K / V heads at columns k_off / v_off of src (N, ld) bf16 -> pages of the caller (nh K blocks of 64 x hd, then nh V
 * blocks of hd x 64); slot_of: optional HOST array, the cache slot of every row (NULL: row n in slot n).  Synchronises the stream. */
int aha_hip_debug_audio_im2col1(const float* feat, int64_t ld, const int32_t* chunks, int32_t C, int32_t mels, int32_t win, void* out, void* stream);
int aha_hip_debug_im2col_nhwc(const void* in, void* out, int32_t B, int32_t Hin, int32_t Win, int32_t Cin, void* stream);
int aha_hip_debug_audio_tokens_gather(const void* in, void* out, int32_t B, int32_t Fq, int32_t T, int32_t Cc, void* stream);
int aha_hip_debug_sinus_pe_add(void* x, int64_t rows, int32_t d, int32_t T, void* stream);
int aha_hip_debug_kv_pack_generic(const void* src, int64_t ld, int32_t k_off, int32_t v_off, const uint64_t* page_ptrs, int32_t n_page_ptrs,
                                  int32_t N, int32_t nh, int32_t hd, const int32_t* slot_of, void* stream);
/* V0-pre, host arithmetic: img_smart_resize (src/utils/img_utils.rs:294-331) -- the size Qwen3VLProcessor::process_img
 * (qwen3vl/processor.rs:159-165) resizes an image to: multiples of `factor` (patch * merge = 32), area within
 * [min_pixels, max_pixels] (shortest_edge / longest_edge of the preprocessor config).  AHA_ERR_INVALID when the aspect ratio
 * exceeds 200, as the reference. */
int aha_hip_img_smart_resize(uint32_t h, uint32_t w, uint32_t factor, uint32_t min_pixels, uint32_t max_pixels, uint32_t* h_out,
                             uint32_t* w_out);
/* The video path's host arithmetic, host only (decoding and the swscale resize stay with the caller):
 *  - video_smart_resize (/root/reference/src/utils/video_utils.rs:9-59): the size get_video_data scales the frames to; factor =
 *    patch_size * merge_size, video_ratio = 16 (0 = none), min / max_pixels = the video preprocessor's shortest / longest edge
 *    (qwen3vl/processor.rs:496-505).  Errors carry the reference's messages.
 *  - the frame sampling of get_video_data (processor.rs:481-489,518-535): nframes (sizes the resize) and the sample interval;
 *    the kept frames are the decoded frames whose index is a multiple of the interval.
 *  - calculate_timestamps (processor.rs:283-307): one f32 second value per temporal patch; returns the count. */
int aha_hip_video_smart_resize(uint32_t num_frames, uint32_t h, uint32_t w, uint32_t temporal_factor, uint32_t factor, uint32_t min_pixels,
                               uint32_t max_pixels, uint32_t video_ratio, uint32_t* h_out, uint32_t* w_out);
int aha_hip_video_sample_frames(uint32_t total_frames, float rate, uint32_t fps, uint32_t min_frames, uint32_t max_frames,
                                uint32_t* nframes_out, uint32_t* interval_out);
int64_t aha_hip_video_timestamps(const uint32_t* frame_indices, size_t n, float fps, uint32_t t_merge_size, float* out, size_t cap);
/* V0-pre: DynamicImage::resize_exact(new_w, new_h, FilterType::CatmullRom) (qwen3vl/processor.rs:166) of an RGB8 image
 * (H, W, 3) in device memory into dst (new_h, new_w, 3), device.  Algorithm of crate image 0.25.10 imageops::resize as
 * restated in oracle/image_pre.py ([unverified] against the crate itself): vertical pass into f32, horizontal pass,
 * CatmullRom taps scaled by max(ratio, 1) and normalised, clamp, round half away from zero.  Synchronises the stream. */
int aha_hip_image_resize(const uint8_t* src_hwc, int32_t H, int32_t W, uint8_t* dst_hwc, int32_t new_h, int32_t new_w, void* stream);
/* Host-only debug views (no GPU work) of the tap tables the two pre-processing kernels use, so that the CPU test tier can
 * compare them bit for bit with the restatements: resize taps of one axis (left[n_out], count[n_out], weights concatenated,
 * returns their number) and the polyphase resampling taps (new_f x klen floats for rates already divided by their gcd). */
int aha_hip_debug_resize_taps(int32_t n_in, int32_t n_out, int32_t* left, int32_t* count, float* weights, int64_t weights_cap);
int64_t aha_hip_debug_resample_taps(int32_t orig, int32_t new_f, float* taps, int64_t cap, int32_t* width, int32_t* klen);
/* V0: one RGB8 image (H, W, 3) in device memory, H and W multiples of patch*merge -> the processor's pixel_values rows
 * ((H/patch)*(W/patch), 3*2*patch*patch) bf16 in merge-window order with the frame duplicated to T = 2
 * (/root/reference/src/models/qwen3vl/processor.rs:174-251; img_transform, /root/reference/src/utils/img_utils.rs:272-293). */
int aha_hip_image_to_patches(const uint8_t* img_hwc, void* out, int32_t H, int32_t W, int32_t patch, int32_t merge,
                             const float mean[3], const float std[3], void* stream);
/* The video counterpart (process_videos, /root/reference/src/models/qwen3vl/processor.rs:253-281): T RGB8 frames (T, H, W, 3) in
 * device memory, already sampled and resized (get_video_data's output) -> (ceil(T/2)*(H/patch)*(W/patch), 3*2*patch*patch) bf16
 * rows, a temporal patch = two consecutive frames (an odd last frame is repeated, processor.rs:176-186).  The normalisation
 * runs in bf16 op by op as the reference's does for videos (to_dtype, affine(1/255, 0), broadcast_sub, broadcast_div). */
int aha_hip_video_to_patches(const uint8_t* frames_thwc, void* out, int32_t T, int32_t H, int32_t W, int32_t patch, int32_t merge,
                             const float mean[3], const float std[3], void* stream);
/* A0: Whisper log-mel frontend on the GPU (extract_fbank_features, feature_extraction_whisper.rs:93-115): n_samples f32
 * device samples -> out (128, n_samples/160) f32 device (n_fft 400, hop 160, symmetric Hann, Slaney mel, log10, max-8 clamp,
 * (x+4)/4).  n_samples must be >= 401. */
int aha_hip_logmel(const float* samples, int64_t n_samples, float* out, void* stream);
/* aha_hip_logmel over n_clips clips in one launch pair: `samples` holds the clips back to back (device), clip j n_samples[j] (> 400,
 * host array) of them; out (128, sum F_j) f32 device, F_j = n_samples[j] / 160, clip j's frames in columns F_0 + .. + F_{j-1} on.  Each
 * clip's columns are bit-identical to aha_hip_logmel on that clip alone (its own max - 8 clamp). */
int aha_hip_logmel_batch(const float* samples, const int64_t* n_samples, size_t n_clips, float* out, void* stream);
/* A0-pre: resample_audio_from_vec_f32 (src/utils/audio_utils.rs:590-616), the step between the audio decoder and the
 * feature extractor on the Qwen3-ASR request path (qwen3_asr/processor.rs:76,85: 16 kHz, 1 channel): interleaved PCM f32
 * (n_frames x channels, host) -> mean over channels -> resample_simple (audio_utils.rs:247-255: sinc interpolation, Hann
 * window, lowpass_filter_width 6, rolloff 0.99; kernel :66-151, strided convolution :154-214) -> mono f32 at target_sr
 * (host).  Returns the number of output samples, min(ceil(new * n / orig), (n / orig + 1) * new) with orig / new the rates
 * divided by their gcd (n_frames itself when the rates are equal), or a negative status; out == NULL only queries it. */
int64_t aha_hip_audio_resample(aha_ctx* ctx, const float* pcm, int64_t n_frames, int32_t channels, int32_t orig_sr,
                               int32_t target_sr, float* out, int64_t out_cap);
/* Debug: audio embeddings of the last forward_initial (rows x output_dim floats). */
int aha_hip_debug_audio_embeds(aha_model* m, float* out, size_t n);
/* D11 greedy: first maximal index of an f32 vector. */
int aha_hip_argmax(const float* x, int64_t n, uint32_t* out_dev, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* AHA_HIP_H */
