//! `aha-hip`: the reference-side binding of `include/aha_hip.h`.
//!
//! * [`sys`] -- `extern "C"` declarations and `#[repr(C)]` mirrors of the header's structs (std only).
//! * [`Model`] -- a safe handle: lifecycle, `forward_initial` / `forward_step` / `clear_cache` / `stop_token_ids`, the
//!   device-resident greedy loop with a per-token callback (what a streaming generate loop needs), the sampled path's
//!   candidate query.
//! * feature `aha`: `impl InferenceModel for HipQwen3` (reference `src/models/common/mod.rs:25-45`), i.e. what
//!   `generate_generic` / `generate_stream_generic` (`src/models/common/generate.rs:87-368`) and the ASR loop
//!   (`src/models/qwen3_asr/generate.rs:130-186`) call.
//!
//! Never compiled in the repository's own build image (no Rust toolchain there) -- see Cargo.toml.

pub mod sys {
    use std::ffi::{c_char, c_void};

    #[repr(C)]
    pub struct AhaCtx {
        _p: [u8; 0],
    }
    #[repr(C)]
    pub struct AhaRng {
        _private: [u8; 0],
    }
    #[repr(C)]
    pub struct AhaModel {
        _p: [u8; 0],
    }
    #[repr(C)]
    pub struct AhaSampler {
        _p: [u8; 0],
    }
    #[repr(C)]
    pub struct AhaEngine {
        _p: [u8; 0],
    }
    /// ctypes mirror `aha_amd._lib.EngineConfig`.
    #[repr(C)]
    #[derive(Debug, Clone, Copy)]
    pub struct AhaEngineConfig {
        pub max_running: usize,
        pub kv_pages: usize,
        pub max_tokens_per_step: usize,
        pub prefill_chunk: usize,
    }
    /// ctypes mirror `aha_amd._lib.EngineEvent`.
    #[repr(C)]
    #[derive(Debug, Clone, Copy, Default)]
    pub struct AhaEngineEvent {
        pub req_id: u64,
        pub token: u32,
        pub flags: u32,
    }
    /// ctypes mirror `aha_amd._lib.EngineStats`.
    #[repr(C)]
    #[derive(Debug, Clone, Copy, Default)]
    pub struct AhaEngineStats {
        pub waiting: usize,
        pub running: usize,
        pub free_pages: usize,
        pub total_pages: usize,
    }
    pub const AHA_ENGINE_EV_FIRST: u32 = 1;
    pub const AHA_ENGINE_EV_STOP: u32 = 2;
    pub const AHA_ENGINE_EV_LENGTH: u32 = 4;
    pub const AHA_ENGINE_EV_CANCELLED: u32 = 8;

    pub const AHA_SAMPLE_HAS_TOP_P: u32 = 1;
    pub const AHA_SAMPLE_HAS_TOP_K: u32 = 2;
    pub const AHA_SAMPLE_NEED_LOGITS: i32 = 1;
    pub const AHA_WQ_NONE: i32 = 0;
    pub const AHA_WQ_MXFP8_E4M3: i32 = 1;
    pub const AHA_WQ_MXFP4_E2M1: i32 = 2;
    pub const AHA_WQ_LM_HEAD: u32 = 1;

    /// `aha_sampling_params`: the Options of `GenerationContext::new` (common/generate.rs:21-53); same fields, same order as the
    /// ctypes mirror `aha_amd._lib.SamplingParams`.
    #[repr(C)]
    #[derive(Debug, Clone, Copy)]
    pub struct AhaSamplingParams {
        pub temperature: f32,
        pub top_p: f32,
        pub top_k: i32,
        pub repeat_penalty: f32,
        pub repeat_last_n: i32,
        pub flags: u32,
        pub seed: u64,
    }

    pub const AHA_BF16: i32 = 0;
    pub const AHA_F16: i32 = 1;
    pub const AHA_F32: i32 = 2;
    pub const AHA_ARCH_QWEN3: i32 = 0;
    pub const AHA_ARCH_QWEN3VL: i32 = 1;
    pub const AHA_ARCH_QWEN3ASR: i32 = 2;

    /// `aha_model_desc` (field order and widths checked against the header by tests/test_host_cpu.py on the ctypes mirror)
    #[repr(C)]
    #[derive(Clone, Copy, Default)]
    pub struct AhaModelDesc {
        pub arch: i32,
        pub hidden_size: i32,
        pub intermediate_size: i32,
        pub num_hidden_layers: i32,
        pub num_attention_heads: i32,
        pub num_key_value_heads: i32,
        pub head_dim: i32,
        pub vocab_size: i32,
        pub rms_norm_eps: f32,
        pub rope_theta: f32,
        pub tie_word_embeddings: i32,
        pub mrope_section: [i32; 3],
        pub vis_depth: i32,
        pub vis_hidden_size: i32,
        pub vis_num_heads: i32,
        pub vis_intermediate_size: i32,
        pub vis_in_channels: i32,
        pub vis_patch_size: i32,
        pub vis_temporal_patch_size: i32,
        pub vis_spatial_merge_size: i32,
        pub vis_out_hidden_size: i32,
        pub vis_num_position_embeddings: i32,
        pub vis_deepstack_indexes: [i32; 8],
        pub vis_num_deepstack: i32,
        pub image_token_id: i32,
        pub video_token_id: i32,
        pub vision_start_token_id: i32,
        pub vision_end_token_id: i32,
        pub kv_reserve_tokens: i32,
        pub n_stop_tokens: i32,
        pub stop_tokens: [u32; 8],
        pub aud_d_model: i32,
        pub aud_encoder_layers: i32,
        pub aud_attention_heads: i32,
        pub aud_ffn_dim: i32,
        pub aud_num_mel_bins: i32,
        pub aud_downsample_hidden_size: i32,
        pub aud_output_dim: i32,
        pub aud_n_window: i32,
        pub audio_token_id: i32,
        pub tp_rank: i32,
        pub tp_size: i32,
        /// AHA_BF16 (0) is the only compute dtype; anything else makes `aha_hip_model_create` fail (AHA_ERR_UNSUPPORTED)
        pub compute_dtype: i32,
    }

    /// `aha_spec_config`: draft-and-verify decoding (aha_hip_generate_batch_spec)
    #[repr(C)]
    #[derive(Clone, Copy, Debug)]
    pub struct AhaSpecConfig {
        /// 1..15 draft tokens per sequence per step; 0 = speculation off
        pub max_draft: i32,
        pub ngram_min: i32,
        pub ngram_max: i32,
    }

    pub const AHA_MAX_TOP_LOGPROBS: usize = 20;

    /// `aha_token_logprobs`: one generated token's log-probability and its `n_top` most likely alternatives (`n_top` -1: the request
    /// asked for none and nothing else is written).  Temperature 1, before the repeat penalty, whatever the sampler.
    #[repr(C)]
    #[derive(Clone, Copy, Debug)]
    pub struct AhaTokenLogprobs {
        pub logprob: f32,
        pub n_top: i32,
        pub top_ids: [u32; AHA_MAX_TOP_LOGPROBS],
        pub top_logprobs: [f32; AHA_MAX_TOP_LOGPROBS],
    }
    impl Default for AhaTokenLogprobs {
        fn default() -> Self {
            Self { logprob: 0.0, n_top: -1, top_ids: [u32::MAX; AHA_MAX_TOP_LOGPROBS], top_logprobs: [f32::NEG_INFINITY; AHA_MAX_TOP_LOGPROBS] }
        }
    }

    pub const AHA_MAX_LOGIT_BIAS: usize = 1024;

    /// `aha_token_mask_fn`: asked once per live sequence per step for the sequence's allowed-token mask (`n_words` = ceil(V / 32) packed
    /// words in `mask_words`, holding its previous mask).  1: use them; 0: this step is unmasked; negative: the call fails.  Like the
    /// rest of this crate it has never been compiled here (no Rust toolchain): it is written against include/aha_hip.h by hand.
    pub type AhaTokenMaskFn =
        unsafe extern "C" fn(user: *mut c_void, seq: usize, generated: *const u32, n_generated: usize, mask_words: *mut u32, n_words: usize) -> i32;
    /// `aha_logit_adjust`: a request's `presence_penalty`, `frequency_penalty` and `logit_bias` (ids / values, `n_bias` of them; a value
    /// of -inf bans the token).  Both penalties 0 and `n_bias` 0: inactive.
    #[repr(C)]
    #[derive(Clone, Copy, Debug)]
    pub struct AhaLogitAdjust {
        pub presence_penalty: f32,
        pub frequency_penalty: f32,
        pub bias_ids: *const u32,
        pub bias_vals: *const f32,
        pub n_bias: usize,
    }
    impl Default for AhaLogitAdjust {
        fn default() -> Self {
            Self { presence_penalty: 0.0, frequency_penalty: 0.0, bias_ids: std::ptr::null(), bias_vals: std::ptr::null(), n_bias: 0 }
        }
    }

    /// `aha_spec_stats`
    #[repr(C)]
    #[derive(Clone, Copy, Debug, Default)]
    pub struct AhaSpecStats {
        pub decode_steps: usize,
        pub rows: usize,
        pub proposed: usize,
        pub accepted: usize,
    }

    /// `aha_tensor_view`
    #[repr(C)]
    pub struct AhaTensorView {
        pub name: *const c_char,
        pub data: *const c_void,
        pub dtype: i32,
        pub ndim: i32,
        pub shape: [i64; 5],
        pub on_device: i32,
    }

    /// `aha_mm_input`
    #[repr(C)]
    pub struct AhaMmInput {
        pub pixel_values: *const c_void,
        pub pixel_dtype: i32,
        pub n_patches: i64,
        pub image_grid_thw: *const u32,
        pub n_images: i32,
        pub audio_features: *const f32,
        pub n_frames: i64,
        pub audio_samples: *const f32,
        pub n_samples: i64,
        pub image_embeds: *const c_void,
        pub n_image_tokens: i64,
        pub pixel_values_video: *const c_void,
        pub n_patches_video: i64,
        pub video_grid_thw: *const u32,
        pub n_videos: i32,
    }
    impl AhaMmInput {
        pub fn empty() -> Self {
            Self {
                pixel_values: std::ptr::null(),
                pixel_dtype: AHA_F32,
                n_patches: 0,
                image_grid_thw: std::ptr::null(),
                n_images: 0,
                audio_features: std::ptr::null(),
                n_frames: 0,
                audio_samples: std::ptr::null(),
                n_samples: 0,
                image_embeds: std::ptr::null(),
                n_image_tokens: 0,
                pixel_values_video: std::ptr::null(),
                n_patches_video: 0,
                video_grid_thw: std::ptr::null(),
                n_videos: 0,
            }
        }
    }

    extern "C" {
        pub fn aha_hip_init(device: i32, out: *mut *mut AhaCtx) -> i32;
        pub fn aha_hip_shutdown(ctx: *mut AhaCtx);
        pub fn aha_hip_last_error() -> *const c_char;
        pub fn aha_hip_version() -> *const c_char;
        pub fn aha_hip_get_dtype(requested: i32, cfg_dtype: *const c_char, out: *mut i32) -> i32;
        pub fn aha_hip_check_dtype(dtype: i32) -> i32;
        pub fn aha_hip_model_create(
            ctx: *mut AhaCtx,
            desc: *const AhaModelDesc,
            weights: *const AhaTensorView,
            n_weights: usize,
            out: *mut *mut AhaModel,
        ) -> i32;
        /// config.json + generation_config.json + every *.safetensors of `dir`, parsed / mmapped by the library itself
        pub fn aha_hip_config_parse(dir: *const c_char, out: *mut AhaModelDesc) -> i32;
        pub fn aha_hip_config_torch_dtype(dir: *const c_char, out: *mut c_char, cap: usize) -> i32;
        pub fn aha_hip_model_load(ctx: *mut AhaCtx, dir: *const c_char, kv_reserve_tokens: usize, out: *mut *mut AhaModel) -> i32;
        pub fn aha_hip_model_destroy(m: *mut AhaModel);
        pub fn aha_hip_forward_initial(
            m: *mut AhaModel,
            ids: *const u32,
            n_ids: usize,
            seqlen_offset: usize,
            mm: *const AhaMmInput,
            logits_out: *mut f32,
            argmax_out: *mut u32,
        ) -> i32;
        pub fn aha_hip_forward_step(m: *mut AhaModel, token: u32, seqlen_offset: usize, logits_out: *mut f32, argmax_out: *mut u32) -> i32;
        pub fn aha_hip_clear_cache(m: *mut AhaModel) -> i32;
        pub fn aha_hip_stop_token_ids(m: *const AhaModel, out: *mut u32, cap: usize) -> i32;
        pub fn aha_hip_decode_greedy(m: *mut AhaModel, first_token: u32, seqlen_offset: usize, max_new: usize, tokens_out: *mut u32) -> i32;
        pub fn aha_hip_sample_candidates(
            m: *mut AhaModel,
            context: *const u32,
            n_context: usize,
            repeat_penalty: f32,
            temperature: f32,
            k: i32,
            vals_out: *mut f32,
            idx_out: *mut u32,
            max_out: *mut f32,
            sumexp_out: *mut f32,
        ) -> i32;
        pub fn aha_hip_last_logits(m: *mut AhaModel, logits_out: *mut f32) -> i32;
        pub fn aha_hip_rng_create(seed: u64, out: *mut *mut AhaRng) -> i32;
        pub fn aha_hip_rng_destroy(rng: *mut AhaRng);
        pub fn aha_hip_rng_next_u32(rng: *mut AhaRng) -> u32;
        pub fn aha_hip_rng_weighted_index(rng: *mut AhaRng, weights: *const f32, n: usize, index_out: *mut u32) -> i32;
        pub fn aha_hip_kv_export(m: *mut AhaModel, out_dev: *mut c_void, out_bytes: usize, bytes_needed: *mut usize, n_tokens: *mut usize, rope_delta: *mut i64) -> i32;
        pub fn aha_hip_kv_import(m: *mut AhaModel, in_dev: *const c_void, in_bytes: usize, src_heads: i32, src_head0: i32, dst_head0: i32, n_heads: i32, n_tokens: usize, rope_delta: i64) -> i32;
        pub fn aha_hip_set_gemm_reserved_cus(n: i32) -> i32;
        /// context-parallel prefill: full weights on every rank, the prompt's rows sharded, one K / V all-gather per layer
        pub fn aha_hip_tp_unique_id(out128: *mut c_void) -> i32;
        pub fn aha_hip_set_context_parallel(
            m: *mut AhaModel,
            rank: i32,
            world: i32,
            all_gather: Option<unsafe extern "C" fn(buf_dev: *mut c_void, bytes_per_rank: usize, user: *mut c_void) -> i32>,
            user: *mut c_void,
        ) -> i32;
        pub fn aha_hip_cp_init_rccl(m: *mut AhaModel, unique_id128: *const c_void) -> i32;
        pub fn aha_hip_embed(m: *mut AhaModel, ids: *const u32, n_ids: usize, out: *mut f32) -> i32;
        pub fn aha_hip_embed_batch(
            m: *mut AhaModel,
            ids: *const u32,
            seq_lens: *const usize,
            n_seqs: usize,
            max_tokens_per_pass: usize,
            out: *mut f32,
        ) -> i32;
        pub fn aha_hip_generate_batch(
            m: *mut AhaModel,
            ids: *const u32,
            seq_lens: *const usize,
            n_seqs: usize,
            max_new: usize,
            max_tokens_per_pass: usize,
            tokens_out: *mut u32,
            n_out: *mut usize,
            logits_out: *mut f32,
        ) -> i32;
        pub fn aha_hip_generate_batch_sampled(
            m: *mut AhaModel,
            ids: *const u32,
            seq_lens: *const usize,
            n_seqs: usize,
            params: *const AhaSamplingParams,
            max_new: usize,
            max_tokens_per_pass: usize,
            tokens_out: *mut u32,
            n_out: *mut usize,
            step_logits_out: *mut f32,
        ) -> i32;
        pub fn aha_hip_generate_batch_mm(
            m: *mut AhaModel,
            ids: *const u32,
            seq_lens: *const usize,
            n_seqs: usize,
            mm: *const *const AhaMmInput,
            params: *const AhaSamplingParams,
            max_new: usize,
            max_tokens_per_pass: usize,
            tokens_out: *mut u32,
            n_out: *mut usize,
            step_logits_out: *mut f32,
        ) -> i32;
        pub fn aha_hip_generate_batch_logprobs(
            m: *mut AhaModel,
            ids: *const u32,
            seq_lens: *const usize,
            n_seqs: usize,
            mm: *const *const AhaMmInput,
            params: *const AhaSamplingParams,
            top_logprobs: *const i32,
            max_new: usize,
            max_tokens_per_pass: usize,
            tokens_out: *mut u32,
            n_out: *mut usize,
            step_logits_out: *mut f32,
            logprobs_out: *mut AhaTokenLogprobs,
        ) -> i32;
        pub fn aha_hip_generate_batch_adjusted(
            m: *mut AhaModel,
            ids: *const u32,
            seq_lens: *const usize,
            n_seqs: usize,
            mm: *const *const AhaMmInput,
            params: *const AhaSamplingParams,
            adjust: *const AhaLogitAdjust,
            top_logprobs: *const i32,
            max_new: usize,
            max_tokens_per_pass: usize,
            tokens_out: *mut u32,
            n_out: *mut usize,
            step_logits_out: *mut f32,
            logprobs_out: *mut AhaTokenLogprobs,
        ) -> i32;
        pub fn aha_hip_generate_batch_masked(
            m: *mut AhaModel,
            ids: *const u32,
            seq_lens: *const usize,
            n_seqs: usize,
            mm: *const *const AhaMmInput,
            params: *const AhaSamplingParams,
            adjust: *const AhaLogitAdjust,
            top_logprobs: *const i32,
            max_new: usize,
            max_tokens_per_pass: usize,
            mask_fn: Option<AhaTokenMaskFn>,
            mask_user: *mut c_void,
            tokens_out: *mut u32,
            n_out: *mut usize,
            step_logits_out: *mut f32,
            logprobs_out: *mut AhaTokenLogprobs,
        ) -> i32;
        pub fn aha_hip_generate_batch_spec(
            m: *mut AhaModel,
            ids: *const u32,
            seq_lens: *const usize,
            n_seqs: usize,
            max_new: usize,
            max_tokens_per_pass: usize,
            spec: *const AhaSpecConfig,
            predictions: *const u32,
            prediction_lens: *const usize,
            tokens_out: *mut u32,
            n_out: *mut usize,
            logits_out: *mut f32,
            n_proposed: *mut usize,
            n_accepted: *mut usize,
            stats: *mut AhaSpecStats,
        ) -> i32;
        pub fn aha_hip_spec_propose(
            spec: *const AhaSpecConfig,
            context: *const u32,
            n_context: usize,
            n_prompt: usize,
            prediction: *const u32,
            n_prediction: usize,
            draft_out: *mut u32,
            n_draft: *mut usize,
        ) -> i32;
        pub fn aha_hip_engine_create(m: *mut AhaModel, cfg: *const AhaEngineConfig, out: *mut *mut AhaEngine) -> i32;
        pub fn aha_hip_engine_destroy(e: *mut AhaEngine);
        pub fn aha_hip_engine_submit(
            e: *mut AhaEngine,
            ids: *const u32,
            n_ids: usize,
            mm: *const AhaMmInput,
            params: *const AhaSamplingParams,
            max_new: usize,
            req_id: *mut u64,
        ) -> i32;
        pub fn aha_hip_engine_submit_logprobs(
            e: *mut AhaEngine,
            ids: *const u32,
            n_ids: usize,
            mm: *const AhaMmInput,
            params: *const AhaSamplingParams,
            max_new: usize,
            top_logprobs: i32,
            req_id: *mut u64,
        ) -> i32;
        pub fn aha_hip_engine_submit_adjusted(
            e: *mut AhaEngine,
            ids: *const u32,
            n_ids: usize,
            mm: *const AhaMmInput,
            params: *const AhaSamplingParams,
            adjust: *const AhaLogitAdjust,
            max_new: usize,
            top_logprobs: i32,
            req_id: *mut u64,
        ) -> i32;
        pub fn aha_hip_engine_submit_masked(
            e: *mut AhaEngine,
            ids: *const u32,
            n_ids: usize,
            mm: *const AhaMmInput,
            params: *const AhaSamplingParams,
            adjust: *const AhaLogitAdjust,
            mask_words: *const u32,
            n_mask_words: usize,
            max_new: usize,
            top_logprobs: i32,
            req_id: *mut u64,
        ) -> i32;
        pub fn aha_hip_engine_set_mask(e: *mut AhaEngine, req_id: u64, words: *const u32, n_words: usize) -> i32;
        pub fn aha_hip_engine_cancel(e: *mut AhaEngine, req_id: u64) -> i32;
        pub fn aha_hip_engine_step(e: *mut AhaEngine, ev: *mut AhaEngineEvent, cap: usize, n_ev: *mut usize, logits_out: *mut f32) -> i32;
        pub fn aha_hip_engine_step_logprobs(
            e: *mut AhaEngine,
            ev: *mut AhaEngineEvent,
            cap: usize,
            n_ev: *mut usize,
            logits_out: *mut f32,
            logprobs_out: *mut AhaTokenLogprobs,
        ) -> i32;
        pub fn aha_hip_engine_stats(e: *const AhaEngine, out: *mut AhaEngineStats) -> i32;
        pub fn aha_hip_engine_debug_ctr_base(e: *mut AhaEngine, base: u32) -> i32;
        pub fn aha_hip_engine_submit_spec(
            e: *mut AhaEngine,
            input_ids: *const u32,
            n_ids: usize,
            mm: *const AhaMmInput,
            max_new: usize,
            spec: *const AhaSpecConfig,
            prediction: *const u32,
            n_prediction: usize,
            req_id: *mut u64,
        ) -> i32;
        pub fn aha_hip_engine_max_events(e: *const AhaEngine) -> usize;
        pub fn aha_hip_engine_spec_stats(e: *const AhaEngine, out: *mut AhaSpecStats) -> i32;
        pub fn aha_hip_engine_request_spec(e: *const AhaEngine, req_id: u64, n_proposed: *mut usize, n_accepted: *mut usize) -> i32;
        pub fn aha_hip_logprob_rows(
            logits: *const f32,
            ld: i64,
            rows: i32,
            vocab: i32,
            tokens: *const u32,
            n_top: *const i32,
            out: *mut AhaTokenLogprobs,
            stream: *mut std::ffi::c_void,
        ) -> i32;
        pub fn aha_hip_sample_rows(
            logits: *const f32,
            ld: i64,
            rows: i32,
            vocab: i32,
            k: *const i32,
            temperature: *const f32,
            repeat_penalty: *const f32,
            context: *const u32,
            context_offsets: *const usize,
            vals_out: *mut f32,
            idx_out: *mut u32,
            ms_out: *mut f32,
            stream: *mut c_void,
        ) -> i32;
        pub fn aha_hip_sample_rows_adjusted(
            logits: *const f32,
            ld: i64,
            rows: i32,
            vocab: i32,
            k: *const i32,
            temperature: *const f32,
            repeat_penalty: *const f32,
            context: *const u32,
            context_offsets: *const usize,
            adj_ids: *const u32,
            adj_vals: *const f32,
            adj_offsets: *const usize,
            vals_out: *mut f32,
            idx_out: *mut u32,
            ms_out: *mut f32,
            stream: *mut c_void,
        ) -> i32;
        pub fn aha_hip_sample_rows_masked(
            logits: *const f32,
            ld: i64,
            rows: i32,
            vocab: i32,
            k: *const i32,
            temperature: *const f32,
            repeat_penalty: *const f32,
            context: *const u32,
            context_offsets: *const usize,
            adj_ids: *const u32,
            adj_vals: *const f32,
            adj_offsets: *const usize,
            masks: *const u32,
            mask_rows: *const i32,
            vals_out: *mut f32,
            idx_out: *mut u32,
            ms_out: *mut f32,
            stream: *mut c_void,
        ) -> i32;
        pub fn aha_hip_sampler_set_mask(s: *mut AhaSampler, words: *const u32, n_words: usize) -> i32;
        pub fn aha_hip_sampler_set_adjust(s: *mut AhaSampler, adjust: *const AhaLogitAdjust) -> i32;
        pub fn aha_hip_sampler_adjust_list(
            s: *mut AhaSampler,
            vocab_size: usize,
            generated: *const u32,
            n_generated: usize,
            ids_out: *mut u32,
            vals_out: *mut f32,
            cap: usize,
            n_out: *mut usize,
        ) -> i32;
        pub fn aha_hip_sampler_create(params: *const AhaSamplingParams, out: *mut *mut AhaSampler) -> i32;
        pub fn aha_hip_sampler_destroy(s: *mut AhaSampler);
        pub fn aha_hip_sampler_plan(
            s: *const AhaSampler,
            vocab_size: usize,
            n_generated: usize,
            k_out: *mut i32,
            temperature_out: *mut f32,
            repeat_penalty_out: *mut f32,
            n_context_out: *mut usize,
        ) -> i32;
        pub fn aha_hip_sampler_pick(
            s: *mut AhaSampler,
            vals: *const f32,
            idx: *const u32,
            k: i32,
            max: f32,
            sumexp: f32,
            logits: *const f32,
            vocab_size: usize,
            generated: *const u32,
            n_generated: usize,
            token_out: *mut u32,
        ) -> i32;
        pub fn aha_hip_sampler_rng_words(s: *const AhaSampler) -> u64;
        pub fn aha_hip_cache_len(m: *const AhaModel) -> usize;
        pub fn aha_hip_model_quantize_weights(m: *mut AhaModel, format: i32, flags: u32) -> i32;
        pub fn aha_hip_model_weight_format(m: *const AhaModel, format: *mut i32, flags: *mut u32) -> i32;
        pub fn aha_hip_debug_fp8_rows(m: *mut AhaModel, on: i32) -> i32;
        pub fn aha_hip_debug_fp8_single(m: *mut AhaModel, on: i32) -> i32;
        pub fn aha_hip_debug_plan_gemv_mxfp8(
            n: i32,
            k: i32,
            epi: i32,
            has_norm: i32,
            r: *mut i32,
            u: *mut i32,
            grid: *mut i32,
            form: *mut i32,
            by_plan: *mut i32,
        ) -> i32;
        pub fn aha_hip_debug_plan_gemv(
            n: i32,
            k: i32,
            epi: i32,
            has_norm: i32,
            r: *mut i32,
            u: *mut i32,
            grid: *mut i32,
            form: *mut i32,
        ) -> i32;
        pub fn aha_hip_debug_plan_gemv_rows(n: i32, k: i32, cw: *mut i32, nks: *mut i32) -> i32;
        pub fn aha_hip_debug_gemv_partial_f32(
            w: *const std::ffi::c_void,
            x: *const std::ffi::c_void,
            y_f32: *mut f32,
            n: i32,
            k: i32,
            norm_w: *const std::ffi::c_void,
            eps: f32,
            stream: *mut std::ffi::c_void,
        ) -> i32;
        pub fn aha_hip_gemv_epi(
            w: *const std::ffi::c_void,
            x: *const std::ffi::c_void,
            y: *mut std::ffi::c_void,
            n: i32,
            k: i32,
            epi: i32,
            norm_w: *const std::ffi::c_void,
            eps: f32,
            residual: *const std::ffi::c_void,
            logits: *mut f32,
            argmax_out: *mut u32,
            stream: *mut std::ffi::c_void,
        ) -> i32;
        pub fn aha_hip_gemv_mxfp8(
            q: *const std::ffi::c_void,
            scales: *const u32,
            x: *const std::ffi::c_void,
            y: *mut std::ffi::c_void,
            n: i32,
            k: i32,
            epi: i32,
            norm_w: *const std::ffi::c_void,
            eps: f32,
            residual: *const std::ffi::c_void,
            logits: *mut f32,
            argmax_out: *mut u32,
            stream: *mut std::ffi::c_void,
        ) -> i32;
        pub fn aha_hip_debug_fp4_single(m: *mut AhaModel, on: i32) -> i32;
        pub fn aha_hip_debug_plan_gemv_mxfp4(
            n: i32,
            k: i32,
            epi: i32,
            has_norm: i32,
            r: *mut i32,
            u: *mut i32,
            grid: *mut i32,
            form: *mut i32,
            by_plan: *mut i32,
        ) -> i32;
        pub fn aha_hip_gemv_mxfp4(
            q: *const std::ffi::c_void,
            scales: *const u32,
            x: *const std::ffi::c_void,
            y: *mut std::ffi::c_void,
            n: i32,
            k: i32,
            epi: i32,
            norm_w: *const std::ffi::c_void,
            eps: f32,
            residual: *const std::ffi::c_void,
            logits: *mut f32,
            argmax_out: *mut u32,
            stream: *mut std::ffi::c_void,
        ) -> i32;
        pub fn aha_hip_quantize_mxfp8(
            w: *const std::ffi::c_void,
            n: i32,
            k: i32,
            q_out: *mut std::ffi::c_void,
            scales_out: *mut u32,
            w_roundtrip_out: *mut std::ffi::c_void,
            stream: *mut std::ffi::c_void,
        ) -> i32;
        pub fn aha_hip_gemv_rows_mxfp8(
            q: *const std::ffi::c_void,
            scales: *const u32,
            x: *const std::ffi::c_void,
            y: *mut std::ffi::c_void,
            r: i32,
            n: i32,
            k: i32,
            epi: i32,
            residual: *const std::ffi::c_void,
            logits: *mut f32,
            argmax_out: *mut u32,
            stream: *mut std::ffi::c_void,
        ) -> i32;
        pub fn aha_hip_quantize_mxfp4(
            w: *const std::ffi::c_void,
            n: i32,
            k: i32,
            q_out: *mut std::ffi::c_void,
            scales_out: *mut u32,
            w_roundtrip_out: *mut std::ffi::c_void,
            stream: *mut std::ffi::c_void,
        ) -> i32;
        pub fn aha_hip_gemv_rows_mxfp4(
            q: *const std::ffi::c_void,
            scales: *const u32,
            x: *const std::ffi::c_void,
            y: *mut std::ffi::c_void,
            r: i32,
            n: i32,
            k: i32,
            epi: i32,
            residual: *const std::ffi::c_void,
            logits: *mut f32,
            argmax_out: *mut u32,
            stream: *mut std::ffi::c_void,
        ) -> i32;
        pub fn aha_hip_logmel_batch(
            samples: *const f32,
            n_samples: *const i64,
            n_clips: usize,
            out: *mut f32,
            stream: *mut std::ffi::c_void,
        ) -> i32;
        pub fn aha_hip_audio_resample(
            ctx: *mut AhaCtx,
            pcm: *const f32,
            n_frames: i64,
            channels: i32,
            orig_sr: i32,
            target_sr: i32,
            out: *mut f32,
            out_cap: i64,
        ) -> i64;
    }
}

use std::ffi::{c_char, c_void, CStr, CString};
use std::fmt;

/// Non-zero status of the library + its thread-local message (`aha_hip_last_error`)
#[derive(Debug, Clone)]
pub struct Error {
    pub code: i32,
    pub message: String,
}
impl fmt::Display for Error {
    fn fmt(&self, f: &mut fmt::Formatter<'_>) -> fmt::Result {
        write!(f, "aha_hip error {}: {}", self.code, self.message)
    }
}
impl std::error::Error for Error {}

/// Weight formats of `Model::quantize_weights` (`AHA_WQ_*` of include/aha_hip.h).
#[derive(Clone, Copy, Debug, PartialEq, Eq)]
#[repr(i32)]
pub enum WeightFormat {
    /// OCP microscaling FP8: E4M3 elements, one E8M0 scale per 32 consecutive k
    Mxfp8E4m3 = 1,
    /// OCP microscaling FP4: E2M1 elements, two to a byte, one E8M0 scale per 32 consecutive k.  Batched decode only: single-sequence
    /// decode of such a model runs the bf16 matvec on the dequantised matrices.
    Mxfp4E2m1 = 2,
}

fn check(rc: i32) -> Result<(), Error> {
    if rc >= 0 {
        return Ok(());
    }
    let message = unsafe { CStr::from_ptr(sys::aha_hip_last_error()) }.to_string_lossy().into_owned();
    Err(Error { code: rc, message })
}

/// `get_dtype(dtype, cfg_dtype)` of the reference (`src/utils/mod.rs:77-115`) with a `hip` arm: an explicit request wins,
/// otherwise the checkpoint's `torch_dtype`; bfloat16 stays bfloat16 (gfx950 computes in it natively).
pub fn get_dtype(requested: Option<i32>, cfg_dtype: &str) -> Result<i32, Error> {
    let c = CString::new(cfg_dtype).unwrap_or_default();
    let mut out = 0i32;
    check(unsafe { sys::aha_hip_get_dtype(requested.unwrap_or(-1), c.as_ptr(), &mut out) })?;
    Ok(out)
}

/// Multi-modal payload of `forward_initial` (host memory, borrowed for the call).
pub enum MmInput<'a> {
    None,
    /// Qwen3-VL: processor output `(n_patches, 1536)` f32 + `image_grid_thw` `(n_images, 3)` (qwen3vl/generate.rs:79-101)
    Image { pixel_values: &'a [f32], n_patches: usize, grid_thw: &'a [u32] },
    /// Qwen3-VL with videos: `data_vec[0..4]` = pixel_values, image_grid_thw, pixel_values_video, video_grid_thw, each pair
    /// optional (qwen3vl/model.rs:1292-1308); rows `(n, 1536)` f32, grids `(n, 3)`
    Vision { image: Option<(&'a [f32], usize, &'a [u32])>, video: Option<(&'a [f32], usize, &'a [u32])> },
    /// Qwen3-ASR: Whisper log-mel `(num_mel_bins, n_frames)` f32 (qwen3_asr/generate.rs:100-125)
    AudioFeatures { features: &'a [f32], n_frames: usize },
    /// Qwen3-ASR: raw 16 kHz mono samples; the library computes the log-mel features on the GPU
    AudioSamples { samples: &'a [f32] },
}

/// One model on one GPU.  Not thread-safe by contract (the reference takes `&mut self` everywhere and a write lock per request).
/// The Whisper log-mel of many clips in one launch pair (aha_hip_logmel_batch): `samples` = the clips back to back in device memory,
/// `n_samples[j]` (> 400) of clip j; `out` = a device (128, sum F_j) f32 buffer, F_j = n_samples[j] / 160, clip j's frames in its own
/// columns, each clip bit-identical to its own aha_hip_logmel.
///
/// # Safety
/// `samples` and `out` must be device buffers of at least the sizes above, `stream` a HIP stream of their device or null.
pub unsafe fn logmel_batch(samples: *const f32, n_samples: &[i64], out: *mut f32, stream: *mut std::ffi::c_void) -> Result<(), Error> {
    check(sys::aha_hip_logmel_batch(samples, n_samples.as_ptr(), n_samples.len(), out, stream))
}

/// A request's `logit_bias` (`bias_ids[i]` -> `bias_vals[i]`; -inf bans the token), `presence_penalty` and `frequency_penalty`
/// (aha_logit_adjust).  `Default` is the inactive adjust.  A server maps the chat request's `logit_bias: {"id": bias}` object by
/// parsing each key as a token id.
#[derive(Clone, Debug, Default)]
pub struct LogitAdjust {
    pub presence_penalty: f32,
    pub frequency_penalty: f32,
    pub bias_ids: Vec<u32>,
    pub bias_vals: Vec<f32>,
}
impl LogitAdjust {
    /// The C view; it borrows the two vectors (an entry without its value is left out).
    pub fn as_c(&self) -> sys::AhaLogitAdjust {
        sys::AhaLogitAdjust {
            presence_penalty: self.presence_penalty,
            frequency_penalty: self.frequency_penalty,
            bias_ids: self.bias_ids.as_ptr(),
            bias_vals: self.bias_vals.as_ptr(),
            n_bias: self.bias_ids.len().min(self.bias_vals.len()),
        }
    }
}

pub struct Model {
    ctx: *mut sys::AhaCtx,
    model: *mut sys::AhaModel,
    vocab: usize,
    hidden: usize,
    stop: Vec<u32>,
}
unsafe impl Send for Model {}

impl Model {
    /// `XxxGenerateModel::init(path, ..)` minus tokenizer / chat template: the library parses `config.json` /
    /// `generation_config.json` and mmaps every `*.safetensors` of `dir` (qwen3/generate.rs:22-50, utils/mod.rs:121-137).
    /// `dtype`: the resolved `Option<DType>` of `init` as an `aha_dtype` code; anything but bf16 is refused, loudly.
    pub fn from_dir(dir: &str, device: i32, dtype: Option<i32>) -> Result<Self, Error> {
        let c = CString::new(dir).map_err(|_| Error { code: -1, message: "path contains NUL".into() })?;
        let mut desc = sys::AhaModelDesc::default();
        check(unsafe { sys::aha_hip_config_parse(c.as_ptr(), &mut desc) })?;
        // get_dtype(dtype, cfg_dtype) exactly as XxxGenerateModel::init resolves it (utils/mod.rs:77-115): an explicit request wins,
        // otherwise the checkpoint's own dtype string decides -- and whatever comes out must be a dtype the kernels compute in, so
        // a float16 / float32 checkpoint with `dtype == None` is REFUSED here instead of silently running in bf16
        let mut buf = [0 as c_char; 64];
        check(unsafe { sys::aha_hip_config_torch_dtype(c.as_ptr(), buf.as_mut_ptr(), buf.len()) })?;
        let cfg_dtype = unsafe { CStr::from_ptr(buf.as_ptr()) }.to_string_lossy().into_owned();
        let resolved = get_dtype(dtype, &cfg_dtype)?;
        check(unsafe { sys::aha_hip_check_dtype(resolved) })?;
        let mut ctx = std::ptr::null_mut();
        check(unsafe { sys::aha_hip_init(device, &mut ctx) })?;
        let mut model = std::ptr::null_mut();
        if let Err(e) = check(unsafe { sys::aha_hip_model_load(ctx, c.as_ptr(), 0, &mut model) }) {
            unsafe { sys::aha_hip_shutdown(ctx) };
            return Err(e);
        }
        let mut stop = vec![0u32; 8];
        let n = unsafe { sys::aha_hip_stop_token_ids(model, stop.as_mut_ptr(), 8) };
        stop.truncate(n.clamp(0, 8) as usize);
        Ok(Self { ctx, model, vocab: desc.vocab_size as usize, hidden: desc.hidden_size as usize, stop })
    }

    /// From tensors the caller already holds (e.g. the mmapped safetensors views `VarBuilder::from_mmaped_safetensors` opens):
    /// `(HF name, bytes, aha_dtype, shape)`; copied to HBM, never aliased.
    pub fn from_tensors(desc: &sys::AhaModelDesc, tensors: &[(String, &[u8], i32, Vec<usize>)], device: i32) -> Result<Self, Error> {
        let names: Vec<CString> = tensors.iter().map(|t| CString::new(t.0.as_str()).unwrap_or_default()).collect();
        let views: Vec<sys::AhaTensorView> = tensors
            .iter()
            .zip(&names)
            .map(|(t, n)| {
                let mut shape = [0i64; 5];
                for (i, s) in t.3.iter().take(5).enumerate() {
                    shape[i] = *s as i64;
                }
                sys::AhaTensorView { name: n.as_ptr(), data: t.1.as_ptr() as *const _, dtype: t.2, ndim: t.3.len() as i32, shape, on_device: 0 }
            })
            .collect();
        let mut ctx = std::ptr::null_mut();
        check(unsafe { sys::aha_hip_init(device, &mut ctx) })?;
        let mut model = std::ptr::null_mut();
        if let Err(e) = check(unsafe { sys::aha_hip_model_create(ctx, desc, views.as_ptr(), views.len(), &mut model) }) {
            unsafe { sys::aha_hip_shutdown(ctx) };
            return Err(e);
        }
        let n = desc.n_stop_tokens.clamp(0, 8) as usize;
        Ok(Self { ctx, model, vocab: desc.vocab_size as usize, hidden: desc.hidden_size as usize, stop: desc.stop_tokens[..n].to_vec() })
    }

    pub fn vocab_size(&self) -> usize {
        self.vocab
    }
    pub fn stop_token_ids(&self) -> Vec<u32> {
        self.stop.clone()
    }
    pub fn cache_len(&self) -> usize {
        unsafe { sys::aha_hip_cache_len(self.model) }
    }

    /// `InferenceModel::forward_initial`: logits of the LAST prompt position (V floats) and their first-max arg-max.
    /// `logits = None` skips the 608 KB device-to-host copy (greedy requests, or the sampled path via `sample_candidates`).
    pub fn forward_initial(&mut self, ids: &[u32], seqlen_offset: usize, mm: MmInput<'_>, logits: Option<&mut [f32]>) -> Result<u32, Error> {
        let mut c = sys::AhaMmInput::empty();
        let mm_ptr: *const sys::AhaMmInput = match mm {
            MmInput::None => std::ptr::null(),
            MmInput::Image { pixel_values, n_patches, grid_thw } => {
                c.pixel_values = pixel_values.as_ptr() as *const _;
                c.pixel_dtype = sys::AHA_F32;
                c.n_patches = n_patches as i64;
                c.image_grid_thw = grid_thw.as_ptr();
                c.n_images = (grid_thw.len() / 3) as i32;
                &c
            }
            MmInput::Vision { image, video } => {
                c.pixel_dtype = sys::AHA_F32;
                if let Some((pv, n, grid)) = image {
                    c.pixel_values = pv.as_ptr() as *const _;
                    c.n_patches = n as i64;
                    c.image_grid_thw = grid.as_ptr();
                    c.n_images = (grid.len() / 3) as i32;
                }
                if let Some((pv, n, grid)) = video {
                    c.pixel_values_video = pv.as_ptr() as *const _;
                    c.n_patches_video = n as i64;
                    c.video_grid_thw = grid.as_ptr();
                    c.n_videos = (grid.len() / 3) as i32;
                }
                &c
            }
            MmInput::AudioFeatures { features, n_frames } => {
                c.audio_features = features.as_ptr();
                c.n_frames = n_frames as i64;
                &c
            }
            MmInput::AudioSamples { samples } => {
                c.audio_samples = samples.as_ptr();
                c.n_samples = samples.len() as i64;
                &c
            }
        };
        let lp = match logits {
            Some(l) => {
                assert!(l.len() >= self.vocab);
                l.as_mut_ptr()
            }
            None => std::ptr::null_mut(),
        };
        let mut am = 0u32;
        check(unsafe { sys::aha_hip_forward_initial(self.model, ids.as_ptr(), ids.len(), seqlen_offset, mm_ptr, lp, &mut am) })?;
        Ok(am)
    }

    /// `InferenceModel::forward_step` for the `(1, 1)` token tensor of a decode step.
    pub fn forward_step(&mut self, token: u32, seqlen_offset: usize, logits: Option<&mut [f32]>) -> Result<u32, Error> {
        let lp = match logits {
            Some(l) => {
                assert!(l.len() >= self.vocab);
                l.as_mut_ptr()
            }
            None => std::ptr::null_mut(),
        };
        let mut am = 0u32;
        check(unsafe { sys::aha_hip_forward_step(self.model, token, seqlen_offset, lp, &mut am) })?;
        Ok(am)
    }

    pub fn clear_cache(&mut self) {
        unsafe { sys::aha_hip_clear_cache(self.model) };
    }

    /// Quantise the layer matrices (and `lm_head` with `lm_head = true`; the embedding table when tied) to block-scaled FP8 in place
    /// (`aha_hip_model_quantize_weights`): the batched decode then streams 1.03 bytes per weight instead of 2, with the bits it would
    /// compute from the dequantised bf16 matrices, which every other path goes on reading.  Single-sequence decode (`forward_step`,
    /// `decode_greedy`, the generate loops) reads the copies too where that measured faster (matrices of 2^24 elements or more in the kernel's FAST form), bit-identical
    /// to the bf16 matvec.  `WeightFormat::Mxfp4E2m1` keeps E2M1 nibbles instead, 0.53 bytes per weight; its single-sequence decode
    /// has a kernel of its own (`gemv_mxfp4_kernel`, bit-identical again) under the switch `debug_fp4_single`.  Needs an empty cache
    /// and no engine.
    pub fn quantize_weights(&mut self, format: WeightFormat, lm_head: bool) -> Result<(), Error> {
        let flags = if lm_head { sys::AHA_WQ_LM_HEAD } else { 0 };
        check(unsafe { sys::aha_hip_model_quantize_weights(self.model, format as i32, flags) })
    }

    /// The single-sequence matvec of a model with MXFP4 copies (`aha_hip_debug_fp4_single`): 0 the bf16 kernel on the dequantised
    /// matrices, 1 (the default) the FP4 kernel on the matrices its plan takes, 2 on every matrix with a copy.  The same bits in all three.
    pub fn debug_fp4_single(&mut self, on: i32) -> Result<(), Error> {
        check(unsafe { sys::aha_hip_debug_fp4_single(self.model, on) })
    }

    /// `None`, or the format and the `lm_head` flag `quantize_weights` was called with.
    pub fn weight_format(&self) -> Result<Option<(WeightFormat, bool)>, Error> {
        let (mut f, mut fl) = (0i32, 0u32);
        check(unsafe { sys::aha_hip_model_weight_format(self.model, &mut f, &mut fl) })?;
        let lm_head = fl & sys::AHA_WQ_LM_HEAD != 0;
        Ok(match f {
            sys::AHA_WQ_MXFP8_E4M3 => Some((WeightFormat::Mxfp8E4m3, lm_head)),
            sys::AHA_WQ_MXFP4_E2M1 => Some((WeightFormat::Mxfp4E2m1, lm_head)),
            _ => None,
        })
    }

    /// `Qwen3Embedding::embed_one` (qwen3_embedding/mod.rs:50-64) of every sequence, computed as packed prefills
    /// (`aha_hip_embed_batch`): row `j` of the `(seqs.len(), hidden)` result is sequence `j`'s L2-normalised embedding.
    /// `max_tokens_per_pass = 0` takes the library default.
    pub fn embed_batch(&mut self, seqs: &[&[u32]], max_tokens_per_pass: usize) -> Result<Vec<f32>, Error> {
        let ids: Vec<u32> = seqs.iter().flat_map(|s| s.iter().copied()).collect();
        let lens: Vec<usize> = seqs.iter().map(|s| s.len()).collect();
        let mut out = vec![0f32; seqs.len() * self.hidden];
        check(unsafe {
            sys::aha_hip_embed_batch(self.model, ids.as_ptr(), lens.as_ptr(), lens.len(), max_tokens_per_pass, out.as_mut_ptr())
        })?;
        Ok(out)
    }

    /// `generate_generic` at temperature 0 for every prompt at once (aha_hip_generate_batch): per prompt, the greedy tokens it
    /// yields alone, ending at (and keeping) the first stop token after the first token.  The cache is empty afterwards.
    pub fn generate_batch(&mut self, prompts: &[&[u32]], max_new: usize, max_tokens_per_pass: usize) -> Result<Vec<Vec<u32>>, Error> {
        let ids: Vec<u32> = prompts.iter().flat_map(|s| s.iter().copied()).collect();
        let lens: Vec<usize> = prompts.iter().map(|s| s.len()).collect();
        let mut toks = vec![0u32; prompts.len() * max_new.max(1)];
        let mut n_out = vec![0usize; prompts.len()];
        check(unsafe {
            sys::aha_hip_generate_batch(
                self.model,
                ids.as_ptr(),
                lens.as_ptr(),
                lens.len(),
                max_new,
                max_tokens_per_pass,
                toks.as_mut_ptr(),
                n_out.as_mut_ptr(),
                std::ptr::null_mut(),
            )
        })?;
        Ok(n_out.iter().enumerate().map(|(j, &n)| toks[j * max_new..j * max_new + n].to_vec()).collect())
    }

    /// `generate_batch` with draft-and-verify decoding (aha_hip_generate_batch_spec): the same tokens, bit for bit, in fewer decode
    /// steps when the drafts are right.  `predictions`: `None`, or per prompt its predicted output (the request's `prediction`,
    /// params/chat.rs:105; an empty slice = none for that prompt).  Returns the token lists, per prompt (proposed, accepted) draft
    /// tokens -- `accepted_prediction_tokens` = accepted, `rejected_prediction_tokens` = proposed - accepted (params/shared.rs:58-63)
    /// -- and the call's statistics.
    pub fn generate_batch_spec(
        &mut self,
        prompts: &[&[u32]],
        max_new: usize,
        max_tokens_per_pass: usize,
        spec: sys::AhaSpecConfig,
        predictions: Option<&[&[u32]]>,
    ) -> Result<(Vec<Vec<u32>>, Vec<(usize, usize)>, sys::AhaSpecStats), Error> {
        if let Some(p) = predictions {
            if p.len() != prompts.len() {
                return Err(Error { code: -1, message: format!("{} predictions for {} prompts", p.len(), prompts.len()) });
            }
        }
        let ids: Vec<u32> = prompts.iter().flat_map(|s| s.iter().copied()).collect();
        let lens: Vec<usize> = prompts.iter().map(|s| s.len()).collect();
        // one spare id keeps the pointer non-null when every prediction is empty
        let pred_ids: Vec<u32> = predictions.map(|p| p.iter().flat_map(|s| s.iter().copied()).chain(std::iter::once(0)).collect()).unwrap_or_default();
        let pred_lens: Vec<usize> = predictions.map(|p| p.iter().map(|s| s.len()).collect()).unwrap_or_default();
        let mut toks = vec![0u32; prompts.len() * max_new.max(1)];
        let mut n_out = vec![0usize; prompts.len()];
        let mut proposed = vec![0usize; prompts.len()];
        let mut accepted = vec![0usize; prompts.len()];
        let mut stats = sys::AhaSpecStats::default();
        check(unsafe {
            sys::aha_hip_generate_batch_spec(
                self.model,
                ids.as_ptr(),
                lens.as_ptr(),
                lens.len(),
                max_new,
                max_tokens_per_pass,
                &spec,
                if predictions.is_some() { pred_ids.as_ptr() } else { std::ptr::null() },
                if predictions.is_some() { pred_lens.as_ptr() } else { std::ptr::null() },
                toks.as_mut_ptr(),
                n_out.as_mut_ptr(),
                std::ptr::null_mut(),
                proposed.as_mut_ptr(),
                accepted.as_mut_ptr(),
                &mut stats,
            )
        })?;
        let out = n_out.iter().enumerate().map(|(j, &n)| toks[j * max_new..j * max_new + n].to_vec()).collect();
        Ok((out, proposed.into_iter().zip(accepted).collect(), stats))
    }

    /// `generate_generic` with each prompt's own sampler, every prompt at once (aha_hip_generate_batch_sampled): per prompt, the
    /// tokens `generate_generic` yields for it alone with `GenerationContext(params[j])`, each on its own RNG stream.
    pub fn generate_batch_sampled(
        &mut self,
        prompts: &[&[u32]],
        params: &[sys::AhaSamplingParams],
        max_new: usize,
        max_tokens_per_pass: usize,
    ) -> Result<Vec<Vec<u32>>, Error> {
        if params.len() != prompts.len() {
            return Err(Error { code: -1, message: format!("{} sampling params for {} prompts", params.len(), prompts.len()) });
        }
        let ids: Vec<u32> = prompts.iter().flat_map(|s| s.iter().copied()).collect();
        let lens: Vec<usize> = prompts.iter().map(|s| s.len()).collect();
        let mut toks = vec![0u32; prompts.len() * max_new.max(1)];
        let mut n_out = vec![0usize; prompts.len()];
        check(unsafe {
            sys::aha_hip_generate_batch_sampled(
                self.model,
                ids.as_ptr(),
                lens.as_ptr(),
                lens.len(),
                params.as_ptr(),
                max_new,
                max_tokens_per_pass,
                toks.as_mut_ptr(),
                n_out.as_mut_ptr(),
                std::ptr::null_mut(),
            )
        })?;
        Ok(n_out.iter().enumerate().map(|(j, &n)| toks[j * max_new..j * max_new + n].to_vec()).collect())
    }

    /// `generate_generic` for many Qwen3-VL requests with their images / videos, or Qwen3-ASR requests with their audio clips, every
    /// request at once (aha_hip_generate_batch_mm): `mm[j]` is request j's payload (`MmInput::None` for a text request; `Image` /
    /// `Vision` / `AudioFeatures` / `AudioSamples` otherwise), `params` `None` = every request greedy, else one sampler per request.
    /// Per request, the tokens `generate_generic` yields for it alone with its data.
    pub fn generate_batch_mm(
        &mut self,
        prompts: &[&[u32]],
        mm: &[MmInput<'_>],
        params: Option<&[sys::AhaSamplingParams]>,
        max_new: usize,
        max_tokens_per_pass: usize,
    ) -> Result<Vec<Vec<u32>>, Error> {
        if mm.len() != prompts.len() {
            return Err(Error { code: -1, message: format!("{} multi-modal inputs for {} prompts", mm.len(), prompts.len()) });
        }
        if let Some(p) = params {
            if p.len() != prompts.len() {
                return Err(Error { code: -1, message: format!("{} sampling params for {} prompts", p.len(), prompts.len()) });
            }
        }
        let mut cs: Vec<sys::AhaMmInput> = Vec::with_capacity(mm.len());
        let mut present: Vec<bool> = Vec::with_capacity(mm.len());
        for x in mm {
            let mut c = sys::AhaMmInput::empty();
            let some = match *x {
                MmInput::None => false,
                MmInput::Image { pixel_values, n_patches, grid_thw } => {
                    c.pixel_values = pixel_values.as_ptr() as *const _;
                    c.pixel_dtype = sys::AHA_F32;
                    c.n_patches = n_patches as i64;
                    c.image_grid_thw = grid_thw.as_ptr();
                    c.n_images = (grid_thw.len() / 3) as i32;
                    true
                }
                MmInput::Vision { image, video } => {
                    c.pixel_dtype = sys::AHA_F32;
                    if let Some((pv, n, grid)) = image {
                        c.pixel_values = pv.as_ptr() as *const _;
                        c.n_patches = n as i64;
                        c.image_grid_thw = grid.as_ptr();
                        c.n_images = (grid.len() / 3) as i32;
                    }
                    if let Some((pv, n, grid)) = video {
                        c.pixel_values_video = pv.as_ptr() as *const _;
                        c.n_patches_video = n as i64;
                        c.video_grid_thw = grid.as_ptr();
                        c.n_videos = (grid.len() / 3) as i32;
                    }
                    true
                }
                MmInput::AudioFeatures { features, n_frames } => {
                    c.audio_features = features.as_ptr();
                    c.n_frames = n_frames as i64;
                    true
                }
                MmInput::AudioSamples { samples } => {
                    c.audio_samples = samples.as_ptr();
                    c.n_samples = samples.len() as i64;
                    true
                }
            };
            cs.push(c);
            present.push(some);
        }
        // (cs is complete: the pointers below stay valid for the call)
        let ptrs: Vec<*const sys::AhaMmInput> =
            cs.iter().zip(present.iter()).map(|(c, &p)| if p { c as *const sys::AhaMmInput } else { std::ptr::null() }).collect();
        let ids: Vec<u32> = prompts.iter().flat_map(|s| s.iter().copied()).collect();
        let lens: Vec<usize> = prompts.iter().map(|s| s.len()).collect();
        let mut toks = vec![0u32; prompts.len() * max_new.max(1)];
        let mut n_out = vec![0usize; prompts.len()];
        check(unsafe {
            sys::aha_hip_generate_batch_mm(
                self.model,
                ids.as_ptr(),
                lens.as_ptr(),
                lens.len(),
                ptrs.as_ptr(),
                params.map_or(std::ptr::null(), |p| p.as_ptr()),
                max_new,
                max_tokens_per_pass,
                toks.as_mut_ptr(),
                n_out.as_mut_ptr(),
                std::ptr::null_mut(),
            )
        })?;
        Ok(n_out.iter().enumerate().map(|(j, &n)| toks[j * max_new..j * max_new + n].to_vec()).collect())
    }

    /// `generate_batch_mm` for text requests plus per-token log-probabilities (aha_hip_generate_batch_logprobs): `top_logprobs[j]` is
    /// `None` (no logprobs for request j) or `Some(0..=20)` alternatives per token.  The tokens are exactly `generate_batch_mm`'s;
    /// entry `[j][t]` of the second result belongs to token `t` of request j (empty for a request that asked for none).  The
    /// log-probabilities are the model's own (temperature 1, before the repeat penalty), whatever the sampler.
    pub fn generate_batch_logprobs(
        &mut self,
        prompts: &[&[u32]],
        params: Option<&[sys::AhaSamplingParams]>,
        top_logprobs: &[Option<u32>],
        max_new: usize,
        max_tokens_per_pass: usize,
    ) -> Result<(Vec<Vec<u32>>, Vec<Vec<sys::AhaTokenLogprobs>>), Error> {
        if top_logprobs.len() != prompts.len() {
            return Err(Error { code: -1, message: format!("{} top_logprobs for {} prompts", top_logprobs.len(), prompts.len()) });
        }
        if let Some(p) = params {
            if p.len() != prompts.len() {
                return Err(Error { code: -1, message: format!("{} sampling params for {} prompts", p.len(), prompts.len()) });
            }
        }
        let top: Vec<i32> = top_logprobs.iter().map(|t| t.map_or(-1, |n| n as i32)).collect();
        let ids: Vec<u32> = prompts.iter().flat_map(|s| s.iter().copied()).collect();
        let lens: Vec<usize> = prompts.iter().map(|s| s.len()).collect();
        let width = max_new.max(1);
        let mut toks = vec![0u32; prompts.len() * width];
        let mut n_out = vec![0usize; prompts.len()];
        let mut lps = vec![sys::AhaTokenLogprobs::default(); prompts.len() * width];
        check(unsafe {
            sys::aha_hip_generate_batch_logprobs(
                self.model,
                ids.as_ptr(),
                lens.as_ptr(),
                lens.len(),
                std::ptr::null(),
                params.map_or(std::ptr::null(), |p| p.as_ptr()),
                top.as_ptr(),
                max_new,
                max_tokens_per_pass,
                toks.as_mut_ptr(),
                n_out.as_mut_ptr(),
                std::ptr::null_mut(),
                lps.as_mut_ptr(),
            )
        })?;
        let tokens = n_out.iter().enumerate().map(|(j, &n)| toks[j * max_new..j * max_new + n].to_vec()).collect();
        let logprobs =
            n_out.iter().enumerate().map(|(j, &n)| if top[j] < 0 { Vec::new() } else { lps[j * max_new..j * max_new + n].to_vec() }).collect();
        Ok((tokens, logprobs))
    }

    /// `generate_batch_logprobs` plus one `LogitAdjust` per request (aha_hip_generate_batch_adjusted): `logit_bias`, `presence_penalty`
    /// and `frequency_penalty` as include/aha_hip.h defines them.  `top_logprobs` None: no logprobs at all (the second result is empty).
    pub fn generate_batch_adjusted(
        &mut self,
        prompts: &[&[u32]],
        params: Option<&[sys::AhaSamplingParams]>,
        adjust: &[LogitAdjust],
        top_logprobs: Option<&[Option<u32>]>,
        max_new: usize,
        max_tokens_per_pass: usize,
    ) -> Result<(Vec<Vec<u32>>, Vec<Vec<sys::AhaTokenLogprobs>>), Error> {
        if adjust.len() != prompts.len() || top_logprobs.map_or(false, |t| t.len() != prompts.len()) {
            return Err(Error { code: -1, message: format!("adjust / top_logprobs entries do not match {} prompts", prompts.len()) });
        }
        if let Some(p) = params {
            if p.len() != prompts.len() {
                return Err(Error { code: -1, message: format!("{} sampling params for {} prompts", p.len(), prompts.len()) });
            }
        }
        let adj: Vec<sys::AhaLogitAdjust> = adjust.iter().map(|a| a.as_c()).collect();
        let top: Option<Vec<i32>> = top_logprobs.map(|t| t.iter().map(|t| t.map_or(-1, |n| n as i32)).collect());
        let ids: Vec<u32> = prompts.iter().flat_map(|s| s.iter().copied()).collect();
        let lens: Vec<usize> = prompts.iter().map(|s| s.len()).collect();
        let width = max_new.max(1);
        let mut toks = vec![0u32; prompts.len() * width];
        let mut n_out = vec![0usize; prompts.len()];
        let mut lps = vec![sys::AhaTokenLogprobs::default(); if top.is_some() { prompts.len() * width } else { 0 }];
        check(unsafe {
            sys::aha_hip_generate_batch_adjusted(
                self.model,
                ids.as_ptr(),
                lens.as_ptr(),
                lens.len(),
                std::ptr::null(),
                params.map_or(std::ptr::null(), |p| p.as_ptr()),
                adj.as_ptr(),
                top.as_ref().map_or(std::ptr::null(), |t| t.as_ptr()),
                max_new,
                max_tokens_per_pass,
                toks.as_mut_ptr(),
                n_out.as_mut_ptr(),
                std::ptr::null_mut(),
                if top.is_some() { lps.as_mut_ptr() } else { std::ptr::null_mut() },
            )
        })?;
        let tokens = n_out.iter().enumerate().map(|(j, &n)| toks[j * max_new..j * max_new + n].to_vec()).collect();
        let logprobs = n_out
            .iter()
            .enumerate()
            .map(|(j, &n)| match &top {
                Some(t) if t[j] >= 0 => lps[j * max_new..j * max_new + n].to_vec(),
                _ => Vec::new(),
            })
            .collect();
        Ok((tokens, logprobs))
    }

    /// `generate_batch_adjusted` under a per-step allowed-token mask (aha_hip_generate_batch_masked; include/aha_hip.h states the
    /// definition).  `constraint(seq, generated, words)` is called once per live prompt per step, the first token included, while the
    /// step's device work runs: `words` (ceil(V / 32) of them; id i is bit `i & 31` of word `i >> 5`) holds that prompt's previous mask,
    /// all ones the first time.  It returns `Ok(true)` to use `words`, `Ok(false)` for an unmasked step, `Err(())` to fail the call.
    /// A grammar / JSON-schema / regex automaton lives in the closure; this crate compiles none.
    pub fn generate_batch_masked<F: FnMut(usize, &[u32], &mut [u32]) -> Result<bool, ()>>(
        &mut self,
        prompts: &[&[u32]],
        params: Option<&[sys::AhaSamplingParams]>,
        adjust: Option<&[LogitAdjust]>,
        max_new: usize,
        max_tokens_per_pass: usize,
        mut constraint: F,
    ) -> Result<Vec<Vec<u32>>, Error> {
        if adjust.map_or(false, |a| a.len() != prompts.len()) || params.map_or(false, |p| p.len() != prompts.len()) {
            return Err(Error { code: -1, message: format!("adjust / params entries do not match {} prompts", prompts.len()) });
        }
        unsafe extern "C" fn trampoline<F: FnMut(usize, &[u32], &mut [u32]) -> Result<bool, ()>>(
            user: *mut c_void,
            seq: usize,
            generated: *const u32,
            n_generated: usize,
            mask_words: *mut u32,
            n_words: usize,
        ) -> i32 {
            let f = &mut *(user as *mut F);
            let gen: &[u32] = if n_generated == 0 { &[] } else { std::slice::from_raw_parts(generated, n_generated) };
            let words = std::slice::from_raw_parts_mut(mask_words, n_words);
            // a panic must not unwind through the C frames
            match std::panic::catch_unwind(std::panic::AssertUnwindSafe(|| f(seq, gen, words))) {
                Ok(Ok(true)) => 1,
                Ok(Ok(false)) => 0,
                _ => -1,
            }
        }
        let adj: Option<Vec<sys::AhaLogitAdjust>> = adjust.map(|a| a.iter().map(|a| a.as_c()).collect());
        let ids: Vec<u32> = prompts.iter().flat_map(|s| s.iter().copied()).collect();
        let lens: Vec<usize> = prompts.iter().map(|s| s.len()).collect();
        let width = max_new.max(1);
        let mut toks = vec![0u32; prompts.len() * width];
        let mut n_out = vec![0usize; prompts.len()];
        check(unsafe {
            sys::aha_hip_generate_batch_masked(
                self.model,
                ids.as_ptr(),
                lens.as_ptr(),
                lens.len(),
                std::ptr::null(),
                params.map_or(std::ptr::null(), |p| p.as_ptr()),
                adj.as_ref().map_or(std::ptr::null(), |a| a.as_ptr()),
                std::ptr::null(),
                max_new,
                max_tokens_per_pass,
                Some(trampoline::<F>),
                &mut constraint as *mut F as *mut c_void,
                toks.as_mut_ptr(),
                n_out.as_mut_ptr(),
                std::ptr::null_mut(),
                std::ptr::null_mut(),
            )
        })?;
        Ok(n_out.iter().enumerate().map(|(j, &n)| toks[j * max_new..j * max_new + n].to_vec()).collect())
    }

    /// The greedy loop of `generate_generic` / `generate_stream_generic` (common/generate.rs:115-159, 161-368) kept on the
    /// device in chunks of `chunk` tokens: `on_token` sees every token in order (what a streaming response forwards) and
    /// returns `false` to stop; an eos id stops after it has been delivered, as in the reference.
    pub fn decode_greedy_stream<F: FnMut(u32) -> bool>(
        &mut self,
        first_token: u32,
        mut seqlen_offset: usize,
        max_new: usize,
        chunk: usize,
        mut on_token: F,
    ) -> Result<usize, Error> {
        let mut buf = vec![0u32; chunk.max(1)];
        let (mut tok, mut produced) = (first_token, 0usize);
        while produced < max_new {
            let n = buf.len().min(max_new - produced);
            let got = unsafe { sys::aha_hip_decode_greedy(self.model, tok, seqlen_offset, n, buf.as_mut_ptr()) };
            check(got)?;
            let got = got as usize;
            for &t in &buf[..got] {
                produced += 1;
                if !on_token(t) || self.stop.contains(&t) {
                    return Ok(produced);
                }
            }
            if got < n || got == 0 {
                break; // the library saw an eos id inside the chunk
            }
            tok = buf[got - 1];
            seqlen_offset += got;
        }
        Ok(produced)
    }

    /// `sample_and_push` without the logits copy (common/generate.rs:70-86): repeat penalty over `context`, the `k` largest
    /// penalised logits (value descending, index ascending), the full-vocabulary max and sum exp((x - max) / T).
    pub fn sample_candidates(&mut self, context: &[u32], repeat_penalty: f32, temperature: f32, k: usize) -> Result<(Vec<f32>, Vec<u32>, f32, f32), Error> {
        let (mut vals, mut idx) = (vec![0f32; k], vec![0u32; k]);
        let (mut mx, mut se) = (0f32, 0f32);
        check(unsafe {
            sys::aha_hip_sample_candidates(self.model, context.as_ptr(), context.len(), repeat_penalty, temperature, k as i32, vals.as_mut_ptr(), idx.as_mut_ptr(), &mut mx, &mut se)
        })?;
        Ok((vals, idx, mx, se))
    }

    pub fn last_logits(&mut self, out: &mut [f32]) -> Result<(), Error> {
        assert!(out.len() >= self.vocab);
        check(unsafe { sys::aha_hip_last_logits(self.model, out.as_mut_ptr()) })
    }

    /// 128 bytes that identify an RCCL communicator: rank 0 makes them, the host sends them to every rank
    pub fn rccl_unique_id() -> Result<[u8; 128], Error> {
        let mut id = [0u8; 128];
        check(unsafe { sys::aha_hip_tp_unique_id(id.as_mut_ptr() as *mut std::ffi::c_void) })?;
        Ok(id)
    }

    /// Context-parallel prefill over `world` GPUs of one node (one process / one `Model` with the FULL weights per GPU): after this,
    /// every rank calls `forward_initial` with the same prompt at offset 0; each ends with the whole KV cache and the same logits, and
    /// decode continues on rank 0 exactly as after a single-GPU prefill (no hand-back).  `unique_id`: `rccl_unique_id()` of rank 0.
    pub fn set_context_parallel(&mut self, rank: usize, world: usize, unique_id: &[u8; 128]) -> Result<(), Error> {
        check(unsafe { sys::aha_hip_set_context_parallel(self.model, rank as i32, world as i32, None, std::ptr::null_mut()) })?;
        if world > 1 {
            check(unsafe { sys::aha_hip_cp_init_rccl(self.model, unique_id.as_ptr() as *const std::ffi::c_void) })?;
        }
        Ok(())
    }
}

impl Drop for Model {
    fn drop(&mut self) {
        unsafe {
            sys::aha_hip_model_destroy(self.model);
            sys::aha_hip_shutdown(self.ctx);
        }
    }
}

/// Continuous batching over one model (`aha_hip_engine_*`): what `generate_stream` drives for `stream: true`
/// (`generate_stream_generic`, reference `src/models/common/generate.rs:231-368`).  `submit` queues a request, every `step` returns
/// the tokens emitted in it (one per running request), `cancel` ends one at the next step.  While it lives the engine owns the model's
/// cache: borrow the model mutably for its lifetime.
pub struct Engine<'a> {
    e: *mut sys::AhaEngine,
    _m: std::marker::PhantomData<&'a mut Model>,
}
impl<'a> Engine<'a> {
    pub fn new(model: &'a mut Model, cfg: sys::AhaEngineConfig) -> Result<Self, Error> {
        let mut e = std::ptr::null_mut();
        check(unsafe { sys::aha_hip_engine_create(model.model, &cfg, &mut e) })?;
        Ok(Self { e, _m: std::marker::PhantomData })
    }
    /// One request: `params` None = greedy.  Text only here (`mm` must outlive the request's first token in the C ABI).
    pub fn submit(&mut self, ids: &[u32], params: Option<&sys::AhaSamplingParams>, max_new: usize) -> Result<u64, Error> {
        let mut id = 0u64;
        let p = params.map_or(std::ptr::null(), |p| p as *const _);
        check(unsafe { sys::aha_hip_engine_submit(self.e, ids.as_ptr(), ids.len(), std::ptr::null(), p, max_new, &mut id) })?;
        Ok(id)
    }
    /// `submit` plus the request's `top_logprobs` (0..=20): `step_logprobs` then reports every token's log-probability.
    pub fn submit_logprobs(&mut self, ids: &[u32], params: Option<&sys::AhaSamplingParams>, max_new: usize, top_logprobs: u32) -> Result<u64, Error> {
        let mut id = 0u64;
        let p = params.map_or(std::ptr::null(), |p| p as *const _);
        check(unsafe {
            sys::aha_hip_engine_submit_logprobs(self.e, ids.as_ptr(), ids.len(), std::ptr::null(), p, max_new, top_logprobs as i32, &mut id)
        })?;
        Ok(id)
    }
    /// `submit_logprobs` plus the request's `LogitAdjust` (copied by the library); `top_logprobs` None: no logprobs.
    pub fn submit_adjusted(
        &mut self,
        ids: &[u32],
        params: Option<&sys::AhaSamplingParams>,
        adjust: &LogitAdjust,
        max_new: usize,
        top_logprobs: Option<u32>,
    ) -> Result<u64, Error> {
        let mut id = 0u64;
        let p = params.map_or(std::ptr::null(), |p| p as *const _);
        let a = adjust.as_c();
        check(unsafe {
            sys::aha_hip_engine_submit_adjusted(
                self.e,
                ids.as_ptr(),
                ids.len(),
                std::ptr::null(),
                p,
                &a,
                max_new,
                top_logprobs.map_or(-1, |n| n as i32),
                &mut id,
            )
        })?;
        Ok(id)
    }
    /// `submit_adjusted` plus an initial allowed-token mask (ceil(V / 32) packed words, copied), which governs the request's tokens from
    /// the first one until `set_mask` replaces or clears it.
    pub fn submit_masked(
        &mut self,
        ids: &[u32],
        params: Option<&sys::AhaSamplingParams>,
        adjust: Option<&LogitAdjust>,
        mask: Option<&[u32]>,
        max_new: usize,
        top_logprobs: Option<u32>,
    ) -> Result<u64, Error> {
        let mut id = 0u64;
        let p = params.map_or(std::ptr::null(), |p| p as *const _);
        let a = adjust.map(|a| a.as_c());
        check(unsafe {
            sys::aha_hip_engine_submit_masked(
                self.e,
                ids.as_ptr(),
                ids.len(),
                std::ptr::null(),
                p,
                a.as_ref().map_or(std::ptr::null(), |a| a as *const _),
                mask.map_or(std::ptr::null(), |m| m.as_ptr()),
                mask.map_or(0, |m| m.len()),
                max_new,
                top_logprobs.map_or(-1, |n| n as i32),
                &mut id,
            )
        })?;
        Ok(id)
    }
    /// Replace (`Some(words)`) or clear (`None`) the mask of a waiting or running request, between steps: it acts from the next token the
    /// request samples and stays until it is replaced.  A server drives its grammar from the streamed tokens and calls this each step.
    pub fn set_mask(&mut self, req_id: u64, mask: Option<&[u32]>) -> Result<(), Error> {
        check(unsafe { sys::aha_hip_engine_set_mask(self.e, req_id, mask.map_or(std::ptr::null(), |m| m.as_ptr()), mask.map_or(0, |m| m.len())) })
    }
    /// A greedy draft-and-verify request (`aha_hip_engine_submit_spec`): the chat request's `prediction` (reference
    /// `src/params/chat.rs:105`) for `stream: true`; `None`: prompt lookup only.  Its tokens are those of `submit` with `params` None; a
    /// step may return up to `1 + spec.max_draft` events for it, consecutive and in generation order.
    pub fn submit_spec(&mut self, ids: &[u32], max_new: usize, spec: &sys::AhaSpecConfig, prediction: Option<&[u32]>) -> Result<u64, Error> {
        let mut id = 0u64;
        check(unsafe {
            sys::aha_hip_engine_submit_spec(
                self.e,
                ids.as_ptr(),
                ids.len(),
                std::ptr::null(),
                max_new,
                spec,
                prediction.map_or(std::ptr::null(), |p| p.as_ptr()),
                prediction.map_or(0, |p| p.len()),
                &mut id,
            )
        })?;
        Ok(id)
    }
    /// The event capacity the next `step` needs (`aha_hip_engine_max_events`), pending cancellations included.
    pub fn max_events(&self) -> usize {
        unsafe { sys::aha_hip_engine_max_events(self.e) }
    }
    /// Decode steps, rows, proposed and accepted draft tokens over the engine's life (`aha_hip_engine_spec_stats`).
    pub fn spec_stats(&self) -> Result<sys::AhaSpecStats, Error> {
        let mut s = sys::AhaSpecStats::default();
        check(unsafe { sys::aha_hip_engine_spec_stats(self.e, &mut s) })?;
        Ok(s)
    }
    /// (proposed, accepted) draft tokens of a running request or of one the most recent step ended (`aha_hip_engine_request_spec`): a
    /// response's `accepted_prediction_tokens` / `rejected_prediction_tokens` (reference `src/params/shared.rs:58-63`).
    pub fn request_spec(&self, req_id: u64) -> Result<(usize, usize), Error> {
        let (mut p, mut a) = (0usize, 0usize);
        check(unsafe { sys::aha_hip_engine_request_spec(self.e, req_id, &mut p, &mut a) })?;
        Ok((p, a))
    }
    pub fn cancel(&mut self, req_id: u64) -> Result<(), Error> {
        check(unsafe { sys::aha_hip_engine_cancel(self.e, req_id) })
    }
    /// The step's events: (request, token or None for a cancellation, flags `AHA_ENGINE_EV_*`).
    pub fn step(&mut self) -> Result<Vec<(u64, Option<u32>, u32)>, Error> {
        let cap = self.max_events();
        let mut ev = vec![sys::AhaEngineEvent::default(); cap];
        let mut n = 0usize;
        check(unsafe { sys::aha_hip_engine_step(self.e, ev.as_mut_ptr(), cap, &mut n, std::ptr::null_mut()) })?;
        Ok(ev[..n]
            .iter()
            .map(|x| (x.req_id, if x.flags & sys::AHA_ENGINE_EV_CANCELLED != 0 { None } else { Some(x.token) }, x.flags))
            .collect())
    }
    /// `step` plus each event's log-probabilities: `None` for a cancellation and for a request submitted without `top_logprobs`.
    pub fn step_logprobs(&mut self) -> Result<Vec<(u64, Option<u32>, u32, Option<sys::AhaTokenLogprobs>)>, Error> {
        let cap = self.max_events();
        let mut ev = vec![sys::AhaEngineEvent::default(); cap];
        let mut lp = vec![sys::AhaTokenLogprobs::default(); cap];
        let mut n = 0usize;
        check(unsafe { sys::aha_hip_engine_step_logprobs(self.e, ev.as_mut_ptr(), cap, &mut n, std::ptr::null_mut(), lp.as_mut_ptr()) })?;
        Ok(ev[..n]
            .iter()
            .zip(lp[..n].iter())
            .map(|(x, l)| {
                let tok = if x.flags & sys::AHA_ENGINE_EV_CANCELLED != 0 { None } else { Some(x.token) };
                (x.req_id, tok, x.flags, if l.n_top < 0 { None } else { Some(*l) })
            })
            .collect())
    }
    pub fn stats(&self) -> Result<sys::AhaEngineStats, Error> {
        let mut s = sys::AhaEngineStats::default();
        check(unsafe { sys::aha_hip_engine_stats(self.e, &mut s) })?;
        Ok(s)
    }
}
impl Drop for Engine<'_> {
    fn drop(&mut self) {
        unsafe { sys::aha_hip_engine_destroy(self.e) }
    }
}

/// candle's `LogitsProcessor::rng` + `sample_multinomial` behind the C ABI (`aha_hip_rng_*`): rand 0.9.2 `StdRng::seed_from_u64`
/// (candle-transformers' own rand, Cargo.lock:590-606) and `WeightedIndex::<f32>::new(prs)?.sample(&mut rng)`.  A host that keeps
/// candle's `LogitsProcessor` does not need this; a host that takes `aha_hip_sample_candidates`' candidates instead of the
/// V-float logits draws with it so that a seed still defines the token sequence.
pub struct StdRng(*mut sys::AhaRng);
unsafe impl Send for StdRng {}
impl StdRng {
    pub fn seed_from_u64(seed: u64) -> Result<Self, Error> {
        let mut h = std::ptr::null_mut();
        check(unsafe { sys::aha_hip_rng_create(seed, &mut h) })?;
        Ok(Self(h))
    }
    pub fn next_u32(&mut self) -> u32 {
        unsafe { sys::aha_hip_rng_next_u32(self.0) }
    }
    /// `WeightedIndex::new(weights)?.sample(self)`: Err for a negative / NaN weight or an all-zero vector, the stream untouched.
    pub fn weighted_index(&mut self, weights: &[f32]) -> Result<usize, Error> {
        let mut idx = 0u32;
        check(unsafe { sys::aha_hip_rng_weighted_index(self.0, weights.as_ptr(), weights.len(), &mut idx) })?;
        Ok(idx as usize)
    }
}
impl Drop for StdRng {
    fn drop(&mut self) {
        unsafe { sys::aha_hip_rng_destroy(self.0) }
    }
}

/// The host half of the sampled single-sequence path (`aha_hip_sampler_*`): `LogitsProcessor` as `get_logit_processor` builds it,
/// `use_repeat_penalty`'s slicing and the RNG stream.  Per token: `plan` says how many candidates to ask `aha_hip_sample_candidates`
/// for, `pick` turns them (or, on `Ok(None)`, the full logits of `aha_hip_last_logits`) into the token.
pub struct Sampler(*mut sys::AhaSampler);
unsafe impl Send for Sampler {}
impl Sampler {
    pub fn new(params: &sys::AhaSamplingParams) -> Result<Self, Error> {
        let mut h = std::ptr::null_mut();
        check(unsafe { sys::aha_hip_sampler_create(params, &mut h) })?;
        Ok(Self(h))
    }
    /// (k, temperature, effective repeat penalty, context length) after `n_generated` tokens; k == 0: no candidate step.
    pub fn plan(&self, vocab_size: usize, n_generated: usize) -> Result<(i32, f32, f32, usize), Error> {
        let (mut k, mut t, mut p, mut n) = (0i32, 0f32, 1f32, 0usize);
        check(unsafe { sys::aha_hip_sampler_plan(self.0, vocab_size, n_generated, &mut k, &mut t, &mut p, &mut n) })?;
        Ok((k, t, p, n))
    }
    /// The token, or `None` when the candidates cannot decide and `logits` was not given.
    pub fn pick(
        &mut self,
        cands: Option<(&[f32], &[u32], f32, f32)>,
        logits: Option<&[f32]>,
        vocab_size: usize,
        generated: &[u32],
    ) -> Result<Option<u32>, Error> {
        let (vals, idx, k, mx, se) = match cands {
            Some((v, i, mx, se)) => (v.as_ptr(), i.as_ptr(), v.len().min(i.len()) as i32, mx, se),
            None => (std::ptr::null(), std::ptr::null(), 0, 0.0, 0.0),
        };
        let lg = logits.map_or(std::ptr::null(), |l| l.as_ptr());
        let mut tok = 0u32;
        let rc = unsafe {
            sys::aha_hip_sampler_pick(self.0, vals, idx, k, mx, se, lg, vocab_size, generated.as_ptr(), generated.len(), &mut tok)
        };
        check(rc)?;
        Ok(if rc == sys::AHA_SAMPLE_NEED_LOGITS { None } else { Some(tok) })
    }
}
impl Drop for Sampler {
    fn drop(&mut self) {
        unsafe { sys::aha_hip_sampler_destroy(self.0) }
    }
}

/// The reference's seam: `trait InferenceModel` (src/models/common/mod.rs:25-45).
#[cfg(feature = "aha")]
pub mod inference_model {
    use super::{MmInput, Model};
    use aha::models::common::{InferenceModel, MultiModalData};
    use anyhow::{anyhow, Result};
    use candle_core::{DType, Device, Tensor};

    pub struct HipQwen3 {
        pub model: Model,
    }

    impl HipQwen3 {
        fn logits_tensor(&self, v: Vec<f32>) -> Result<Tensor> {
            // generate.rs:75 squeezes the (1, 1, V) tensor and casts it to f32 on the host: hand it over that way
            Ok(Tensor::from_vec(v, (1, 1, self.model.vocab_size()), &Device::Cpu)?)
        }
    }

    impl InferenceModel for HipQwen3 {
        fn forward_initial(&mut self, input_ids: &Tensor, seqlen_offset: usize, data: MultiModalData) -> Result<Tensor> {
            let ids = input_ids.flatten_all()?.to_vec1::<u32>()?;
            let mut logits = vec![0f32; self.model.vocab_size()];
            let first = data.data_vec.first().cloned().flatten();
            let second = data.data_vec.get(1).cloned().flatten();
            let third = data.data_vec.get(2).cloned().flatten();
            let fourth = data.data_vec.get(3).cloned().flatten();
            let (host_a, host_b, host_c, host_d);
            let mm = match (first, second) {
                // Qwen3-VL with a video: data_vec = [pixel_values?, image_grid_thw?, pixel_values_video, video_grid_thw,
                // cache_position] (qwen3vl/model.rs:1292-1308)
                (img, igrid) if third.is_some() && fourth.is_some() => {
                    let (pvv, vgrid) = (third.unwrap(), fourth.unwrap());
                    host_c = pvv.to_dtype(DType::F32)?.flatten_all()?.to_vec1::<f32>()?;
                    host_d = vgrid.flatten_all()?.to_vec1::<u32>()?;
                    let image = match (img, igrid) {
                        (Some(pv), Some(grid)) => {
                            host_a = pv.to_dtype(DType::F32)?.flatten_all()?.to_vec1::<f32>()?;
                            host_b = grid.flatten_all()?.to_vec1::<u32>()?;
                            Some((&host_a[..], pv.dim(0)?, &host_b[..]))
                        }
                        _ => None,
                    };
                    MmInput::Vision { image, video: Some((&host_c[..], pvv.dim(0)?, &host_d[..])) }
                }
                // Qwen3-VL: data_vec = [pixel_values, image_grid_thw, None, None, cache_position] (qwen3vl/generate.rs:79-101)
                (Some(pv), Some(grid)) => {
                    host_a = pv.to_dtype(DType::F32)?.flatten_all()?.to_vec1::<f32>()?;
                    host_b = grid.flatten_all()?.to_vec1::<u32>()?;
                    MmInput::Image { pixel_values: &host_a, n_patches: pv.dim(0)?, grid_thw: &host_b }
                }
                // Qwen3-ASR: data_vec = [input_features] (num_mel_bins, n_frames) (qwen3_asr/generate.rs:100-125)
                (Some(feat), None) => {
                    let n_frames = feat.dim(feat.rank() - 1)?;
                    host_a = feat.to_dtype(DType::F32)?.flatten_all()?.to_vec1::<f32>()?;
                    MmInput::AudioFeatures { features: &host_a, n_frames }
                }
                _ => MmInput::None,
            };
            self.model.forward_initial(&ids, seqlen_offset, mm, Some(&mut logits)).map_err(|e| anyhow!(e.to_string()))?;
            self.logits_tensor(logits)
        }

        fn forward_step(&mut self, input_ids: &Tensor, seqlen_offset: usize) -> Result<Tensor> {
            let tok = input_ids.flatten_all()?.to_vec1::<u32>()?[0];
            let mut logits = vec![0f32; self.model.vocab_size()];
            self.model.forward_step(tok, seqlen_offset, Some(&mut logits)).map_err(|e| anyhow!(e.to_string()))?;
            self.logits_tensor(logits)
        }

        fn clear_cache(&mut self) {
            self.model.clear_cache();
        }

        fn stop_token_ids(&self) -> Vec<u32> {
            self.model.stop_token_ids()
        }
    }
}
