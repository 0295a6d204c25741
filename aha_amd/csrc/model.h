// Host-side model object behind the C ABI (include/aha_hip.h).  Mirrors the reference's Qwen3Model
// (/root/reference/src/models/qwen3/model.rs:94-214) and its InferenceModel impl, re-designed for one MI355X:
// fused weight layouts, a paged KV cache that grows without reallocating, device-resident step state.
#pragma once
#include <hip/hip_runtime.h>

#include <map>
#include <string>
#include <vector>

#include "../../include/aha_hip.h"
#include "kernels.h"

struct aha_ctx {
  int device = 0;
  hipStream_t stream = nullptr;
};

namespace aha {

void set_error(const std::string& msg);
#define AHA_HIP_CHECK(expr)                                                                          \
  do {                                                                                               \
    hipError_t _e = (expr);                                                                          \
    if (_e != hipSuccess) {                                                                          \
      ::aha::set_error(std::string(#expr) + " failed: " + hipGetErrorString(_e));                    \
      return AHA_ERR_HIP;                                                                            \
    }                                                                                                \
  } while (0)

struct Pk13Copy {
  void* p = nullptr;   // pk13_bytes(N, K), a hipMalloc of its own (freed by model_free_packed)
  int bh = 0;          // the matrix's exponent base
  // exception rows: rows of w (ascending, in its own order) with a finite weight below the window, which the kernel computes from w itself
  const void* w = nullptr;   // the bf16 matrix the copy was made of (the model keeps it)
  int nrows = 0;
  int rows[PK13_MAX_EXC] = {};
};
// aha_hip_pk13_status: "packed", "<n> weights outside the window: packed, rows ... read from bf16", or the reason there is no copy
struct Pk13Entry { std::string name; Pk13Copy* slot; std::string status; };

struct LayerWeights {
  void* wqkv = nullptr;     // ((nh+2kvh)*d, H): q rows, then k rows, then v rows
  void* wo = nullptr;       // (H, nh*d)
  void* wgu = nullptr;      // (2I, H): 16-row blocks alternating gate / up (see kernels_gemm.hip ACT_SILU_MUL_PAIRS)
  void* wdown = nullptr;    // (H, I)
  void* in_norm = nullptr;  // (H)
  void* post_norm = nullptr;
  void* q_norm = nullptr;   // (d)
  void* k_norm = nullptr;
  // MXFP8 or MXFP4 copies of the four matrices (aha_hip_model_quantize_weights; null: none; the format is aha_model::wq_format): the batched
  // decode matvec streams these
  WQuant q_wqkv, q_wo, q_wgu, q_wdown;
  // exact 13-bit copies (kernels_gemv_pk13.hip; model_pack_weights; null: none): the single-sequence matvec streams these
  Pk13Copy p_wqkv, p_wo, p_wgu, p_wdown;
};

// device-resident scalars every decode kernel reads (so a step can be enqueued / replayed without host values)
constexpr uint32_t RING_CAP = 256;   // token ring of the device-resident greedy loop (>> its run-ahead)

struct StepState {
  uint32_t token;
  int32_t pos[3];     // rope position rows T,H,W of the current token
  int32_t kv_start;   // cache slot the current token is written to
  int32_t kv_len;     // valid cache tokens after the append
  uint32_t next_token;  // argmax of the last logits
  int32_t step;       // index into the device token log
};

struct ProfRec { int cls; hipEvent_t e0, e1; double bytes, flops; };

struct VisionModel;  // vision.h
struct AudioModel;   // audio.h

}  // namespace aha

// mmapped checkpoint directory (loader.hip)
struct aha_weights {
  struct Mapping { void* base; size_t len; };
  std::vector<Mapping> maps;
  std::vector<std::string> names;       // stable storage for aha_tensor_view::name
  std::vector<aha_tensor_view> views;
  ~aha_weights();
};

struct aha_model {
  aha_ctx* ctx = nullptr;
  aha_model_desc desc{};
  hipStream_t stream = nullptr;
  // weights
  void* embed = nullptr;
  void* lm_head = nullptr;  // == embed when tied
  void* final_norm = nullptr;
  std::vector<aha::LayerWeights> layers;
  std::vector<void*> owned;  // every hipMalloc'd block (weights, scratch), freed on destroy
  // aha_hip_model_quantize_weights: AHA_WQ_NONE or the format the matrices were quantised with, its flags, lm_head's copy (AHA_WQ_LM_HEAD)
  int32_t wq_format = 0;
  uint32_t wq_flags = 0;
  aha::WQuant q_lm_head;
  bool fp8_rows = true;      // aha_hip_debug_fp8_rows: false = the bf16 matvec on W' although a copy (of either format) exists
  int fp8_single = 1;        // aha_hip_debug_fp8_single, the single-sequence matvec (enqueue_decode_step, enqueue_lm_head): 0 = bf16 on W',
                             // 1 = the FP8 kernel where the plan takes the shape (gemv_mxfp8_by_plan), 2 = wherever a copy exists; MXFP8 models only
  // Exact 13-bit copies of the four layer matrices and lm_head, made when the model is created (model_pack_weights; a bf16 model only:
  // aha_hip_model_quantize_weights frees them).  pk13_single (aha_hip_debug_pk13_single): 0 = the bf16 kernel, 1 = the packed kernel where
  // the plan takes the shape (gemv_pk13_by_plan), 2 = wherever a copy exists
  aha::Pk13Copy p_lm_head;
  std::vector<aha::Pk13Entry> pk13;
  int pk13_single = 1;
  int fp4_single = 1;        // aha_hip_debug_fp4_single: the same three values for an MXFP4 model and gemv_mxfp4_kernel (gemv_mxfp4_by_plan)
  // rope constants
  float* d_inv_freq = nullptr;
  int32_t* d_axis_map = nullptr;
  float* d_rope = nullptr;       // (128) f32: the current decode step's rope cos/sin table (embed_state_kernel)
  float attn_scale = 0.f;
  // paged KV cache
  std::vector<void*> slabs;
  std::vector<uint64_t> h_page_ptrs;  // logical page -> byte address of its layer-0 storage
  uint64_t* d_page_ptrs = nullptr;
  size_t page_table_cap = 0;
  size_t pages_per_slab = 0;
  uint64_t page_bytes = 0;      // bytes of one page of one layer (K block + V block)
  uint64_t layer_stride = 0;    // bytes between layers inside a slab
  size_t n_pages = 0;           // pages currently mapped
  // Pages [0, lin_pages) are the arithmetic progression lin_p0 + i * lin_step (model_ensure_pages keeps this up to date, O(1) per page):
  // one slab handed out in order, which is every cache up to a slab's tokens.  The decode step's attention then takes (lin_p0 + layer
  // offset, lin_step) as kernel arguments and never reads the page table (kernels.h AttnDecodeFusedArgs::lin_step).
  size_t lin_pages = 0;
  uint64_t lin_p0 = 0;
  int64_t lin_step = 0;
  int last_attn_form = -1;      // the last decode step's attention launches: 1 linear form, 0 table form, -1 none yet (debug getter)
  size_t cache_len = 0;         // tokens in the cache (== reference kv_cache.dim(2))
  bool scramble_pages = false;
  std::vector<uint64_t> free_pages;
  // step state
  aha::StepState* d_state = nullptr;
  aha::StepState* h_state = nullptr;  // pinned
  uint32_t* d_token_log = nullptr;
  size_t token_log_cap = 0;
  // device-resident greedy loop (model_decode_greedy): the generated tokens and the count of finished steps, written by the last
  // kernel of every step into PINNED host memory (system-scope stores) so the host can watch for a stop token while later steps
  // are still queued, without a stream synchronisation
  uint32_t* h_ring = nullptr;        // [RING_CAP] tokens, slot = step % RING_CAP   (host pointer)
  uint32_t* h_ring_dev = nullptr;    // the same buffer as the device sees it
  uint32_t* h_done = nullptr;        // steps finished since the loop started (host pointer; h_ring + RING_CAP)
  uint32_t* h_done_dev = nullptr;
  int64_t steps_executed = 0;        // decode steps that ran on the device in the last model_decode_greedy call (tests)
  bool rope_delta_valid = false;  // Qwen3VLModel::rope_deltas.is_some() (qwen3vl/model.rs:1229-1236)
  int64_t rope_delta = 0;  // Qwen3-VL: decode position = seqlen_offset + rope_delta (qwen3vl/model.rs:1235-1264)
  // decode scratch
  void *d_x = nullptr, *d_qkv = nullptr, *d_q = nullptr, *d_attn = nullptr, *d_act = nullptr, *d_hlast = nullptr;
  float* d_logits = nullptr;
  float* d_blk_max = nullptr;
  uint32_t* d_blk_idx = nullptr;
  float* d_part_o = nullptr;
  float* d_part_ml = nullptr;
  int max_nsplit = 64;
  // tensor parallelism (desc.tp_rank / tp_size); desc.num_attention_heads etc. hold the LOCAL (per-rank) sizes
  int tp_rank = 0, tp_size = 1;
  aha_allreduce_fn allreduce_cb = nullptr;
  void* allreduce_user = nullptr;
  aha_reduce_scatter_fn reduce_scatter_cb = nullptr;   // sequence-parallel prefill (aha_hip_set_seq_parallel)
  aha_all_gather_fn all_gather_cb = nullptr;
  void* sp_user = nullptr;
  void* rccl_comm = nullptr;
  void* rccl_comm_side = nullptr;   // a second communicator of the same ranks (ncclCommSplit) for the collectives enqueued on comm_stream
  // sequence-parallel prefill with the collectives of a row-parallel projection overlapped with its GEMM (model.hip
  // gemm_row_parallel): RCCL runs on its own high-priority stream, ordered against the compute stream by events
  hipStream_t comm_stream = nullptr;
  bool reserved_cus_set = false;   // this model holds a share of the reference-counted CU reservation (released with the communicator)
  hipEvent_t ev_gemm[8] = {};
  hipEvent_t ev_ag[8] = {};   // chunk i of a chunked all-gather has landed (norm_gather_gemm)
  hipEvent_t ev_comm = nullptr;
  int async_rc = 0;             // first error of an all-reduce issued from inside an enqueue helper
  int lm_rows = 0, lm_row0 = 0; // lm_head rows this rank streams (vocab-parallel under TP) and the first of them
  float* d_partial = nullptr;   // decode: (hidden) f32 partial projection; also the 2T-float argmax pair exchange
  float* p_partial = nullptr;   // prefill: (S, hidden) f32
  // Context-parallel prefill (aha_hip_set_context_parallel; model.hip cp_make_plan): every rank holds the FULL weights (tp_size 1) and
  // owns two page-aligned row chunks of the prompt; the only exchange is one all-gather of the layer's K / V pages per layer
  int cp_rank = 0, cp_size = 1;
  int comm_rank = 0;              // this rank's index in rccl_comm (tp_rank or cp_rank)
  aha_all_gather_fn cp_all_gather_cb = nullptr;   // host-callback seam (tests); RCCL otherwise
  void* cp_user = nullptr;
  void* p_cp_stage = nullptr;     // [rank][page slot][kv heads][K | V] of ONE layer, bf16
  // context-parallel prefill in flight: prompt row -> row of this rank's (compacted) activation buffers, or the scratch row behind them
  // for rows another rank owns; empty otherwise.  The vision tower's scatter / DeepStack adds go through it (vision_tower.hip).
  std::vector<int32_t> cp_row_map;
  size_t cp_stage_bytes = 0;
  void* p_hstage = nullptr;     // tensor-parallel prefill: staging of the chunked all-gather, [chunk][rank][rows] bf16 (norm_gather_gemm)
  unsigned head_ctr_base = 0;       // value every kv head's split-arrival counter has reached after all launches so far
  unsigned* d_bar = nullptr;        // split-arrival counters of the fused decode attention (kernels.h DECODE_SYNC_BYTES)
  unsigned long long* d_gemv_trace = nullptr;  // AHA_GEMV_TRACE timeline
  unsigned long long* d_attn_trace = nullptr;  // AHA_ATTN_TRACE timeline
  bool decode_fused = true;  // attention block of a decode step in one launch (kernels_attn.hip attn_decode_fused_kernel)
  float* h_logits = nullptr;  // pinned
  bool have_logits = false;   // d_logits holds the logits of a completed forward call
  bool logits_assembled = false;  // vocab-parallel TP: d_logits already all-reduced into the full vector
  // D11 candidate extraction (kernels_sample.hip), allocated on first use
  float* d_samp_work = nullptr;   // (V) penalised copy of the logits
  float* d_samp_f = nullptr;      // cand_val | part_m | part_s | out block {vals[64], max, sumexp, idx[64]}
  unsigned* d_samp_u = nullptr;   // cand_idx
  uint32_t* d_samp_ctx = nullptr;
  uint32_t* h_samp = nullptr;     // pinned: context ids (samp_ctx_cap) followed by the 130-word out block
  size_t samp_ctx_cap = 0;
  // prefill scratch (grown on demand)
  size_t pf_cap = 0;
  uint32_t* p_ids = nullptr;
  int32_t* p_pos = nullptr;
  void *p_x = nullptr, *p_h = nullptr, *p_qkv = nullptr, *p_q = nullptr, *p_attn = nullptr, *p_act = nullptr;
  void* p_rope = nullptr;       // (S, 128) bf16 cos | sin table of the prefill's positions (kernels.h launch_rope_table)
  void* p_gemm_ws = nullptr;    // f32 split-K slabs (kernels_gemm.hip)
  size_t gemm_ws_bytes = 0;
  void* d_sk_ctrs = nullptr;    // SK_MAX_COUNTERS zeroed u32: per-tile arrival counters of the persistent GEMM kernel (kernels_gemm_sk.hip)
  std::vector<void*> pf_owned;
  // packed prefill passes (model_embed_batch, the generate_batch entries; model.hip PackedPass), grown on demand: the pass's int32 table
  // (segments | items | row slots | page rows | last rows), and the pinned staging buffer its ids | positions | table go up through
  int32_t* p_pass_tab = nullptr;
  size_t p_pass_tab_cap = 0;
  int32_t* h_pass_stage = nullptr;
  size_t h_pass_stage_cap = 0;
  float* p_pool = nullptr;   // model_embed_batch: a pass's (sequences, hidden) f32 embeddings
  size_t p_pool_cap = 0;
  // the continuous batching engine that owns the cache while it exists (model.hip engine_*): every other entry that touches the cache
  // returns AHA_ERR_STATE meanwhile (capi.hip)
  aha_engine* engine = nullptr;
  // vision tower (Qwen3-VL)
  aha::VisionModel* vision = nullptr;
  // audio tower (Qwen3-ASR)
  aha::AudioModel* audio = nullptr;
  // profiling
  bool profiling = false;
  std::vector<aha::ProfRec> prof;
  std::map<std::string, int> prof_cls;
  std::vector<std::string> prof_names;
  struct ProfAcc { double ms = 0, bytes = 0, flops = 0; int64_t n = 0; };
  std::vector<ProfAcc> prof_acc;
};

namespace aha {

// model.hip
int model_create(aha_ctx* ctx, const aha_model_desc* desc, const aha_tensor_view* w, size_t nw, aha_model** out);
void model_destroy(aha_model* m);
int model_embed(aha_model* m, const uint32_t* ids, size_t n, float* out);
int model_embed_batch(aha_model* m, const uint32_t* ids, const size_t* seq_lens, size_t n_seqs, size_t max_tokens_per_pass, float* out);
// What a batch generation call may carry beyond ids, lens, max_new, the pass budget, tokens_out and n_out: every field absent by default.
// A new per-request option is a field here, a check in capi.hip's gen_options_check and its use in model_generate_batch.
struct GenOptions {
  const aha_mm_input* const* mm = nullptr;         // per sequence null or its images / videos / audio
  const aha_sampling_params* params = nullptr;     // per sequence; null: every sequence greedy
  const aha_logit_adjust* adjust = nullptr;        // per sequence
  const int32_t* top_logprobs = nullptr;           // per sequence (-1: none), with logprobs_out
  aha_token_logprobs* logprobs_out = nullptr;
  aha_token_mask_fn mask_fn = nullptr;
  void* mask_user = nullptr;
  float* logits_out = nullptr;                     // (n_seqs, vocab): the logits that chose each sequence's last token
  float* step_logits_out = nullptr;                // (n_seqs, max_new, vocab): every step's logits
  // aha_hip_generate_batch_spec (spec set: a draft-and-verify run, checked by spec_config_check)
  const aha_spec_config* spec = nullptr;
  const uint32_t* predictions = nullptr;           // packed like input_ids, or null
  const size_t* prediction_lens = nullptr;
  size_t *n_proposed = nullptr, *n_accepted = nullptr;   // per sequence, may be null
  aha_spec_stats* stats = nullptr;                 // may be null
};
int model_generate_batch(aha_model* m, const uint32_t* ids, const size_t* seq_lens, size_t n_seqs, size_t max_new, size_t max_tokens_per_pass,
                         const GenOptions& o, uint32_t* tokens_out, size_t* n_out);
// spec_host.hip: the draft proposer (host only).  spec_config_check: AHA_OK or AHA_ERR_INVALID with the message set (who: the entry's name)
int spec_config_check(const aha_spec_config* spec, const char* who);
void spec_propose(const aha_spec_config& spec, const uint32_t* ctx, size_t n_ctx, size_t n_prompt, const uint32_t* pred, size_t n_pred,
                  uint32_t* draft_out, size_t* n_draft);
int engine_config_check(const aha_engine_config* cfg, size_t* budget_out, size_t* chunk_out);
int engine_create(aha_model* m, const aha_engine_config* cfg, aha_engine** out);
void engine_destroy(aha_engine* e);
struct SubmitOptions {   // what an engine request may carry beyond its ids, max_new and req_id: every field absent by default
  const aha_mm_input* mm = nullptr;
  const aha_sampling_params* params = nullptr;   // null: greedy
  const aha_logit_adjust* adjust = nullptr;
  int32_t top_logprobs = -1;                     // -1: no logprobs
  const uint32_t* mask = nullptr;                // n_mask_words packed allowed-token words, or null
  size_t n_mask_words = 0;
  // aha_hip_engine_submit_spec (spec set: checked by spec_config_check; max_draft 0: an ordinary greedy request)
  const aha_spec_config* spec = nullptr;
  const uint32_t* prediction = nullptr;          // n_prediction ids, or null: prompt lookup only
  size_t n_prediction = 0;
};
int engine_submit(aha_engine* e, const uint32_t* ids, size_t n_ids, const SubmitOptions& o, size_t max_new, uint64_t* req_id);
int engine_set_mask(aha_engine* e, uint64_t req_id, const uint32_t* words, size_t n_words);
int engine_cancel(aha_engine* e, uint64_t req_id);
int engine_step(aha_engine* e, aha_engine_event* ev, size_t cap, size_t* n_ev, float* logits_out, aha_token_logprobs* logprobs_out = nullptr);
int engine_stats(const aha_engine* e, aha_engine_stats* out);
int engine_debug_ctr_base(aha_engine* e, uint32_t base);
size_t engine_max_events(const aha_engine* e);
int engine_spec_stats(const aha_engine* e, aha_spec_stats* out);
int engine_request_spec(const aha_engine* e, uint64_t req_id, size_t* n_proposed, size_t* n_accepted);
int model_forward_initial(aha_model* m, const uint32_t* ids, size_t n, size_t offset, const aha_mm_input* mm,
                          float* logits_out, uint32_t* argmax_out);
int model_forward_step(aha_model* m, uint32_t token, size_t offset, float* logits_out, uint32_t* argmax_out);
int model_decode_greedy(aha_model* m, uint32_t first_token, size_t offset, size_t max_new, uint32_t* out);
int model_clear_cache(aha_model* m);
int model_quantize_weights(aha_model* m, int32_t format, uint32_t flags);
int model_last_logits(aha_model* m, float* logits_out);
int model_sample_candidates(aha_model* m, const uint32_t* ctx, size_t n_ctx, float repeat_penalty, float temperature, int k,
                            float* vals_out, uint32_t* idx_out, float* max_out, float* sumexp_out);
int model_ensure_pages(aha_model* m, size_t tokens);
KvLayer model_kv_layer(aha_model* m, int layer);
int model_debug_graph_step(aha_model* m, int replays, double* us_launches, double* us_graph);
int model_kv_export(aha_model* m, void* out_dev, size_t out_bytes, size_t* bytes_needed, size_t* n_tokens, int64_t* rope_delta);
int model_kv_import(aha_model* m, const void* in_dev, size_t in_bytes, int src_heads, int src_head0, int dst_head0, int n_heads, size_t n_tokens,
                    int64_t rope_delta);
int prof_collect(aha_model* m);
int model_allreduce(aha_model* m, float* buf, size_t count);
// loader.hip
int config_parse(const char* dir, aha_model_desc* out);
int config_torch_dtype(const char* dir, std::string* out);
int weights_open(const char* dir, aha_weights** out);
int model_load(aha_ctx* ctx, const char* dir, size_t kv_reserve_tokens, aha_model** out);
int rccl_allreduce(aha_model* m, float* buf, size_t count);  // tp_rccl.hip
int rccl_reduce_scatter(aha_model* m, float* buf, size_t count_per_rank, hipStream_t st = nullptr);   // in place: rank r keeps slice r; st: stream (default: the model's)
int rccl_all_gather(aha_model* m, void* buf, size_t bytes_per_rank, hipStream_t st = nullptr);   // in place: slice r is rank r's contribution
int tp_unique_id(void* out128);
int tp_init_rccl(aha_model* m, const void* id128);
int cp_init_rccl(aha_model* m, const void* id128);
int debug_cp_plan(int S, int world, int rank, int* out5);
void tp_destroy(aha_model* m);

// helpers shared with vision.hip
const aha_tensor_view* find_tensor(const aha_tensor_view* w, size_t nw, const std::string& name);
int upload_tensor(aha_model* m, const aha_tensor_view* t, const std::vector<int64_t>& shape, void** out,
                  int64_t pad_rows_to = 0, int64_t pad_cols_to = 0);
int dev_alloc(aha_model* m, size_t bytes, void** out, bool zero = false);

struct ProfScope {
  aha_model* m;
  int idx = -1;
  ProfScope(aha_model* m, const char* cls, double bytes, double flops);
  ~ProfScope();
};

}  // namespace aha
