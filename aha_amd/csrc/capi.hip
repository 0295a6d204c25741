// extern "C" surface of libaha_hip.so -- see include/aha_hip.h for the contract of every entry point.
#include <math.h>
#include <string.h>

#include <algorithm>
#include <map>
#include <memory>
#include <mutex>
#include <numeric>
#include <vector>

#include "common.h"
#include "model.h"
#include "sampler.h"
#include "audio.h"
#include "vision.h"

namespace aha {
const char* last_error_cstr();
}
using namespace aha;

#define API_GUARD_BEGIN try {
#define API_GUARD_END                                   \
  }                                                     \
  catch (const std::exception& e) {                     \
    set_error(std::string("exception: ") + e.what());   \
    return AHA_ERR_INVALID;                             \
  }                                                     \
  catch (...) {                                         \
    set_error("unknown exception");                     \
    return AHA_ERR_INVALID;                             \
  }

// While an engine exists on a model it owns the cache: the other entries that use it are refused
static int engine_owns_cache(const aha_model* m, const char* who) {
  if (!m->engine) return AHA_OK;
  set_error(std::string(who) + ": the model's cache belongs to its engine (aha_hip_engine_destroy first)");
  return AHA_ERR_STATE;
}

extern "C" {

const char* aha_hip_last_error(void) { return last_error_cstr(); }
const char* aha_hip_version(void) { return "aha-hip 0.2 (gfx950)"; }   // 0.2: aha_mm_input grew (video fields)

int aha_hip_get_dtype(int32_t requested, const char* cfg_dtype, int32_t* out) {
  API_GUARD_BEGIN
  if (!out) {
    set_error("aha_hip_get_dtype: out is null");
    return AHA_ERR_INVALID;
  }
  if (requested >= 0) {   // Some(d) => d
    if (requested != AHA_BF16 && requested != AHA_F16 && requested != AHA_F32) {
      set_error("aha_hip_get_dtype: not a floating-point model dtype");
      return AHA_ERR_INVALID;
    }
    *out = requested;
    return AHA_OK;
  }
  const std::string c = cfg_dtype ? cfg_dtype : "";
  if (c == "float32" || c == "float") *out = AHA_F32;
  else if (c == "float16") *out = AHA_F16;
  else if (c == "bfloat16") *out = AHA_BF16;
  else *out = AHA_F32;
  return AHA_OK;
  API_GUARD_END
}

int aha_hip_check_dtype(int32_t dtype) {
  if (dtype == AHA_BF16) return AHA_OK;
  set_error(std::string("compute dtype ") + (dtype == AHA_F16 ? "f16" : dtype == AHA_F32 ? "f32" : "?") +
            " is not supported: the gfx950 kernels compute in bf16 (f16 / f32 checkpoints are cast to bf16 at load); pass "
            "Some(DType::BF16) or leave the dtype to a bfloat16 checkpoint's config");
  return AHA_ERR_UNSUPPORTED;
}

int aha_hip_init(int device, aha_ctx** out) {
  API_GUARD_BEGIN
  if (!out) {
    set_error("aha_hip_init: out is null");
    return AHA_ERR_INVALID;
  }
  int n = 0;
  AHA_HIP_CHECK(hipGetDeviceCount(&n));
  if (device < 0 || device >= n) {
    set_error("aha_hip_init: device " + std::to_string(device) + " out of range (" + std::to_string(n) + " visible)");
    return AHA_ERR_INVALID;
  }
  AHA_HIP_CHECK(hipSetDevice(device));
  aha_ctx* c = new aha_ctx();
  c->device = device;
  AHA_HIP_CHECK(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
  *out = c;
  return AHA_OK;
  API_GUARD_END
}

void aha_hip_shutdown(aha_ctx* ctx) {
  if (!ctx) return;
  if (ctx->stream) hipStreamDestroy(ctx->stream);
  delete ctx;
}

int aha_hip_model_create(aha_ctx* ctx, const aha_model_desc* desc, const aha_tensor_view* weights, size_t n_weights,
                         aha_model** out) {
  API_GUARD_BEGIN
  if (desc) {
    const int rc = aha_hip_check_dtype(desc->compute_dtype);
    if (rc) return rc;
  }
  return model_create(ctx, desc, weights, n_weights, out);
  API_GUARD_END
}
void aha_hip_model_destroy(aha_model* m) { model_destroy(m); }

int aha_hip_forward_initial(aha_model* m, const uint32_t* input_ids, size_t n_ids, size_t seqlen_offset,
                            const aha_mm_input* mm, float* logits_out, uint32_t* argmax_out) {
  API_GUARD_BEGIN
  if (!m) {
    set_error("null model");
    return AHA_ERR_INVALID;
  }
  if (int rc = engine_owns_cache(m, "forward_initial")) return rc;
  return model_forward_initial(m, input_ids, n_ids, seqlen_offset, mm, logits_out, argmax_out);
  API_GUARD_END
}
int aha_hip_forward_step(aha_model* m, uint32_t token, size_t seqlen_offset, float* logits_out, uint32_t* argmax_out) {
  API_GUARD_BEGIN
  if (!m) {
    set_error("null model");
    return AHA_ERR_INVALID;
  }
  if (int rc = engine_owns_cache(m, "forward_step")) return rc;
  return model_forward_step(m, token, seqlen_offset, logits_out, argmax_out);
  API_GUARD_END
}
int aha_hip_clear_cache(aha_model* m) {
  if (!m) {
    set_error("null model");
    return AHA_ERR_INVALID;
  }
  if (int rc = engine_owns_cache(m, "clear_cache")) return rc;
  return model_clear_cache(m);
}
int aha_hip_stop_token_ids(const aha_model* m, uint32_t* out, size_t cap) {
  if (!m) {
    set_error("null model");
    return AHA_ERR_INVALID;
  }
  const int n = m->desc.n_stop_tokens;
  for (int i = 0; i < n && (size_t)i < cap; ++i) out[i] = m->desc.stop_tokens[i];
  return n;
}
int aha_hip_decode_greedy(aha_model* m, uint32_t first_token, size_t seqlen_offset, size_t max_new, uint32_t* tokens_out) {
  API_GUARD_BEGIN
  if (!m || !tokens_out) {
    set_error("null argument");
    return AHA_ERR_INVALID;
  }
  if (int rc = engine_owns_cache(m, "decode_greedy")) return rc;
  return model_decode_greedy(m, first_token, seqlen_offset, max_new, tokens_out);
  API_GUARD_END
}

int aha_hip_sample_candidates(aha_model* m, const uint32_t* context, size_t n_context, float repeat_penalty, float temperature,
                              int32_t k, float* vals_out, uint32_t* idx_out, float* max_out, float* sumexp_out) {
  API_GUARD_BEGIN
  if (!m) {
    set_error("null handle");
    return AHA_ERR_INVALID;
  }
  return model_sample_candidates(m, context, n_context, repeat_penalty, temperature, k, vals_out, idx_out, max_out, sumexp_out);
  API_GUARD_END
}

int aha_hip_last_logits(aha_model* m, float* logits_out) {
  API_GUARD_BEGIN
  if (!m || !logits_out) {
    set_error("null argument");
    return AHA_ERR_INVALID;
  }
  return model_last_logits(m, logits_out);
  API_GUARD_END
}

size_t aha_hip_cache_len(const aha_model* m) { return m ? m->cache_len : 0; }
int64_t aha_hip_debug_steps_executed(const aha_model* m) { return m ? m->steps_executed : 0; }
int aha_hip_debug_attn_decode_form(const aha_model* m) { return m ? m->last_attn_form : -1; }
int aha_hip_debug_graph_step(aha_model* m, int32_t replays, double* us_launches, double* us_graph) {
  if (!m) return AHA_ERR_INVALID;
  API_GUARD_BEGIN
  if (int rc = engine_owns_cache(m, "debug_graph_step")) return rc;
  return model_debug_graph_step(m, replays, us_launches, us_graph);
  API_GUARD_END
}
int aha_hip_kv_export(aha_model* m, void* out_dev, size_t out_bytes, size_t* bytes_needed, size_t* n_tokens, int64_t* rope_delta) {
  if (!m) return AHA_ERR_INVALID;
  API_GUARD_BEGIN
  if (int rc = engine_owns_cache(m, "kv_export")) return rc;
  return model_kv_export(m, out_dev, out_bytes, bytes_needed, n_tokens, rope_delta);
  API_GUARD_END
}
int aha_hip_kv_import(aha_model* m, const void* in_dev, size_t in_bytes, int32_t src_heads, int32_t src_head0, int32_t dst_head0, int32_t n_heads,
                      size_t n_tokens, int64_t rope_delta) {
  if (!m) return AHA_ERR_INVALID;
  API_GUARD_BEGIN
  if (int rc = engine_owns_cache(m, "kv_import")) return rc;
  return model_kv_import(m, in_dev, in_bytes, src_heads, src_head0, dst_head0, n_heads, n_tokens, rope_delta);
  API_GUARD_END
}

int aha_hip_set_profiling(aha_model* m, int enable) {
  if (!m) return AHA_ERR_INVALID;
  int rc = prof_collect(m);
  if (rc) return rc;
  m->profiling = enable != 0;
  if (enable)
    for (auto& a : m->prof_acc) a = aha_model::ProfAcc();
  return AHA_OK;
}
int aha_hip_get_profile(aha_model* m, const char* kernel_class, double* total_ms, int64_t* launches, double* bytes,
                        double* flops) {
  if (!m || !kernel_class) return AHA_ERR_INVALID;
  int rc = prof_collect(m);
  if (rc) return rc;
  auto it = m->prof_cls.find(kernel_class);
  aha_model::ProfAcc a;
  if (it != m->prof_cls.end()) a = m->prof_acc[it->second];
  if (total_ms) *total_ms = a.ms;
  if (launches) *launches = a.n;
  if (bytes) *bytes = a.bytes;
  if (flops) *flops = a.flops;
  return AHA_OK;
}
int aha_hip_debug_scramble_pages(aha_model* m, int enable) {
  if (!m) return AHA_ERR_INVALID;
  m->scramble_pages = enable != 0;
  if (enable && !m->free_pages.empty()) {
    uint64_t s = 0x2545F4914F6CDD1Dull;
    for (size_t i = m->free_pages.size(); i > 1; --i) {
      s = s * 6364136223846793005ull + 1442695040888963407ull;
      std::swap(m->free_pages[i - 1], m->free_pages[(s >> 33) % i]);
    }
  }
  return AHA_OK;
}
int aha_hip_debug_poison_lds(uint32_t seed, void* stream) {
  API_GUARD_BEGIN
  launch_poison_lds(seed, (hipStream_t)stream);
  AHA_HIP_CHECK(hipGetLastError());
  return AHA_OK;
  API_GUARD_END
}
int aha_hip_debug_attn_variant(int32_t smx) {
  if (smx < -1 || smx > 3 || smx == 2) {
    set_error("debug_attn_variant: smx -1 (default), 0, 1 or 3");
    return AHA_ERR_INVALID;
  }
  set_attn_variant_override(smx);
  return AHA_OK;
}
int aha_hip_debug_attn_form(int32_t form) {
  if (form != -1 && form != 16 && form != 64 && form != 65) {
    set_error("debug_attn_form: -1 (automatic), 16, 64 or 65");
    return AHA_ERR_INVALID;
  }
  set_attn_form_override(form);
  return AHA_OK;
}
int aha_hip_debug_gemm_plan(int32_t tile, int32_t splitk) {
  const bool sk = tile == 1256 || tile == 1192;   // the persistent kernel; splitk = style * 10 + cuts of the last round (0 = the planner's)
  if ((tile != 0 && tile != 128 && tile != 2128 && tile != 256 && tile != 192 && !sk) || splitk < 0 || (!sk && splitk > 8) ||
      (sk && !(splitk <= 4 || (splitk >= 11 && splitk <= 13)))) {
    set_error("debug_gemm_plan: tile must be 0, 128, 2128 (256 x 128), 192 (256 x 192, where instantiated), 256 or 1256 / 1192 (persistent kernel); splitk 0..8 "
              "(persistent: 0..4 equal pieces, 11..13 big pieces + remainder)");
    return AHA_ERR_INVALID;
  }
  set_gemm_plan_override(tile, splitk);
  return AHA_OK;
}
int aha_hip_debug_plan_gemm(int32_t M, int32_t N, int32_t K, int32_t act, int32_t has_bias, int32_t has_residual, size_t workspace_bytes,
                            int32_t* out3) {
  if (!out3 || M <= 0 || N <= 0 || K <= 0) {
    set_error("debug_plan_gemm: bad argument");
    return AHA_ERR_INVALID;
  }
  int o[3];
  debug_plan_gemm(M, N, K, act, has_bias != 0, (has_residual & 1) != 0, workspace_bytes, o, (has_residual & 2) != 0);
  out3[0] = o[0]; out3[1] = o[1]; out3[2] = o[2];
  return AHA_OK;
}
int aha_hip_debug_streamk_plan(int32_t M, int32_t N, int32_t K, int32_t tile_n, int32_t workers, size_t workspace_bytes, int32_t* out,
                               int32_t cap, int32_t* off_out, int32_t* info7) {
  if (!out || cap < 0 || M <= 0 || N <= 0 || K <= 0) {
    set_error("debug_streamk_plan: bad argument");
    return AHA_ERR_INVALID;
  }
  const int n = debug_streamk_plan(M, N, K, tile_n, workers, 8, workspace_bytes, out, cap, off_out, info7);
  if (n < 0) {
    set_error("debug_streamk_plan: K must be a multiple of 64, workers a multiple of 8, tile_n 256 or 192, and the workspace must hold the chunks");
    return AHA_ERR_INVALID;
  }
  return n;
}
int aha_hip_set_gemm_reserved_cus(int32_t n) {
  set_gemm_reserved_cus(n);
  return AHA_OK;
}
int aha_hip_debug_last_hidden(aha_model* m, float* out, size_t n) {
  API_GUARD_BEGIN
  if (!m || !out || n != (size_t)m->desc.hidden_size) {
    set_error("debug_last_hidden: bad size");
    return AHA_ERR_INVALID;
  }
  std::vector<uint16_t> tmp(n);
  AHA_HIP_CHECK(hipMemcpy(tmp.data(), m->d_hlast, n * 2, hipMemcpyDeviceToHost));
  for (size_t i = 0; i < n; ++i) {
    uint32_t u = (uint32_t)tmp[i] << 16;
    memcpy(&out[i], &u, 4);
  }
  return AHA_OK;
  API_GUARD_END
}

// ---- op-level entry points --------------------------------------------------------------------------------------
namespace {
struct DevBuf {   // a small device allocation freed on every return path
  void* p = nullptr;
  ~DevBuf() { if (p) hipFree(p); }
  int upload(const void* host, size_t bytes) {
    AHA_HIP_CHECK(hipMalloc(&p, bytes));
    AHA_HIP_CHECK(hipMemcpy(p, host, bytes, hipMemcpyHostToDevice));
    return AHA_OK;
  }
};
}  // namespace

int aha_hip_rmsnorm(const void* x, const void* w, void* y, int64_t rows, int32_t dim, float eps, void* stream) {
  if (!x || !w || !y || dim % 8 || dim > 8192) {
    set_error("rmsnorm: dim must be a multiple of 8 and <= 8192");
    return AHA_ERR_INVALID;
  }
  launch_rmsnorm_rows(x, w, y, rows, dim, dim, dim, eps, (hipStream_t)stream);
  AHA_HIP_CHECK(hipGetLastError());
  return AHA_OK;
}

int aha_hip_gemv(const void* W, const void* x, void* y, int32_t N, int32_t K, const void* norm_w, float eps,
                 const void* residual, void* stream) {
  if (!W || !x || !y || K % 8 || K > 32768) {
    set_error("gemv: K must be a multiple of 8 and <= 32768");
    return AHA_ERR_INVALID;
  }
  GemvArgs g{};
  g.W = W; g.x = x; g.y = y; g.N = N; g.K = K; g.norm_w = norm_w; g.eps = eps; g.residual = residual;
  launch_gemv(g, residual ? GEMV_RESIDUAL : GEMV_STORE, (hipStream_t)stream);
  AHA_HIP_CHECK(hipGetLastError());
  return AHA_OK;
}

int aha_hip_gemv_gate_up(const void* Wg, const void* Wu, const void* x, void* y, int32_t I, int32_t K,
                         const void* norm_w, float eps, void* stream) {
  if (!Wg || !Wu || !x || !y || K % 8 || K > 32768) {
    set_error("gemv_gate_up: bad arguments");
    return AHA_ERR_INVALID;
  }
  GemvArgs g{};
  g.W = Wg; g.W2 = Wu; g.x = x; g.y = y; g.N = I; g.K = K; g.norm_w = norm_w; g.eps = eps;
  launch_gemv(g, GEMV_SILU_MUL, (hipStream_t)stream);
  AHA_HIP_CHECK(hipGetLastError());
  return AHA_OK;
}

// the op-level GEMM entries' split-K scratch (aha_hip_gemm, aha_hip_debug_gemm_layernorm): one per DEVICE, grown on demand; not for
// concurrent callers
static void op_gemm_scratch(GemmArgs& g) {
  const int M = g.M, N = g.N;
  struct OpScratch { void* ws = nullptr; size_t ws_bytes = 0; void* ctrs = nullptr; };
  static std::map<int, OpScratch> scratch_by_dev;
  static std::mutex scratch_mu;   // the map is reachable from several devices / threads; a device's scratch itself is still one caller at a time
  int cur_dev = 0;
  if (hipGetDevice(&cur_dev) != hipSuccess) (void)hipGetLastError();
  std::unique_lock<std::mutex> scratch_lk(scratch_mu);
  OpScratch& sc = scratch_by_dev[cur_dev];
  const size_t want = std::max((size_t)4 * M * N * 4, (size_t)96 << 20);   // split-K slabs / >= 384 chunks of the persistent kernel
  if (want > sc.ws_bytes && want <= ((size_t)1 << 30)) {
    if (sc.ws) hipFree(sc.ws);
    sc.ws = nullptr;
    sc.ws_bytes = 0;
    if (hipMalloc(&sc.ws, want) == hipSuccess) sc.ws_bytes = want;
  }
  // the persistent kernel's per-tile counters (zero between launches)
  if (!sc.ctrs && (hipMalloc(&sc.ctrs, SK_MAX_COUNTERS * 4) != hipSuccess || hipMemset(sc.ctrs, 0, SK_MAX_COUNTERS * 4) != hipSuccess)) sc.ctrs = nullptr;
  g.workspace = sc.ws;
  g.workspace_bytes = sc.ws_bytes;
  g.sk_counters = sc.ws ? sc.ctrs : nullptr;
}

int aha_hip_gemm(const void* A, const void* W, void* C, int32_t M, int32_t N, int32_t K, int32_t lda, int32_t ldw,
                 int32_t ldc, const void* bias, const void* residual, int32_t act, void* stream) {
  if (!A || !W || !C || K % 8 || N % 8 || lda % 8 || ldw % 8 || ldc % 4 || act < 0 || act > ACT_SILU_MUL_PAIRS) {
    set_error("gemm: K, N, lda, ldw must be multiples of 8 (16-byte rows), ldc of 4");
    return AHA_ERR_INVALID;
  }
  if (act == ACT_SILU_MUL_PAIRS && (N % 32 || bias || residual)) {
    set_error("gemm: ACT_SILU_MUL_PAIRS needs N % 32 == 0 and no bias/residual");
    return AHA_ERR_INVALID;
  }
  GemmArgs g{};
  g.A = A; g.W = W; g.C = C; g.M = M; g.N = N; g.K = K; g.lda = lda; g.ldw = ldw; g.ldc = ldc; g.bias = bias; g.residual = residual; g.act = act;
  op_gemm_scratch(g);
  launch_gemm(g, (hipStream_t)stream);
  AHA_HIP_CHECK(hipGetLastError());
  return AHA_OK;
}

// ---- op-level test entries of the towers' row kernels (tests/test_tower_rows_gpu.py) ------------------------------------------------------
int aha_hip_debug_layernorm_rows(const void* x, const void* w, const void* b, void* y, int64_t rows, int32_t dim, float eps, void* stream) {
  if (!x || !w || !b || !y || rows < 1 || dim < 8 || dim % 8 || dim > 8192) {
    set_error("debug_layernorm_rows: null pointer, rows < 1, or dim not a multiple of 8 in 8 .. 8192");
    return AHA_ERR_INVALID;
  }
  launch_layernorm_rows(x, w, b, y, rows, dim, eps, (hipStream_t)stream);
  AHA_HIP_CHECK(hipGetLastError());
  return AHA_OK;
}

int aha_hip_debug_gemm_layernorm(const void* A, const void* W, void* C, int32_t M, int32_t N, int32_t K, int32_t lda, int32_t ldw, int32_t ldc,
                                 const void* bias, const void* residual, int32_t act, const void* norm_w, const void* norm_b, void* norm_out,
                                 float eps, void* stream) {
  if (!A || !W || !C || !norm_w || !norm_b || !norm_out) {
    set_error("debug_gemm_layernorm: null pointer");
    return AHA_ERR_INVALID;
  }
  if (M < 1 || N < 8 || K < 8 || K % 8 || N % 8 || N > 8192 || lda % 8 || ldw % 8 || lda < K || ldw < K || ldc != N || act < 0 || act >= ACT_SILU_MUL_PAIRS) {
    set_error("debug_gemm_layernorm: M >= 1, K, N, lda, ldw multiples of 8, N <= 8192 (the LayerNorm's row), ldc == N (the norm reads C's rows "
              "back to back), act below the gate+up pairs");
    return AHA_ERR_INVALID;
  }
  GemmArgs g{};
  g.A = A; g.W = W; g.C = C; g.M = M; g.N = N; g.K = K; g.lda = lda; g.ldw = ldw; g.ldc = ldc; g.bias = bias; g.residual = residual; g.act = act;
  g.norm_w = norm_w; g.norm_b = norm_b; g.norm_out = norm_out; g.norm_eps = eps;
  op_gemm_scratch(g);
  launch_gemm(g, (hipStream_t)stream);
  AHA_HIP_CHECK(hipGetLastError());
  return AHA_OK;
}

namespace {
// the grids of a tower test entry: t >= 1, h and w positive multiples of merge; -> the patch rows they describe, or -1
int64_t check_vit_grids(const uint32_t* grid_thw, int32_t n_grids, int32_t merge) {
  if (!grid_thw || n_grids < 1 || merge < 1) return -1;
  int64_t N = 0;
  for (int i = 0; i < n_grids; ++i) {
    const uint32_t* g = grid_thw + 3 * i;
    if (g[0] < 1 || g[1] < 1 || g[2] < 1 || g[1] % merge || g[2] % merge || g[0] > 4096 || g[1] > 4096 || g[2] > 4096) return -1;
    N += (int64_t)g[0] * g[1] * g[2];
    if (N > (1 << 24)) return -1;
  }
  return N;
}
void vit_host_tables(const uint32_t* grid_thw, int32_t n_grids, int G, int merge, VisHostTables* ht) {
  std::vector<const uint32_t*> grids(n_grids);
  for (int i = 0; i < n_grids; ++i) grids[i] = grid_thw + 3 * i;
  vision_host_tables(grids.data(), grids.size(), G, merge, ht);
}
}  // namespace

int aha_hip_debug_vit_pos_embed(const uint32_t* grid_thw, int32_t n_grids, int32_t G, int32_t merge, const void* table, void* x, int64_t N,
                                int32_t D, int32_t* idx_out, float* wt_out, void* stream) {
  API_GUARD_BEGIN
  const char* who = "debug_vit_pos_embed: ";
  auto bad = [&](const std::string& why) {
    set_error(who + why);
    return AHA_ERR_INVALID;
  };
  if (!grid_thw || !table || !x || !idx_out || !wt_out) return bad("null pointer");
  if (G < 1 || G > 4096 || D < 8 || D % 8) return bad("the table side must be 1 .. 4096 and D a positive multiple of 8");
  const int64_t rows = check_vit_grids(grid_thw, n_grids, merge);
  if (rows < 0) return bad("n_grids, merge >= 1 and every grid t >= 1, h and w positive multiples of merge (each at most 4096, 2^24 rows in all)");
  if (rows != N) return bad("the grids describe " + std::to_string(rows) + " rows, N is " + std::to_string(N));
  VisHostTables ht;
  vit_host_tables(grid_thw, n_grids, G, merge, &ht);
  hipStream_t st = (hipStream_t)stream;
  DevBuf d_idx, d_wt;
  int rc;
  if ((rc = d_idx.upload(ht.idx.data(), ht.idx.size() * 4)) || (rc = d_wt.upload(ht.wt.data(), ht.wt.size() * 4))) return rc;
  launch_pos_embed_add(x, table, (const int32_t*)d_idx.p, (const float*)d_wt.p, N, D, st);
  hipError_t e = hipGetLastError();
  hipStreamSynchronize(st);   // (the tables above are freed on return)
  AHA_HIP_CHECK(e);
  memcpy(idx_out, ht.idx.data(), ht.idx.size() * 4);
  memcpy(wt_out, ht.wt.data(), ht.wt.size() * 4);
  return AHA_OK;
  API_GUARD_END
}

int aha_hip_debug_vit_rope(const void* qkv, const uint32_t* grid_thw, int32_t n_grids, int32_t merge, const float* inv_freq,
                           const uint64_t* page_ptrs, int32_t n_page_ptrs, int64_t N, int32_t nh, int32_t hd, float* cs_tab, void* q_out,
                           int32_t* rowcol_out, int32_t* page_of_out, int32_t* slot_of_out, void* stream) {
  API_GUARD_BEGIN
  const char* who = "debug_vit_rope: ";
  auto bad = [&](const std::string& why) {
    set_error(who + why);
    return AHA_ERR_INVALID;
  };
  if (!qkv || !grid_thw || !inv_freq || !page_ptrs || !cs_tab || !q_out || !rowcol_out || !page_of_out || !slot_of_out) return bad("null pointer");
  if (hd != 72) return bad("head_dim must be 72");
  if (nh < 1 || nh > 1024) return bad("nh outside 1 .. 1024");
  const int64_t rows = check_vit_grids(grid_thw, n_grids, merge);
  if (rows < 0) return bad("n_grids, merge >= 1 and every grid t >= 1, h and w positive multiples of merge (each at most 4096, 2^24 rows in all)");
  if (rows != N) return bad("the grids describe " + std::to_string(rows) + " rows, N is " + std::to_string(N));
  VisHostTables ht;
  vit_host_tables(grid_thw, n_grids, 0, merge, &ht);
  if (n_page_ptrs < 1 || ht.pages > n_page_ptrs)
    return bad("the call writes " + std::to_string(ht.pages) + " pages, page_ptrs holds " + std::to_string(n_page_ptrs));
  hipStream_t st = (hipStream_t)stream;
  DevBuf d_rowcol, d_page_of, d_slot_of, d_first, d_cnt;
  int rc;
  if ((rc = d_rowcol.upload(ht.rowcol.data(), ht.rowcol.size() * 4)) || (rc = d_page_of.upload(ht.page_of.data(), ht.page_of.size() * 4)) ||
      (rc = d_slot_of.upload(ht.slot_of.data(), ht.slot_of.size() * 4)) || (rc = d_first.upload(ht.page_first.data(), ht.page_first.size() * 4)) ||
      (rc = d_cnt.upload(ht.page_cnt.data(), ht.page_cnt.size() * 4)))
    return rc;
  launch_vit_rope_table((const int32_t*)d_rowcol.p, inv_freq, (int)N, hd, cs_tab, st);
  VitRopeArgs r{};
  r.qkv = qkv; r.rowcol = (const int32_t*)d_rowcol.p; r.inv_freq = inv_freq; r.page_of = (const int32_t*)d_page_of.p;
  r.slot_of = (const int32_t*)d_slot_of.p; r.q_out = q_out;
  r.kv.page_ptrs = page_ptrs; r.kv.layer_off = 0; r.kv.kvh = nh; r.kv.d = hd;
  r.N = (int)N; r.nh = nh; r.hd = hd; r.cs_tab = cs_tab;
  r.page_first = (const int32_t*)d_first.p; r.page_cnt = (const int32_t*)d_cnt.p; r.n_pages = (int)ht.pages;
  launch_vit_rope_pack(r, st);
  hipError_t e = hipGetLastError();
  hipStreamSynchronize(st);   // (the tables above are freed on return)
  AHA_HIP_CHECK(e);
  memcpy(rowcol_out, ht.rowcol.data(), ht.rowcol.size() * 4);
  memcpy(page_of_out, ht.page_of.data(), ht.page_of.size() * 4);
  memcpy(slot_of_out, ht.slot_of.data(), ht.slot_of.size() * 4);
  return AHA_OK;
  API_GUARD_END
}

int aha_hip_debug_scatter_rows(void* dst, const void* src, const int32_t* rows, int64_t n, int64_t dst_rows, int32_t D, int32_t add, void* stream) {
  API_GUARD_BEGIN
  const char* who = "debug_scatter_rows: ";
  auto bad = [&](const std::string& why) {
    set_error(who + why);
    return AHA_ERR_INVALID;
  };
  if (!dst || !src || !rows) return bad("null pointer");
  if (n < 1 || n > (1 << 24) || dst_rows < 1 || D < 8 || D % 8 || (add != 0 && add != 1)) return bad("n, dst_rows >= 1, D a positive multiple of 8, add 0 or 1");
  for (int64_t i = 0; i < n; ++i)
    if (rows[i] < 0 || rows[i] >= dst_rows) return bad("rows[" + std::to_string(i) + "] outside the destination");
  hipStream_t st = (hipStream_t)stream;
  DevBuf d_rows;
  if (int rc = d_rows.upload(rows, (size_t)n * 4)) return rc;
  launch_scatter_rows(dst, src, (const int32_t*)d_rows.p, n, D, add, st);
  hipError_t e = hipGetLastError();
  hipStreamSynchronize(st);
  AHA_HIP_CHECK(e);
  return AHA_OK;
  API_GUARD_END
}

int aha_hip_debug_audio_im2col1(const float* feat, int64_t ld, const int32_t* chunks, int32_t C, int32_t mels, int32_t win, void* out, void* stream) {
  API_GUARD_BEGIN
  const char* who = "debug_audio_im2col1: ";
  auto bad = [&](const std::string& why) {
    set_error(who + why);
    return AHA_ERR_INVALID;
  };
  if (!feat || !chunks || !out) return bad("null pointer");
  if (C < 1 || C > (1 << 20) || mels < 1 || mels > 4096 || win < 1 || win > 4096 || ld < 1) return bad("C, mels, win, ld must be positive");
  for (int i = 0; i < C; ++i) {   // {first column of the clip, its frames, window index}: the window starts inside the clip, the clip inside a row
    const int64_t base = chunks[3 * i], F = chunks[3 * i + 1], ci = chunks[3 * i + 2];
    if (base < 0 || F < 1 || base + F > ld || ci < 0 || ci * win >= F) return bad("chunk " + std::to_string(i) + " outside its clip, or its clip outside the feature rows");
  }
  hipStream_t st = (hipStream_t)stream;
  DevBuf d_chunks;
  if (int rc = d_chunks.upload(chunks, (size_t)C * 3 * 4)) return rc;
  launch_audio_im2col1(feat, (const int32_t*)d_chunks.p, out, ld, C, mels, win, st);
  hipError_t e = hipGetLastError();
  hipStreamSynchronize(st);
  AHA_HIP_CHECK(e);
  return AHA_OK;
  API_GUARD_END
}

int aha_hip_debug_im2col_nhwc(const void* in, void* out, int32_t B, int32_t Hin, int32_t Win, int32_t Cin, void* stream) {
  if (!in || !out || B < 1 || Hin < 1 || Win < 1 || Cin < 8 || Cin % 8 || (int64_t)B * Hin * Win > (1 << 26)) {
    set_error("debug_im2col_nhwc: null pointer, a non-positive size, or Cin not a positive multiple of 8");
    return AHA_ERR_INVALID;
  }
  launch_im2col_nhwc(in, out, B, Hin, Win, Cin, (hipStream_t)stream);
  AHA_HIP_CHECK(hipGetLastError());
  return AHA_OK;
}

int aha_hip_debug_audio_tokens_gather(const void* in, void* out, int32_t B, int32_t Fq, int32_t T, int32_t Cc, void* stream) {
  if (!in || !out || B < 1 || Fq < 1 || T < 1 || Cc < 1 || (int64_t)B * Fq * T * Cc > ((int64_t)1 << 32)) {
    set_error("debug_audio_tokens_gather: null pointer or a non-positive size");
    return AHA_ERR_INVALID;
  }
  launch_audio_tokens_gather(in, out, B, Fq, T, Cc, (hipStream_t)stream);
  AHA_HIP_CHECK(hipGetLastError());
  return AHA_OK;
}

int aha_hip_debug_sinus_pe_add(void* x, int64_t rows, int32_t d, int32_t T, void* stream) {
  if (!x || rows < 1 || d < 2 || d % 2 || T < 1) {
    set_error("debug_sinus_pe_add: null pointer, rows or T < 1, or d not a positive even number");
    return AHA_ERR_INVALID;
  }
  launch_sinus_pe_add(x, rows, d, T, (hipStream_t)stream);
  AHA_HIP_CHECK(hipGetLastError());
  return AHA_OK;
}

int aha_hip_debug_kv_pack_generic(const void* src, int64_t ld, int32_t k_off, int32_t v_off, const uint64_t* page_ptrs, int32_t n_page_ptrs,
                                  int32_t N, int32_t nh, int32_t hd, const int32_t* slot_of, void* stream) {
  API_GUARD_BEGIN
  const char* who = "debug_kv_pack_generic: ";
  auto bad = [&](const std::string& why) {
    set_error(who + why);
    return AHA_ERR_INVALID;
  };
  if (!src || !page_ptrs) return bad("null pointer");
  if (N < 1 || N > (1 << 24) || nh < 1 || nh > 1024 || hd < 32 || hd % 32 || hd > 256 || n_page_ptrs < 1) return bad("N, nh, n_page_ptrs >= 1 and head_dim a multiple of 32 in 32 .. 256");
  const int64_t width = (int64_t)nh * hd;
  if (k_off < 0 || v_off < 0 || k_off + width > ld || v_off + width > ld) return bad("the K or V heads run past the row pitch ld");
  const int64_t slots = (int64_t)n_page_ptrs * KV_PAGE_TOKENS;
  if (!slot_of && N > slots) return bad("N rows need more pages than page_ptrs holds");
  for (int n = 0; slot_of && n < N; ++n)   // slot_of (HOST here): the cache slot of every row
    if (slot_of[n] < 0 || slot_of[n] >= slots) return bad("slot_of[" + std::to_string(n) + "] outside the pages of the call");
  hipStream_t st = (hipStream_t)stream;
  DevBuf d_slot;
  if (slot_of)
    if (int rc = d_slot.upload(slot_of, (size_t)N * 4)) return rc;
  KvLayer kv{};
  kv.page_ptrs = page_ptrs; kv.layer_off = 0; kv.kvh = nh; kv.d = hd;
  launch_kv_pack_generic(src, ld, k_off, v_off, kv, N, nh, hd, st, (const int32_t*)d_slot.p);
  hipError_t e = hipGetLastError();
  hipStreamSynchronize(st);
  AHA_HIP_CHECK(e);
  return AHA_OK;
  API_GUARD_END
}

int aha_hip_debug_gemm_grouped(const void* A, const void* W, void* C, int32_t M, int32_t N, int32_t K, int32_t ldc, int32_t act,
                               int32_t groups, int32_t a_gstride, int32_t c_gstride, int32_t c_row0, int32_t m_total, void* stream) {
  if (!A || !W || !C || M <= 0 || N <= 0 || K % 8 || N % 8 || ldc % 4 || (act != ACT_NONE && act != ACT_SILU_MUL_PAIRS) || groups < 1 ||
      a_gstride < M || c_gstride < 0 || c_row0 < 0 || m_total < 0 || (act == ACT_SILU_MUL_PAIRS && N % 32)) {
    set_error("debug_gemm_grouped: bad argument");
    return AHA_ERR_INVALID;
  }
  GemmArgs g{};
  g.A = A; g.W = W; g.C = C; g.M = M; g.N = N; g.K = K; g.lda = K; g.ldw = K; g.ldc = ldc; g.act = act;
  g.groups = groups; g.a_gstride = a_gstride; g.c_gstride = c_gstride; g.c_row0 = c_row0; g.m_total = m_total;
  launch_gemm_grouped(g, (hipStream_t)stream);
  AHA_HIP_CHECK(hipGetLastError());
  return AHA_OK;
}

int aha_hip_qknorm_rope(const void* qkv, const void* q_norm_w, const void* k_norm_w, const int32_t* pos,
                        const int32_t* axis_map, void* q_out, void* k_out, void* v_out, int32_t S, int32_t nh,
                        int32_t kvh, int32_t d, float eps, float theta, void* stream) {
  API_GUARD_BEGIN
  if (d != 128) {
    set_error("qknorm_rope: head_dim must be 128");
    return AHA_ERR_UNSUPPORTED;
  }
  hipStream_t st = (hipStream_t)stream;
  std::vector<float> inv(d / 2);
  for (int i = 0; i < d / 2; ++i) inv[i] = 1.0f / powf(theta, (float)(2 * i) / (float)d);
  float* d_inv = nullptr;
  AHA_HIP_CHECK(hipMalloc((void**)&d_inv, inv.size() * 4));
  AHA_HIP_CHECK(hipMemcpy(d_inv, inv.data(), inv.size() * 4, hipMemcpyHostToDevice));
  RopeArgs r{};
  r.qkv = qkv; r.ld = (int64_t)(nh + 2 * kvh) * d; r.q_norm_w = q_norm_w; r.k_norm_w = k_norm_w; r.pos = pos; r.pos_ld = S;
  r.inv_freq = d_inv; r.axis_map = axis_map; r.q_out = q_out; r.k_out = k_out; r.v_out = v_out;
  r.kv.page_ptrs = nullptr; r.S = S; r.nh = nh; r.kvh = kvh; r.d = d; r.eps = eps;
  launch_qknorm_rope(r, st);
  AHA_HIP_CHECK(hipGetLastError());
  AHA_HIP_CHECK(hipStreamSynchronize(st));
  hipFree(d_inv);
  return AHA_OK;
  API_GUARD_END
}

namespace {
struct TmpPages {
  void* store = nullptr;
  uint64_t* d_ptrs = nullptr;
  int32_t* d_len = nullptr;
  void* fused = nullptr;   // head_dim 64 entry: the [K | V] rows the audio tower's packer reads (freed here: every early return is covered)
  KvLayer kv{};
  ~TmpPages() {
    if (fused) hipFree(fused);
    if (store) hipFree(store);
    if (d_ptrs) hipFree(d_ptrs);
    if (d_len) hipFree(d_len);
  }
};
int build_tmp_pages(TmpPages& t, const void* k, const void* v, int L, int kvh, int d, hipStream_t st) {
  const int npages = (L + KV_PAGE_TOKENS - 1) / KV_PAGE_TOKENS;
  const size_t page_bytes = (size_t)2 * kvh * KV_PAGE_TOKENS * d * 2;
  AHA_HIP_CHECK(hipMalloc(&t.store, page_bytes * npages));
  AHA_HIP_CHECK(hipMemsetAsync(t.store, 0, page_bytes * npages, st));
  std::vector<uint64_t> ptrs(npages);
  // hand the pages out back to front so the test exercises the indirection
  for (int i = 0; i < npages; ++i) ptrs[i] = (uint64_t)(uintptr_t)t.store + (size_t)(npages - 1 - i) * page_bytes;
  AHA_HIP_CHECK(hipMalloc((void**)&t.d_ptrs, npages * 8));
  AHA_HIP_CHECK(hipMemcpy(t.d_ptrs, ptrs.data(), npages * 8, hipMemcpyHostToDevice));
  AHA_HIP_CHECK(hipMalloc((void**)&t.d_len, 4));
  AHA_HIP_CHECK(hipMemcpy(t.d_len, &L, 4, hipMemcpyHostToDevice));
  t.kv.page_ptrs = t.d_ptrs;
  t.kv.layer_off = 0;
  t.kv.kvh = kvh;
  t.kv.d = d;
  launch_kv_pack_pages(k, v, t.kv, L, st);
  AHA_HIP_CHECK(hipGetLastError());
  return AHA_OK;
}
}  // namespace

int aha_hip_debug_attn_prefill_segs(const void* q, const void* k, const void* v, void* o, int32_t nh, int32_t kvh, const int32_t* segs,
                                    int32_t n_seg, int32_t with_kv0, float scale, void* stream) {
  API_GUARD_BEGIN
  if (!q || !k || !v || !o || !segs || n_seg < 1 || kvh < 1 || nh % kvh || nh / kvh > 16) {
    set_error("debug_attn_prefill_segs: bad arguments");
    return AHA_ERR_INVALID;
  }
  const int d = 128;
  std::vector<int32_t> seg(3 * (size_t)n_seg), kv0(n_seg);
  int S = 0;
  for (int j = 0; j < n_seg; ++j) {
    const int len = segs[2 * j], k0 = segs[2 * j + 1];
    if (len < 1 || k0 < 0 || k0 % KV_PAGE_TOKENS || (!with_kv0 && k0)) {
      set_error("debug_attn_prefill_segs: segment " + std::to_string(j) + " needs len >= 1 and kv0 a multiple of 64 (0 without with_kv0)");
      return AHA_ERR_INVALID;
    }
    kv0[j] = k0;
  }
  hipStream_t st = (hipStream_t)stream;
  // every segment's cache on pages of its own (handed out back to front), the page tables back to back
  std::vector<std::unique_ptr<TmpPages>> tp;
  std::vector<uint64_t> ptrs;
  int64_t c0 = 0;
  const size_t row_bytes = (size_t)kvh * d * 2, page_bytes = (size_t)2 * kvh * KV_PAGE_TOKENS * d * 2;
  for (int j = 0; j < n_seg; ++j) {
    const int len = segs[2 * j], L = kv0[j] + len, np = (L + KV_PAGE_TOKENS - 1) / KV_PAGE_TOKENS;
    tp.emplace_back(new TmpPages());
    if (int rc = build_tmp_pages(*tp.back(), (const char*)k + c0 * row_bytes, (const char*)v + c0 * row_bytes, L, kvh, d, st)) return rc;
    seg[3 * j] = S, seg[3 * j + 1] = len, seg[3 * j + 2] = (int32_t)ptrs.size();
    for (int i = 0; i < np; ++i) ptrs.push_back((uint64_t)(uintptr_t)tp.back()->store + (size_t)(np - 1 - i) * page_bytes);
    S += len;
    c0 += L;
  }
  const std::vector<int32_t> items = seg_items_of(seg, true, with_kv0 ? &kv0 : nullptr);
  std::vector<int32_t> tab(seg);
  tab.insert(tab.end(), items.begin(), items.end());
  tab.insert(tab.end(), kv0.begin(), kv0.end());
  uint64_t* d_ptrs = nullptr;
  int32_t* d_tab = nullptr;
  AHA_HIP_CHECK(hipMalloc((void**)&d_ptrs, ptrs.size() * 8));
  if (hipMalloc((void**)&d_tab, tab.size() * 4) != hipSuccess) {
    hipFree(d_ptrs);
    set_error("debug_attn_prefill_segs: hipMalloc failed");
    return AHA_ERR_HIP;
  }
  hipMemcpy(d_ptrs, ptrs.data(), ptrs.size() * 8, hipMemcpyHostToDevice);
  hipMemcpy(d_tab, tab.data(), tab.size() * 4, hipMemcpyHostToDevice);
  AttnPrefillArgs a{};
  a.q = q; a.q_ld = (int64_t)nh * d; a.kv.page_ptrs = d_ptrs; a.kv.layer_off = 0; a.kv.kvh = kvh; a.kv.d = d; a.o = o;
  a.S = S; a.nh = nh; a.kvh = kvh; a.d = d; a.kv_offset = 0; a.kv_total = S; a.causal = 1; a.scale = scale;
  a.seg_tab = d_tab; a.seg_items = d_tab + seg.size(); a.n_items = (int)items.size() / 2;
  a.seg_kv0 = with_kv0 ? d_tab + seg.size() + items.size() : nullptr;
  launch_attn_prefill(a, st);
  hipError_t e = hipGetLastError();
  hipStreamSynchronize(st);
  hipFree(d_ptrs);
  hipFree(d_tab);
  AHA_HIP_CHECK(e);
  return AHA_OK;
  API_GUARD_END
}

int aha_hip_debug_prefill_rope(const void* qkv, const void* q_norm_w, const void* k_norm_w, const int32_t* pos, const int32_t* axis_map,
                               const float* inv_freq, const uint64_t* page_ptrs, int32_t n_page_ptrs, int32_t S, int32_t nh, int32_t kvh,
                               int32_t d, float eps, int32_t form, int32_t kv_start, int32_t skip_q, const int32_t* row_slot,
                               const int32_t* page_rows, int32_t n_pages, void* rope_tab, void* q_out, void* stream) {
  API_GUARD_BEGIN
  const char* who = "debug_prefill_rope: ";
  auto bad = [&](const std::string& why) {
    set_error(who + why);
    return AHA_ERR_INVALID;
  };
  // (q_out even with skip_q: with AHA_ROPE_ROWS=0 the per-element kernel runs instead, and it writes the q heads whatever skip_q says)
  if (!qkv || !q_norm_w || !k_norm_w || !pos || !axis_map || !inv_freq || !page_ptrs || !rope_tab || !q_out) return bad("null pointer");
  if (d != 128) return bad("head_dim must be 128");
  if (S < 1 || S > (1 << 24) || nh < 1 || kvh < 1 || nh > 1024 || kvh > 1024 || n_page_ptrs < 1) return bad("S outside 1 .. 2^24, nh or kvh outside 1 .. 1024, or n_page_ptrs < 1");
  if (form < AHA_ROPE_FORM_TABLE || form > AHA_ROPE_FORM_PACKED) return bad("form must be 0 .. 3");
  if (skip_q != 0 && skip_q != 1) return bad("skip_q must be 0 or 1");
  if (form == AHA_ROPE_FORM_PACKED && !skip_q) return bad("the packed form writes K and V only (skip_q = 1)");
  if (form == AHA_ROPE_FORM_DEVICE_START && skip_q) return bad("the per-element kernel always writes the q heads (skip_q = 0)");
  if (skip_q && form != AHA_ROPE_FORM_PACKED && S < 16) return bad("skip_q needs the row-vectorised kernel (S >= 16)");
  const int64_t slots = (int64_t)n_page_ptrs * KV_PAGE_TOKENS;
  if (form == AHA_ROPE_FORM_PACKED) {
    if (!row_slot || !page_rows) return bad("the packed form needs row_slot and page_rows");
    if (n_pages < 1 || n_pages > n_page_ptrs) return bad("n_pages outside 1 .. n_page_ptrs");
    for (int r = 0; r < S; ++r)
      if (row_slot[r] < 0 || row_slot[r] >= (int64_t)n_pages * KV_PAGE_TOKENS) return bad("row_slot[" + std::to_string(r) + "] outside the pages of the call");
    for (int p = 0; p < n_pages; ++p) {
      const int r0 = page_rows[2 * p], n = page_rows[2 * p + 1];
      if (r0 < 0 || n < 1 || n > KV_PAGE_TOKENS || (int64_t)r0 + n > S) return bad("page_rows of page " + std::to_string(p) + " outside the rows of the call");
    }
  } else {
    if (kv_start < 0 || (int64_t)kv_start + S > slots) return bad("the cache range [kv_start, kv_start + S) runs past the page table");
  }
  hipStream_t st = (hipStream_t)stream;
  DevBuf d_start, d_slot, d_prow;
  int rc;
  if (form == AHA_ROPE_FORM_DEVICE_START && (rc = d_start.upload(&kv_start, 4))) return rc;
  if (form == AHA_ROPE_FORM_PACKED &&
      ((rc = d_slot.upload(row_slot, (size_t)S * 4)) || (rc = d_prow.upload(page_rows, (size_t)n_pages * 2 * 4))))
    return rc;
  launch_rope_table(pos, S, inv_freq, axis_map, S, rope_tab, st);   // stage 1: cos / sin once, as the prefill has them for all layers
  RopeArgs r{};
  r.qkv = qkv; r.ld = (int64_t)(nh + 2 * kvh) * d; r.q_norm_w = q_norm_w; r.k_norm_w = k_norm_w; r.pos = pos; r.pos_ld = S;
  r.inv_freq = inv_freq; r.axis_map = axis_map; r.q_out = q_out;
  r.kv.page_ptrs = page_ptrs; r.kv.layer_off = 0; r.kv.kvh = kvh; r.kv.d = d;
  r.S = S; r.nh = nh; r.kvh = kvh; r.d = d; r.eps = eps; r.skip_q = skip_q;
  switch (form) {
    case AHA_ROPE_FORM_TABLE: r.kv_start_host = kv_start; r.rope_tab = rope_tab; break;           // forward_initial_impl's call
    case AHA_ROPE_FORM_NO_TABLE: r.kv_start_host = kv_start; break;                               // the angles computed in place
    case AHA_ROPE_FORM_DEVICE_START: r.kv_start_host = -1; r.kv_start = (const int32_t*)d_start.p; break;
    default:                                                                                      // packed_layers' call
      r.kv_start_host = 0; r.rope_tab = rope_tab;
      r.row_slot = (const int32_t*)d_slot.p; r.page_rows = (const int32_t*)d_prow.p; r.n_pages = n_pages;
  }
  launch_qknorm_rope(r, st);
  hipError_t e = hipGetLastError();
  hipStreamSynchronize(st);   // (the tables above are freed on return)
  AHA_HIP_CHECK(e);
  return AHA_OK;
  API_GUARD_END
}

int aha_hip_debug_prefill_attn_qfuse(const void* qkv, const void* q_norm_w, const void* rope_tab, const uint64_t* page_ptrs,
                                     int32_t n_page_ptrs, int32_t S, int32_t nh, int32_t kvh, int32_t d, float eps, float scale,
                                     int32_t kv_offset, int32_t kv_total, int32_t S2, int32_t kv_offset2, int32_t kv_total2,
                                     const int32_t* segs, int32_t n_seg, int32_t with_kv0, void* o, void* stream) {
  API_GUARD_BEGIN
  const char* who = "debug_prefill_attn_qfuse: ";
  auto bad = [&](const std::string& why) {
    set_error(who + why);
    return AHA_ERR_INVALID;
  };
  if (!qkv || !q_norm_w || !rope_tab || !page_ptrs || !o) return bad("null pointer");
  if (d != 128) return bad("head_dim must be 128");
  if (S < 1 || S > (1 << 24) || nh < 1 || kvh < 1 || nh % kvh || nh / kvh > 16 || n_page_ptrs < 1)
    return bad("S outside 1 .. 2^24, n_page_ptrs < 1, nh not a multiple of kvh, or a group size above 16");
  const int64_t slots = (int64_t)n_page_ptrs * KV_PAGE_TOKENS;
  std::vector<int32_t> tab;
  size_t o_items = 0, o_kv0 = 0;
  int n_items = 0;
  if (n_seg > 0) {
    if (!segs || S2 != 0) return bad("a packed launch needs segs and takes no second segment");
    std::vector<int32_t> seg(3 * (size_t)n_seg), kv0(n_seg);
    int64_t rows = 0;
    for (int j = 0; j < n_seg; ++j) {
      const int len = segs[3 * j], p0 = segs[3 * j + 1], k0 = segs[3 * j + 2];
      if (len < 1 || p0 < 0 || k0 < 0 || k0 % KV_PAGE_TOKENS || (!with_kv0 && k0) || (int64_t)k0 + len > (1 << 24) ||
          (int64_t)p0 * KV_PAGE_TOKENS + k0 + len > slots)
        return bad("segment " + std::to_string(j) + ": len >= 1, kv0 a multiple of 64 (0 without with_kv0), its cache within the page table");
      seg[3 * j] = (int32_t)rows, seg[3 * j + 1] = len, seg[3 * j + 2] = p0, kv0[j] = k0;
      rows += len;
    }
    if (rows != S) return bad("the segments' lengths must add up to S");
    const std::vector<int32_t> items = seg_items_of(seg, true, with_kv0 ? &kv0 : nullptr);
    n_items = (int)items.size() / 2;
    tab = seg;
    o_items = tab.size();
    tab.insert(tab.end(), items.begin(), items.end());
    o_kv0 = tab.size();
    tab.insert(tab.end(), kv0.begin(), kv0.end());
  } else {
    if (n_seg < 0 || S2 < 0 || S2 > (1 << 24)) return bad("n_seg and S2 must be >= 0");
    if (kv_offset < 0 || kv_total < 1 || kv_total > slots || (int64_t)kv_offset + S > kv_total)
      return bad("rows [kv_offset, kv_offset + S) must lie within kv_total cache tokens within the page table");
    if (S2 > 0 && (kv_offset2 < 0 || kv_total2 < 1 || kv_total2 > slots || (int64_t)kv_offset2 + S2 > kv_total2))
      return bad("second segment: rows [kv_offset2, kv_offset2 + S2) must lie within kv_total2 cache tokens within the page table");
  }
  AttnPrefillArgs a{};
  a.q = qkv; a.q_ld = (int64_t)(nh + 2 * kvh) * d; a.kv.page_ptrs = page_ptrs; a.kv.layer_off = 0; a.kv.kvh = kvh; a.kv.d = d; a.o = o;
  a.S = S; a.nh = nh; a.kvh = kvh; a.d = d; a.causal = 1; a.scale = scale;
  a.q_norm_w = q_norm_w; a.q_rope_tab = rope_tab; a.q_eps = eps;
  if (n_seg > 0) {
    a.kv_offset = 0; a.kv_total = S;
    a.seg_tab = tab.data();   // (host address: only its presence matters to the form; the device copy replaces it below)
  } else {
    a.kv_offset = kv_offset; a.kv_total = kv_total; a.S2 = S2; a.kv_offset2 = kv_offset2; a.kv_total2 = kv_total2;
  }
  if (!attn_prefill_takes_qfuse(a)) {
    set_error(std::string(who) + "the attention form these arguments select does not norm and rotate Q itself");
    return AHA_ERR_UNSUPPORTED;
  }
  hipStream_t st = (hipStream_t)stream;
  DevBuf d_tab;
  if (n_seg > 0) {
    if (int rc = d_tab.upload(tab.data(), tab.size() * 4)) return rc;
    const int32_t* t = (const int32_t*)d_tab.p;
    a.seg_tab = t; a.seg_items = t + o_items; a.n_items = n_items;
    a.seg_kv0 = with_kv0 ? t + o_kv0 : nullptr;
  }
  launch_attn_prefill(a, st);
  hipError_t e = hipGetLastError();
  hipStreamSynchronize(st);
  AHA_HIP_CHECK(e);
  return AHA_OK;
  API_GUARD_END
}

int aha_hip_attn_decode(const void* q, const void* k, const void* v, void* o, int32_t nh, int32_t kvh, int32_t d,
                        int32_t L, float scale, void* stream) {
  API_GUARD_BEGIN
  if (d != 128 || L <= 0 || nh % kvh || nh / kvh > 16) {
    set_error("attn_decode: head_dim must be 128, L > 0, group size <= 16");
    return AHA_ERR_UNSUPPORTED;
  }
  hipStream_t st = (hipStream_t)stream;
  TmpPages t;
  int rc = build_tmp_pages(t, k, v, L, kvh, d, st);
  if (rc) return rc;
  const int npages = (L + KV_PAGE_TOKENS - 1) / KV_PAGE_TOKENS;
  const int nsplit = std::max(1, std::min((npages + 3) / 4, 64));
  float *po = nullptr, *pml = nullptr;
  AHA_HIP_CHECK(hipMalloc((void**)&po, (size_t)nsplit * 4 * nh * d * 4));
  AHA_HIP_CHECK(hipMalloc((void**)&pml, (size_t)nsplit * 4 * nh * 2 * 4));
  AttnDecodeArgs a{};
  a.q = q; a.kv = t.kv; a.kv_len = t.d_len; a.part_o = po; a.part_ml = pml; a.o = o; a.nh = nh; a.kvh = kvh; a.d = d;
  a.nsplit = nsplit; a.scale = scale;
  launch_attn_decode(a, st);
  hipError_t e = hipGetLastError();
  hipStreamSynchronize(st);
  hipFree(po);
  hipFree(pml);
  AHA_HIP_CHECK(e);
  return AHA_OK;
  API_GUARD_END
}

// ---- batched decode, op level (scratch allocated per call: test / measurement entries) ----
// One body for the three weight forms: W and scales == nullptr for bf16 weights (K % 8 == 0), (q, scales) for an MXFP8 (mx == 8) or
// MXFP4 (mx == 4) copy (K % 32 == 0).
static int gemv_rows_op(int mx, const void* W, const uint32_t* scales, const void* x, void* y, int32_t R, int32_t N, int32_t K, int32_t epi,
                        const void* residual, float* logits, uint32_t* argmax_out, void* stream) {
  const int kmul = mx ? 32 : 8;
  if (!W || (mx && !scales) || !x || R < 1 || R > 32 || N < 1 || K < kmul || K % kmul || epi < 0 || epi > 3 || (epi == 1 && (!residual || !y)) ||
      ((epi == 0 || epi == 2) && !y) || (epi == 2 && N % 32) || (epi == 3 && (!logits || !argmax_out))) {
    if (!mx) set_error("gemv_rows: bad arguments (1 <= R <= 32, K % 8 == 0, epi 0..3 with its outputs; epi 2 needs N % 32 == 0)");
    else set_error(std::string("gemv_rows_mxfp") + (mx == 8 ? "8" : "4") +
                   ": bad arguments (q, scales, 1 <= R <= 32, K % 32 == 0, epi 0..3 with its outputs; epi 2 needs N % 32 == 0)");
    return AHA_ERR_INVALID;
  }
  hipStream_t st = (hipStream_t)stream;
  const int tiles = gemv_rows_num_tiles(N);
  float *ws = nullptr, *bm = nullptr;
  uint32_t* bi = nullptr;
  AHA_HIP_CHECK(hipMalloc((void**)&ws, gemv_rows_ws_floats(R, N, K) * 4));
  AHA_HIP_CHECK(hipMalloc((void**)&bm, (size_t)R * tiles * 4));
  AHA_HIP_CHECK(hipMalloc((void**)&bi, (size_t)R * tiles * 4));
  GemvRowsArgs a{};
  a.W = mx ? nullptr : W; a.x = x; a.ldx = K; a.R = R; a.N = N; a.K = K; a.ws = ws;
  a.y = y; a.residual = residual; a.ldy = epi == 2 ? N / 2 : N;
  a.y_f32 = logits; a.ldf = N; a.blk_max = bm; a.blk_idx = bi;
  const GemvEpi e = epi == 0 ? GEMV_STORE : epi == 1 ? GEMV_RESIDUAL : epi == 2 ? GEMV_SILU_MUL : GEMV_LOGITS;
  if (mx == 8) launch_gemv_rows_mxfp8(a, W, scales, e, st);
  else if (mx == 4) launch_gemv_rows_mxfp4(a, W, scales, e, st);
  else launch_gemv_rows(a, e, st);
  if (epi == 3) launch_argmax_rows(bm, bi, tiles, R, argmax_out, st);
  hipError_t err = hipGetLastError();
  hipStreamSynchronize(st);
  hipFree(ws);
  hipFree(bm);
  hipFree(bi);
  AHA_HIP_CHECK(err);
  return AHA_OK;
}

int aha_hip_gemv_rows(const void* W, const void* x, void* y, int32_t R, int32_t N, int32_t K, int32_t epi, const void* residual,
                      float* logits, uint32_t* argmax_out, void* stream) {
  API_GUARD_BEGIN
  return gemv_rows_op(0, W, nullptr, x, y, R, N, K, epi, residual, logits, argmax_out, stream);
  API_GUARD_END
}

int aha_hip_gemv_rows_mxfp8(const void* q, const uint32_t* scales, const void* x, void* y, int32_t R, int32_t N, int32_t K, int32_t epi,
                            const void* residual, float* logits, uint32_t* argmax_out, void* stream) {
  API_GUARD_BEGIN
  return gemv_rows_op(8, q, scales, x, y, R, N, K, epi, residual, logits, argmax_out, stream);
  API_GUARD_END
}

int aha_hip_gemv_rows_mxfp4(const void* q, const uint32_t* scales, const void* x, void* y, int32_t R, int32_t N, int32_t K, int32_t epi,
                            const void* residual, float* logits, uint32_t* argmax_out, void* stream) {
  API_GUARD_BEGIN
  return gemv_rows_op(4, q, scales, x, y, R, N, K, epi, residual, logits, argmax_out, stream);
  API_GUARD_END
}

static int quantize_mx_op(int mx, const void* W, int32_t N, int32_t K, void* q_out, uint32_t* scales_out, void* w_roundtrip_out, void* stream) {
  if (!W || !q_out || !scales_out || N < 1 || K < 32 || K % 32) {
    set_error(std::string("quantize_mxfp") + (mx == 8 ? "8" : "4") +
              ": bad arguments (W, q_out, scales_out, N >= 1, K a positive multiple of 32)");
    return AHA_ERR_INVALID;
  }
  hipStream_t st = (hipStream_t)stream;
  if (mx == 8) launch_mxfp8_quantize(W, N, K, q_out, scales_out, w_roundtrip_out, st);
  else launch_mxfp4_quantize(W, N, K, q_out, scales_out, w_roundtrip_out, st);
  AHA_HIP_CHECK(hipGetLastError());
  AHA_HIP_CHECK(hipStreamSynchronize(st));
  return AHA_OK;
}

int aha_hip_quantize_mxfp8(const void* W, int32_t N, int32_t K, void* q_out, uint32_t* scales_out, void* w_roundtrip_out, void* stream) {
  API_GUARD_BEGIN
  return quantize_mx_op(8, W, N, K, q_out, scales_out, w_roundtrip_out, stream);
  API_GUARD_END
}

int aha_hip_quantize_mxfp4(const void* W, int32_t N, int32_t K, void* q_out, uint32_t* scales_out, void* w_roundtrip_out, void* stream) {
  API_GUARD_BEGIN
  return quantize_mx_op(4, W, N, K, q_out, scales_out, w_roundtrip_out, stream);
  API_GUARD_END
}

int aha_hip_model_quantize_weights(aha_model* m, int32_t format, uint32_t flags) {
  API_GUARD_BEGIN
  if (!m) {
    set_error("quantize_weights: null model");
    return AHA_ERR_INVALID;
  }
  return model_quantize_weights(m, format, flags);
  API_GUARD_END
}

int aha_hip_model_weight_format(const aha_model* m, int32_t* format, uint32_t* flags) {
  if (!m) {
    set_error("weight_format: null model");
    return AHA_ERR_INVALID;
  }
  if (format) *format = m->wq_format;
  if (flags) *flags = m->wq_flags;
  return AHA_OK;
}

int aha_hip_debug_fp8_rows(aha_model* m, int on) {
  if (!m) {
    set_error("debug_fp8_rows: null model");
    return AHA_ERR_INVALID;
  }
  m->fp8_rows = on != 0;
  return AHA_OK;
}

int aha_hip_debug_fp8_single(aha_model* m, int on) {
  if (!m) {
    set_error("debug_fp8_single: null model");
    return AHA_ERR_INVALID;
  }
  if (on < 0 || on > 2) {
    set_error("debug_fp8_single: on must be 0 (bf16), 1 (by plan) or 2 (every matrix with a copy)");
    return AHA_ERR_INVALID;
  }
  m->fp8_single = on;
  return AHA_OK;
}

int aha_hip_debug_pk13_single(aha_model* m, int on) {
  if (!m) {
    set_error("debug_pk13_single: null model");
    return AHA_ERR_INVALID;
  }
  if (on < 0 || on > 2) {
    set_error("debug_pk13_single: on must be 0 (bf16), 1 (by plan) or 2 (every matrix with a copy)");
    return AHA_ERR_INVALID;
  }
  m->pk13_single = on;
  return AHA_OK;
}

int aha_hip_pk13_status(const aha_model* m, char* buf, size_t cap) {
  if (!m || (!buf && cap)) {
    set_error("pk13_status: null model or buffer");
    return AHA_ERR_INVALID;
  }
  std::string s;
  int n = 0;
  for (const Pk13Entry& e : m->pk13) {
    s += e.name + "\t" + e.status + "\n";
    n += e.slot->p != nullptr;
  }
  if (cap) {
    const size_t k = std::min(s.size(), cap - 1);
    memcpy(buf, s.data(), k);
    buf[k] = 0;
  }
  return n;
}

int aha_hip_debug_fp4_single(aha_model* m, int on) {
  if (!m) {
    set_error("debug_fp4_single: null model");
    return AHA_ERR_INVALID;
  }
  if (on < 0 || on > 2) {
    set_error("debug_fp4_single: on must be 0 (bf16), 1 (by plan) or 2 (every matrix with a copy)");
    return AHA_ERR_INVALID;
  }
  m->fp4_single = on;
  return AHA_OK;
}

// aha_hip_debug_plan_gemv_mxfp8 / _mxfp4 (mx: 8 / 4)
static int debug_plan_gemv_mx(int mx, int32_t N, int32_t K, int32_t epi, int32_t has_norm, int32_t* R, int32_t* U, int32_t* grid, int32_t* form,
                              int32_t* by_plan) {
  if (!R || !U || !grid || N < 1 || K < 32 || K % 32 || epi < 0 || epi > 3 || (epi == 2 && N % 32)) {
    set_error(std::string("debug_plan_gemv_mxfp") + (mx == 8 ? "8" : "4") +
              ": bad argument (N >= 1, K a positive multiple of 32, epi 0..3, epi 2 needs N % 32 == 0)");
    return AHA_ERR_INVALID;
  }
  int o[5];
  (mx == 8 ? debug_plan_gemv_mxfp8 : debug_plan_gemv_mxfp4)(epi == 2 ? N / 2 : N, K, (GemvEpi)epi, has_norm != 0, o);
  *R = o[0]; *U = o[1]; *grid = o[2];
  if (form) *form = o[3] ? 1 + o[4] : 0;
  if (by_plan) *by_plan = (mx == 8 ? gemv_mxfp8_by_plan : gemv_mxfp4_by_plan)(N, K, (GemvEpi)epi) ? 1 : 0;
  return AHA_OK;
}

int aha_hip_debug_plan_gemv_mxfp8(int32_t N, int32_t K, int32_t epi, int32_t has_norm, int32_t* R, int32_t* U, int32_t* grid, int32_t* form,
                                  int32_t* by_plan) {
  return debug_plan_gemv_mx(8, N, K, epi, has_norm, R, U, grid, form, by_plan);
}

int aha_hip_debug_plan_gemv_pk13(int32_t N, int32_t K, int32_t epi, int32_t has_norm, int32_t* R, int32_t* U, int32_t* grid, int32_t* form,
                                 int32_t* by_plan) {
  if (!R || !U || !grid || epi < 0 || epi > 3 || (epi == 2 && N % 32) || !gemv_pk13_shape_ok(N, K)) {
    set_error("debug_plan_gemv_pk13: bad argument (N >= 1, K a multiple of 4096 and at most 32768, epi 0..3, epi 2 needs N % 32 == 0)");
    return AHA_ERR_INVALID;
  }
  int o[5];
  debug_plan_gemv_pk13(epi == 2 ? N / 2 : N, K, (GemvEpi)epi, has_norm != 0, o);
  *R = o[0]; *U = o[1]; *grid = o[2];
  if (form) *form = 1 + o[4];
  if (by_plan) *by_plan = gemv_pk13_by_plan(N, K, (GemvEpi)epi) ? 1 : 0;
  return AHA_OK;
}

int aha_hip_debug_plan_gemv_mxfp4(int32_t N, int32_t K, int32_t epi, int32_t has_norm, int32_t* R, int32_t* U, int32_t* grid, int32_t* form,
                                  int32_t* by_plan) {
  return debug_plan_gemv_mx(4, N, K, epi, has_norm, R, U, grid, form, by_plan);
}

int aha_hip_debug_plan_gemv(int32_t N, int32_t K, int32_t epi, int32_t has_norm, int32_t* R, int32_t* U, int32_t* grid, int32_t* form) {
  if (!R || !U || !grid || N < 1 || K < 8 || K % 8 || K > 32768 || epi < 0 || epi > 4 || (epi == 2 && N % 2)) {
    set_error("debug_plan_gemv: bad argument (N >= 1, K a positive multiple of 8 and at most 32768, epi 0..4, epi 2 needs an even N)");
    return AHA_ERR_INVALID;
  }
  int o[5];
  debug_plan_gemv(epi == 2 ? N / 2 : N, K, (GemvEpi)epi, has_norm != 0, o);
  *R = o[0]; *U = o[1]; *grid = o[2];
  if (form) *form = o[3] ? 1 + o[4] : 0;
  return AHA_OK;
}

int aha_hip_debug_plan_gemv_rows(int32_t N, int32_t K, int32_t* cw, int32_t* nks) {
  if (!cw || !nks || N < 1 || K < 8 || K % 8) {
    set_error("debug_plan_gemv_rows: bad argument (cw, nks not null, N >= 1, K a positive multiple of 8)");
    return AHA_ERR_INVALID;
  }
  int c, s;
  gemv_rows_plan(N, K, &c, &s);
  *cw = c; *nks = s;
  return AHA_OK;
}

int aha_hip_debug_gemv_partial_f32(const void* W, const void* x, float* y_f32, int32_t N, int32_t K, const void* norm_w, float eps,
                                   void* stream) {
  API_GUARD_BEGIN
  if (!W || !x || !y_f32 || N < 1 || K < 8 || K % 8 || K > 32768) {
    set_error("debug_gemv_partial_f32: bad argument (W, x, y_f32 not null, N >= 1, K a positive multiple of 8 and at most 32768)");
    return AHA_ERR_INVALID;
  }
  GemvArgs g{};
  g.W = W; g.x = x; g.y_f32 = y_f32; g.N = N; g.K = K; g.norm_w = norm_w; g.eps = eps;
  launch_gemv(g, GEMV_PARTIAL_F32, (hipStream_t)stream);
  AHA_HIP_CHECK(hipGetLastError());
  return AHA_OK;
  API_GUARD_END
}

// ---- batch-1 matvec with an epilogue, op level (the partials of epi 3 are allocated per call: test / measurement entries) ----
namespace {
struct GemvPartials {   // released when the call returns, on the error paths too
  void* p[2] = {nullptr, nullptr};
  ~GemvPartials() {
    for (void* q : p)
      if (q) hipFree(q);
  }
};
const char* gemv_epi_args_bad(const void* w, const void* x, const void* y, int N, int K, int kmul, int epi, const void* residual,
                              const float* logits, const uint32_t* argmax_out) {
  if (!w || !x) return "null matrix or x";
  if (N < 1) return "N must be at least 1";
  if (K < kmul || K % kmul) return kmul == 32 ? "K must be a positive multiple of 32 (the MX block)" : "K must be a positive multiple of 8";
  if (K > 32768) return "K must be at most 32768";
  if (epi < 0 || epi > 3) return "epi must be 0..3";
  if (epi != 3 && !y) return "null y";
  if (epi == 1 && !residual) return "epi 1 needs a residual";
  if (epi == 2 && N % 32) return "epi 2 needs N % 32 == 0";
  if (epi == 3 && (!logits || !argmax_out)) return "epi 3 needs logits and argmax_out";
  return nullptr;
}
}  // namespace

// q: the MXFP8 (mx == 8) or MXFP4 (mx == 4) copy in place of W, or the exact 13-bit copy (mx == 13, its base in pk13_bh)
static int gemv_epi_run(const void* W, int mx, const void* q, const uint32_t* scales, const void* x, void* y, int32_t N, int32_t K,
                        int32_t epi, const void* norm_w, float eps, const void* residual, float* logits, uint32_t* argmax_out, void* stream,
                        int pk13_bh = 0, const int32_t* pk13_rows = nullptr, int pk13_nrows = 0) {
  hipStream_t st = (hipStream_t)stream;
  GemvArgs g{};
  g.W = W; g.x = x; g.y = y; g.N = epi == 2 ? N / 2 : N; g.K = K; g.norm_w = norm_w; g.eps = eps; g.residual = epi == 1 ? residual : nullptr;
  g.y_f32 = logits;
  const GemvEpi e = epi == 0 ? GEMV_STORE : epi == 1 ? GEMV_RESIDUAL : epi == 2 ? GEMV_SILU_MUL : GEMV_LOGITS;
  GemvPartials part;
  int tiles = 0;
  if (epi == 3) {
    tiles = !q ? gemv_num_tiles(N, K) : mx == 8 ? gemv_mxfp8_num_tiles(N, K) : mx == 13 ? gemv_pk13_num_tiles(N, K) : gemv_mxfp4_num_tiles(N, K);
    AHA_HIP_CHECK(hipMalloc(&part.p[0], (size_t)tiles * 4));
    AHA_HIP_CHECK(hipMalloc(&part.p[1], (size_t)tiles * 4));
    g.blk_max = (float*)part.p[0];
    g.blk_idx = (uint32_t*)part.p[1];
  }
  if (!q) launch_gemv(g, e, st);
  else if (mx == 8) launch_gemv_mxfp8(g, q, scales, e, st);
  else if (mx == 13) launch_gemv_pk13(g, q, pk13_bh, pk13_rows, pk13_nrows, e, st);   // g.W: the bf16 matrix, read for the exception rows
  else launch_gemv_mxfp4(g, q, scales, e, st);
  if (epi == 3) launch_argmax_partials(g.blk_max, g.blk_idx, tiles, argmax_out, st);
  hipError_t err = hipGetLastError();
  if (epi == 3) {   // the partials are freed on return
    const hipError_t e2 = hipStreamSynchronize(st);
    if (err == hipSuccess) err = e2;
  }
  AHA_HIP_CHECK(err);
  return AHA_OK;
}

int aha_hip_gemv_epi(const void* W, const void* x, void* y, int32_t N, int32_t K, int32_t epi, const void* norm_w, float eps,
                     const void* residual, float* logits, uint32_t* argmax_out, void* stream) {
  API_GUARD_BEGIN
  if (const char* bad = gemv_epi_args_bad(W, x, y, N, K, 8, epi, residual, logits, argmax_out)) {
    set_error(std::string("gemv_epi: ") + bad);
    return AHA_ERR_INVALID;
  }
  return gemv_epi_run(W, 0, nullptr, nullptr, x, y, N, K, epi, norm_w, eps, residual, logits, argmax_out, stream);
  API_GUARD_END
}

int aha_hip_gemv_mxfp8(const void* q, const uint32_t* scales, const void* x, void* y, int32_t N, int32_t K, int32_t epi, const void* norm_w,
                       float eps, const void* residual, float* logits, uint32_t* argmax_out, void* stream) {
  API_GUARD_BEGIN
  if (!scales) {
    set_error("gemv_mxfp8: null scales");
    return AHA_ERR_INVALID;
  }
  if (const char* bad = gemv_epi_args_bad(q, x, y, N, K, 32, epi, residual, logits, argmax_out)) {
    set_error(std::string("gemv_mxfp8: ") + bad);
    return AHA_ERR_INVALID;
  }
  return gemv_epi_run(nullptr, 8, q, scales, x, y, N, K, epi, norm_w, eps, residual, logits, argmax_out, stream);
  API_GUARD_END
}

int aha_hip_gemv_pk13(const void* packed, int32_t bh, const void* x, void* y, int32_t N, int32_t K, int32_t epi, const void* norm_w,
                      float eps, const void* residual, float* logits, uint32_t* argmax_out, void* stream) {
  API_GUARD_BEGIN
  if (const char* bad = gemv_epi_args_bad(packed, x, y, N, K, 8, epi, residual, logits, argmax_out)) {
    set_error(std::string("gemv_pk13: ") + bad);
    return AHA_ERR_INVALID;
  }
  if (K % 4096) {
    set_error("gemv_pk13: K must be a multiple of 4096 (the unit)");
    return AHA_ERR_INVALID;
  }
  if (bh < 0 || bh > 112) {
    set_error("gemv_pk13: bh must be 0..112");
    return AHA_ERR_INVALID;
  }
  return gemv_epi_run(nullptr, 13, packed, nullptr, x, y, N, K, epi, norm_w, eps, residual, logits, argmax_out, stream, bh);
  API_GUARD_END
}

int aha_hip_pack_pk13(const void* W, int32_t N, int32_t K, void* out, int32_t* bh_out, int64_t* bad_out, void* stream) {
  API_GUARD_BEGIN
  if (!W || !bh_out || !bad_out || N < 1 || K < 4096 || K % 4096) {
    set_error("pack_pk13: bad argument (W, bh_out, bad_out not null, N >= 1, K a positive multiple of 4096)");
    return AHA_ERR_INVALID;
  }
  hipStream_t st = (hipStream_t)stream;
  GemvPartials d;
  AHA_HIP_CHECK(hipMalloc(&d.p[0], sizeof(Pk13Stats)));
  AHA_HIP_CHECK(hipMemsetAsync(d.p[0], 0, sizeof(Pk13Stats), st));
  launch_pk13_stats(W, N, K, (Pk13Stats*)d.p[0], st);
  AHA_HIP_CHECK(hipGetLastError());
  Pk13Stats h{};
  AHA_HIP_CHECK(hipMemcpyAsync(&h, d.p[0], sizeof(h), hipMemcpyDeviceToHost, st));
  AHA_HIP_CHECK(hipStreamSynchronize(st));
  *bh_out = pk13_base(h.max_e2);
  *bad_out = (int64_t)h.bad;
  if (out && !h.bad) {
    launch_pk13_pack(W, N, K, *bh_out, out, st);
    AHA_HIP_CHECK(hipGetLastError());
    AHA_HIP_CHECK(hipStreamSynchronize(st));
  }
  return AHA_OK;
  API_GUARD_END
}

int aha_hip_pack_pk13_rows(const void* W, int32_t N, int32_t K, void* out, int32_t* bh_out, int32_t* rows_out, int32_t cap, int32_t* nrows_out,
                           int64_t* below_out, int64_t* nonfinite_out, void* stream) {
  API_GUARD_BEGIN
  if (!W || !bh_out || !rows_out || !nrows_out || !below_out || !nonfinite_out || cap < 0 || cap > PK13_MAX_EXC || N < 1 || K < 4096 || K % 4096) {
    set_error("pack_pk13_rows: bad argument (W and the outputs not null, cap 0..16, N >= 1, K a positive multiple of 4096)");
    return AHA_ERR_INVALID;
  }
  hipStream_t st = (hipStream_t)stream;
  GemvPartials d;
  AHA_HIP_CHECK(hipMalloc(&d.p[0], sizeof(Pk13Stats)));
  AHA_HIP_CHECK(hipMemsetAsync(d.p[0], 0, sizeof(Pk13Stats), st));
  launch_pk13_stats(W, N, K, (Pk13Stats*)d.p[0], st);
  AHA_HIP_CHECK(hipGetLastError());
  Pk13Stats h{};
  AHA_HIP_CHECK(hipMemcpyAsync(&h, d.p[0], sizeof(h), hipMemcpyDeviceToHost, st));
  AHA_HIP_CHECK(hipStreamSynchronize(st));
  int rows[PK13_MAX_EXC];
  const int n = pk13_exception_rows(h, rows);
  *bh_out = pk13_base(h.max_e2);
  *nonfinite_out = (int64_t)h.nonfinite;
  *below_out = (int64_t)(h.bad - h.nonfinite);
  *nrows_out = n;
  for (int i = 0; i < cap && i < n && n <= PK13_MAX_EXC; ++i) rows_out[i] = rows[i];
  if (out && !h.nonfinite && n <= cap) {
    launch_pk13_pack(W, N, K, *bh_out, out, st);
    AHA_HIP_CHECK(hipGetLastError());
    AHA_HIP_CHECK(hipStreamSynchronize(st));
  }
  return AHA_OK;
  API_GUARD_END
}

int aha_hip_gemv_pk13_rows(const void* packed, int32_t bh, const void* W, const int32_t* rows, int32_t nrows, const void* x, void* y, int32_t N,
                           int32_t K, int32_t epi, const void* norm_w, float eps, const void* residual, float* logits, uint32_t* argmax_out,
                           void* stream) {
  API_GUARD_BEGIN
  if (const char* bad = gemv_epi_args_bad(packed, x, y, N, K, 8, epi, residual, logits, argmax_out)) {
    set_error(std::string("gemv_pk13_rows: ") + bad);
    return AHA_ERR_INVALID;
  }
  if (K % 4096) {
    set_error("gemv_pk13_rows: K must be a multiple of 4096 (the unit)");
    return AHA_ERR_INVALID;
  }
  if (bh < 0 || bh > 112) {
    set_error("gemv_pk13_rows: bh must be 0..112");
    return AHA_ERR_INVALID;
  }
  if (nrows < 0 || nrows > PK13_MAX_EXC || (nrows > 0 && (!W || !rows))) {
    set_error("gemv_pk13_rows: nrows must be 0..16, and rows need W and the list");
    return AHA_ERR_INVALID;
  }
  for (int i = 0; i < nrows; ++i)
    if (rows[i] < 0 || rows[i] >= N) {
      set_error("gemv_pk13_rows: row " + std::to_string(rows[i]) + " is not a row of the matrix");
      return AHA_ERR_INVALID;
    }
  return gemv_epi_run(W, 13, packed, nullptr, x, y, N, K, epi, norm_w, eps, residual, logits, argmax_out, stream, bh, rows, nrows);
  API_GUARD_END
}

int aha_hip_gemv_mxfp4(const void* q, const uint32_t* scales, const void* x, void* y, int32_t N, int32_t K, int32_t epi, const void* norm_w,
                       float eps, const void* residual, float* logits, uint32_t* argmax_out, void* stream) {
  API_GUARD_BEGIN
  if (!scales) {
    set_error("gemv_mxfp4: null scales");
    return AHA_ERR_INVALID;
  }
  if (const char* bad = gemv_epi_args_bad(q, x, y, N, K, 32, epi, residual, logits, argmax_out)) {
    set_error(std::string("gemv_mxfp4: ") + bad);
    return AHA_ERR_INVALID;
  }
  return gemv_epi_run(nullptr, 4, q, scales, x, y, N, K, epi, norm_w, eps, residual, logits, argmax_out, stream);
  API_GUARD_END
}

namespace {
struct DevFree {   // device buffers released when the call returns, on the error paths too
  void* p[2] = {nullptr, nullptr};
  ~DevFree() {
    for (void* q : p)
      if (q) hipFree(q);
  }
};
}  // namespace

// aha_hip_sample_rows / aha_hip_sample_rows_adjusted / aha_hip_sample_rows_masked (adj_offsets == nullptr: no addends; mask_rows ==
// nullptr: no masks)
static int sample_rows_impl(const float* logits, int64_t ld, int32_t R, int32_t V, const int32_t* k, const float* temperature,
                            const float* repeat_penalty, const uint32_t* context, const size_t* context_offsets, const uint32_t* adj_ids,
                            const float* adj_vals, const size_t* adj_offsets, float* vals_out, uint32_t* idx_out, float* ms_out, void* stream,
                            const uint32_t* masks, const int32_t* mask_rows) {
  if (!logits || R < 1 || V < 1 || ld < V || !k || !temperature || !repeat_penalty || !context_offsets || !vals_out || !idx_out || !ms_out) {
    set_error("sample_rows: bad arguments (R >= 1, ld >= V >= 1, per-row k / temperature / repeat_penalty / context_offsets, outputs)");
    return AHA_ERR_INVALID;
  }
  for (int r = 0; r < R; ++r)
    if (!sample_shape_ok(V, k[r]) || !(repeat_penalty[r] > 0.f) || context_offsets[r + 1] < context_offsets[r] ||
        (context_offsets[r + 1] > context_offsets[r] && !context)) {
      set_error("sample_rows: row " + std::to_string(r) + " needs 1 <= k <= 64, repeat_penalty > 0 and ordered context offsets");
      return AHA_ERR_INVALID;
    }
  hipStream_t st = (hipStream_t)stream;
  // the row table and the deduplicated in-vocabulary context of model.hip's sampled step
  std::vector<int32_t> tab((size_t)R * SAMPLE_ROW_WORDS, 0);
  std::vector<uint32_t> ctx;
  for (int r = 0; r < R; ++r) {
    int32_t* t = tab.data() + (size_t)r * SAMPLE_ROW_WORDS;
    const size_t c0 = ctx.size();
    if (repeat_penalty[r] != 1.0f) {
      for (size_t i = context_offsets[r]; i < context_offsets[r + 1]; ++i)
        if (context[i] < (uint32_t)V) ctx.push_back(context[i]);
      std::sort(ctx.begin() + c0, ctx.end());
      ctx.erase(std::unique(ctx.begin() + c0, ctx.end()), ctx.end());
    }
    const float inv_t = temperature[r] > 0.f ? (float)(1.0 / (double)temperature[r]) : 1.0f;
    t[SAMPLE_ROW_LROW] = r;
    t[SAMPLE_ROW_K] = k[r];
    memcpy(&t[SAMPLE_ROW_INVT], &inv_t, 4);
    memcpy(&t[SAMPLE_ROW_PEN], &repeat_penalty[r], 4);
    t[SAMPLE_ROW_CTX0] = (int32_t)c0;
    t[SAMPLE_ROW_NCTX] = (int32_t)(ctx.size() - c0);
    t[SAMPLE_ROW_MASK] = mask_rows && mask_rows[r] >= 0 ? mask_rows[r] : -1;
    if (t[SAMPLE_ROW_MASK] >= 0 && (!masks || (int64_t)t[SAMPLE_ROW_MASK] * ((V + 31) / 32) > (int64_t)INT32_MAX)) {
      set_error("sample_rows_masked: row " + std::to_string(r) + " names a mask but masks is null, or the mask index is out of range");
      return AHA_ERR_INVALID;
    }
  }
  // every row's addends sorted by id; an id >= V or a duplicate is refused before anything touches the device
  std::vector<uint32_t> aid;
  std::vector<float> aval;
  for (int r = 0; adj_offsets && r < R; ++r) {
    const size_t a0 = adj_offsets[r], a1 = adj_offsets[r + 1];
    if (a1 < a0 || (a1 > a0 && (!adj_ids || !adj_vals)) || a1 - a0 > (size_t)V) {
      set_error("sample_rows_adjusted: row " + std::to_string(r) + " needs ordered adj_offsets, adj_ids / adj_vals and at most V entries");
      return AHA_ERR_INVALID;
    }
    std::vector<size_t> o(a1 - a0);
    std::iota(o.begin(), o.end(), a0);
    std::sort(o.begin(), o.end(), [&](size_t x, size_t y) { return adj_ids[x] < adj_ids[y]; });
    int32_t* t = tab.data() + (size_t)r * SAMPLE_ROW_WORDS;
    t[SAMPLE_ROW_ADJ0] = (int32_t)aid.size();
    t[SAMPLE_ROW_NADJ] = (int32_t)o.size();
    for (size_t i = 0; i < o.size(); ++i) {
      const uint32_t id = adj_ids[o[i]];
      const float a = adj_vals[o[i]];
      if (id >= (uint32_t)V || (i && id == aid.back()) || isnan(a) || a == INFINITY) {
        set_error("sample_rows_adjusted: row " + std::to_string(r) + " needs distinct ids < V and addends that are finite or -inf");
        return AHA_ERR_INVALID;
      }
      aid.push_back(id);
      aval.push_back(a);
    }
  }
  if (aid.size() > (size_t)INT32_MAX) {
    set_error("sample_rows_adjusted: too many addends");
    return AHA_ERR_INVALID;
  }
  const int nw = sample_stage1_waves(V);
  const size_t cand = (size_t)R * (nw + 16) * 64;
  DevFree adj_free;
  uint32_t* d_aid = nullptr;
  float* d_aval = nullptr;
  if (!aid.empty()) {
    AHA_HIP_CHECK(hipMalloc((void**)&d_aid, aid.size() * 4));
    adj_free.p[0] = d_aid;
    AHA_HIP_CHECK(hipMalloc((void**)&d_aval, aid.size() * 4));
    adj_free.p[1] = d_aval;
    AHA_HIP_CHECK(hipMemcpyAsync(d_aid, aid.data(), aid.size() * 4, hipMemcpyHostToDevice, st));
    AHA_HIP_CHECK(hipMemcpyAsync(d_aval, aval.data(), aid.size() * 4, hipMemcpyHostToDevice, st));
  }
  int32_t* d_tab = nullptr;
  uint32_t *d_ctx = nullptr, *d_cidx = nullptr;
  float *d_cval = nullptr, *d_part = nullptr, *d_out = nullptr;
  AHA_HIP_CHECK(hipMalloc((void**)&d_tab, tab.size() * 4));
  AHA_HIP_CHECK(hipMalloc((void**)&d_ctx, std::max<size_t>(ctx.size(), 1) * 4));
  AHA_HIP_CHECK(hipMalloc((void**)&d_cval, cand * 4));
  AHA_HIP_CHECK(hipMalloc((void**)&d_cidx, cand * 4));
  AHA_HIP_CHECK(hipMalloc((void**)&d_part, 2 * (size_t)R * nw * 4));
  AHA_HIP_CHECK(hipMalloc((void**)&d_out, (size_t)R * SAMPLE_OUT_WORDS * 4));
  AHA_HIP_CHECK(hipMemcpyAsync(d_tab, tab.data(), tab.size() * 4, hipMemcpyHostToDevice, st));
  if (!ctx.empty()) AHA_HIP_CHECK(hipMemcpyAsync(d_ctx, ctx.data(), ctx.size() * 4, hipMemcpyHostToDevice, st));
  for (int stage = 0; stage < 3; ++stage)
    launch_topk_rows(logits, ld, V, R, d_tab, d_ctx, d_cval, d_cidx, d_part, d_part + (size_t)R * nw, d_out, stage, st, d_aid, d_aval, masks);
  hipError_t err = hipGetLastError();
  // {vals[64], max, sumexp, idx[64]} per row -> the three outputs
  if (err == hipSuccess) err = hipMemcpy2DAsync(vals_out, 64 * 4, d_out, SAMPLE_OUT_WORDS * 4, 64 * 4, R, hipMemcpyDeviceToDevice, st);
  if (err == hipSuccess) err = hipMemcpy2DAsync(ms_out, 2 * 4, d_out + 64, SAMPLE_OUT_WORDS * 4, 2 * 4, R, hipMemcpyDeviceToDevice, st);
  if (err == hipSuccess) err = hipMemcpy2DAsync(idx_out, 64 * 4, d_out + 66, SAMPLE_OUT_WORDS * 4, 64 * 4, R, hipMemcpyDeviceToDevice, st);
  hipStreamSynchronize(st);
  hipFree(d_tab);
  hipFree(d_ctx);
  hipFree(d_cval);
  hipFree(d_cidx);
  hipFree(d_part);
  hipFree(d_out);
  AHA_HIP_CHECK(err);
  return AHA_OK;
}

int aha_hip_sample_rows(const float* logits, int64_t ld, int32_t R, int32_t V, const int32_t* k, const float* temperature,
                        const float* repeat_penalty, const uint32_t* context, const size_t* context_offsets, float* vals_out,
                        uint32_t* idx_out, float* ms_out, void* stream) {
  API_GUARD_BEGIN
  return sample_rows_impl(logits, ld, R, V, k, temperature, repeat_penalty, context, context_offsets, nullptr, nullptr, nullptr, vals_out, idx_out,
                          ms_out, stream, nullptr, nullptr);
  API_GUARD_END
}

int aha_hip_sample_rows_adjusted(const float* logits, int64_t ld, int32_t R, int32_t V, const int32_t* k, const float* temperature,
                                 const float* repeat_penalty, const uint32_t* context, const size_t* context_offsets,
                                 const uint32_t* adj_ids, const float* adj_vals, const size_t* adj_offsets, float* vals_out,
                                 uint32_t* idx_out, float* ms_out, void* stream) {
  API_GUARD_BEGIN
  if (!adj_offsets) {
    set_error("sample_rows_adjusted: null adj_offsets");
    return AHA_ERR_INVALID;
  }
  return sample_rows_impl(logits, ld, R, V, k, temperature, repeat_penalty, context, context_offsets, adj_ids, adj_vals, adj_offsets, vals_out,
                          idx_out, ms_out, stream, nullptr, nullptr);
  API_GUARD_END
}

int aha_hip_sample_rows_masked(const float* logits, int64_t ld, int32_t R, int32_t V, const int32_t* k, const float* temperature,
                               const float* repeat_penalty, const uint32_t* context, const size_t* context_offsets, const uint32_t* adj_ids,
                               const float* adj_vals, const size_t* adj_offsets, const uint32_t* masks, const int32_t* mask_rows,
                               float* vals_out, uint32_t* idx_out, float* ms_out, void* stream) {
  API_GUARD_BEGIN
  if (!mask_rows) {
    set_error("sample_rows_masked: null mask_rows");
    return AHA_ERR_INVALID;
  }
  return sample_rows_impl(logits, ld, R, V, k, temperature, repeat_penalty, context, context_offsets, adj_ids, adj_vals, adj_offsets, vals_out,
                          idx_out, ms_out, stream, masks, mask_rows);
  API_GUARD_END
}

int aha_hip_logprob_rows(const float* logits, int64_t ld, int32_t R, int32_t V, const uint32_t* tokens, const int32_t* n_top,
                         aha_token_logprobs* out, void* stream) {
  API_GUARD_BEGIN
  if (!logits || R < 1 || V < 1 || ld < V || !tokens || !n_top || !out) {
    set_error("logprob_rows: bad arguments (R >= 1, ld >= V >= 1, logits / tokens / n_top / out)");
    return AHA_ERR_INVALID;
  }
  for (int r = 0; r < R; ++r)
    if (n_top[r] < 0 || n_top[r] > AHA_MAX_TOP_LOGPROBS) {
      set_error("logprob_rows: row " + std::to_string(r) + " needs 0 <= n_top <= " + std::to_string(AHA_MAX_TOP_LOGPROBS));
      return AHA_ERR_INVALID;
    }
  if (!logprob_shape_ok(V)) {
    set_error("logprob_rows: vocabulary too large for the logprob pass");
    return AHA_ERR_UNSUPPORTED;
  }
  hipStream_t st = (hipStream_t)stream;
  std::vector<int32_t> tab((size_t)R * LOGPROB_ROW_WORDS, 0);
  for (int r = 0; r < R; ++r) {
    int32_t* t = tab.data() + (size_t)r * LOGPROB_ROW_WORDS;
    t[LOGPROB_ROW_LROW] = r;
    t[LOGPROB_ROW_NTOP] = n_top[r];
    t[LOGPROB_ROW_TOK] = r;
    t[LOGPROB_ROW_CSLOT] = -1;
  }
  const int nw = logprob_stage1_waves(V);
  const size_t cand = (size_t)R * nw * LOGPROB_MAX_TOP;
  int32_t* d_tab = nullptr;
  uint32_t* d_cidx = nullptr;
  float *d_cval = nullptr, *d_part = nullptr, *d_out = nullptr;
  AHA_HIP_CHECK(hipMalloc((void**)&d_tab, tab.size() * 4));
  AHA_HIP_CHECK(hipMalloc((void**)&d_cval, cand * 4));
  AHA_HIP_CHECK(hipMalloc((void**)&d_cidx, cand * 4));
  AHA_HIP_CHECK(hipMalloc((void**)&d_part, 2 * (size_t)R * nw * 4));
  AHA_HIP_CHECK(hipMalloc((void**)&d_out, (size_t)R * LOGPROB_OUT_WORDS * 4));
  AHA_HIP_CHECK(hipMemcpyAsync(d_tab, tab.data(), tab.size() * 4, hipMemcpyHostToDevice, st));
  for (int stage = 0; stage < 2; ++stage)
    launch_logprob_rows(logits, ld, V, R, d_tab, tokens, d_cval, d_cidx, d_part, d_part + (size_t)R * nw, nullptr, d_out, stage, st);
  hipError_t err = hipGetLastError();
  // the aha_token_logprobs at the head of every output row
  if (err == hipSuccess)
    err = hipMemcpy2DAsync(out, sizeof(aha_token_logprobs), d_out, LOGPROB_OUT_WORDS * 4, sizeof(aha_token_logprobs), R, hipMemcpyDeviceToDevice, st);
  hipStreamSynchronize(st);
  hipFree(d_tab);
  hipFree(d_cval);
  hipFree(d_cidx);
  hipFree(d_part);
  hipFree(d_out);
  AHA_HIP_CHECK(err);
  return AHA_OK;
  API_GUARD_END
}

static bool attn_batch_geometry_ok(int32_t nh, int32_t kvh) { return nh > 0 && kvh > 0 && nh % kvh == 0 && nh / kvh <= 16 && kvh <= 64; }

// The row table of an op-level decode attention call: splits from the row's own length, counters from zero, one counter block per row.
// -> the largest split count of a row.
static int attn_batch_row_table(const int32_t* page0, const int32_t* kv_len, int rows, int g, std::vector<int32_t>& tab) {
  int max_split = 1;
  tab.assign((size_t)rows * GEN_ROW_WORDS, 0);
  for (int r = 0; r < rows; ++r) {
    int32_t* t = tab.data() + (size_t)r * GEN_ROW_WORDS;
    t[GEN_ROW_PAGE0] = page0[r];
    t[GEN_ROW_KVLEN] = kv_len[r];
    t[GEN_ROW_NSPLIT] = attn_decode_nsplit(kv_len[r], g, 64);
    t[GEN_ROW_POS] = kv_len[r] - 1;
    t[GEN_ROW_CTRROW] = r;
    max_split = std::max(max_split, t[GEN_ROW_NSPLIT]);
  }
  return max_split;
}

int aha_hip_attn_decode_batch(const void* qkv, const void* q_norm_w, const void* k_norm_w, const float* rope, const uint64_t* page_ptrs,
                              const int32_t* page0, const int32_t* kv_len, int32_t rows, int32_t nh, int32_t kvh, float eps, float scale,
                              void* o, void* stream) {
  API_GUARD_BEGIN
  if (!qkv || !q_norm_w || !k_norm_w || !rope || !page_ptrs || !page0 || !kv_len || !o || rows < 1 || !attn_batch_geometry_ok(nh, kvh)) {
    set_error("attn_decode_batch: bad arguments (rows >= 1, nh % kvh == 0, group size <= 16)");
    return AHA_ERR_INVALID;
  }
  for (int r = 0; r < rows; ++r)
    if (kv_len[r] < 1 || page0[r] < 0) {
      set_error("attn_decode_batch: row " + std::to_string(r) + " needs kv_len >= 1 and page0 >= 0");
      return AHA_ERR_INVALID;
    }
  hipStream_t st = (hipStream_t)stream;
  std::vector<int32_t> tab;
  const int max_split = attn_batch_row_table(page0, kv_len, rows, nh / kvh, tab);
  int32_t* d_tab = nullptr;
  float *po = nullptr, *pml = nullptr;
  unsigned* ctr = nullptr;
  AHA_HIP_CHECK(hipMalloc((void**)&d_tab, tab.size() * 4));
  AHA_HIP_CHECK(hipMalloc((void**)&po, (size_t)rows * max_split * nh * 128 * 4));
  AHA_HIP_CHECK(hipMalloc((void**)&pml, (size_t)rows * max_split * nh * 2 * 4));
  AHA_HIP_CHECK(hipMalloc((void**)&ctr, (size_t)rows * kvh * 32 * 4));
  AHA_HIP_CHECK(hipMemsetAsync(ctr, 0, (size_t)rows * kvh * 32 * 4, st));
  AHA_HIP_CHECK(hipMemcpyAsync(d_tab, tab.data(), tab.size() * 4, hipMemcpyHostToDevice, st));
  AttnDecodeBatchArgs b{};
  b.qkv = qkv; b.q_norm_w = q_norm_w; b.k_norm_w = k_norm_w; b.rope = rope; b.page_ptrs = page_ptrs; b.layer_off = 0; b.row_tab = d_tab;
  b.part_o = po; b.part_ml = pml; b.o = o; b.head_ctr = ctr; b.ctr_step = 1; b.nh = nh; b.kvh = kvh; b.max_nsplit = max_split;
  b.eps = eps; b.scale = scale;
  launch_attn_decode_batch(b, rows, max_split, st);
  hipError_t err = hipGetLastError();
  hipStreamSynchronize(st);
  hipFree(d_tab);
  hipFree(po);
  hipFree(pml);
  hipFree(ctr);
  AHA_HIP_CHECK(err);
  return AHA_OK;
  API_GUARD_END
}

int aha_hip_debug_attn_decode_rows(const void* qkv, const void* q_norm_w, const void* k_norm_w, const float* rope, const uint64_t* page_ptrs,
                                   const int32_t* page0, const int32_t* kv_len, int32_t rows, int32_t nh, int32_t kvh, float eps, float scale,
                                   void* o, int32_t form, void* stream) {
  API_GUARD_BEGIN
  const char* who = "debug_attn_decode_rows: ";
  auto bad = [&](const std::string& why) {
    set_error(who + why);
    return AHA_ERR_INVALID;
  };
  if (form < 0 || form > 2) return bad("form must be 0 .. 2");
  if (!qkv || !q_norm_w || !k_norm_w || !rope || !page_ptrs || !page0 || !kv_len || (!o && form != 2)) return bad("null pointer");
  if (rows < 1 || rows > 65535 || !attn_batch_geometry_ok(nh, kvh)) return bad("bad arguments (rows 1 .. 65535, nh % kvh == 0, group size <= 16)");
  for (int r = 0; r < rows; ++r)
    if (kv_len[r] < 1 || page0[r] < 0) return bad("row " + std::to_string(r) + " needs kv_len >= 1 and page0 >= 0");
  hipStream_t st = (hipStream_t)stream;
  std::vector<int32_t> tab;
  const int max_split = attn_batch_row_table(page0, kv_len, rows, nh / kvh, tab);
  DevBuf d_tab, po, pml, ctr;
  if (int rc = d_tab.upload(tab.data(), tab.size() * 4)) return rc;
  AttnDecodeBatchArgs b{};
  b.qkv = qkv; b.q_norm_w = q_norm_w; b.k_norm_w = k_norm_w; b.rope = rope; b.page_ptrs = page_ptrs; b.layer_off = 0;
  b.row_tab = (const int32_t*)d_tab.p; b.o = o; b.ctr_step = 1; b.nh = nh; b.kvh = kvh; b.max_nsplit = max_split; b.eps = eps; b.scale = scale;
  if (form != 2) {
    AHA_HIP_CHECK(hipMalloc(&po.p, (size_t)rows * max_split * nh * 128 * 4));
    AHA_HIP_CHECK(hipMalloc(&pml.p, (size_t)rows * max_split * nh * 2 * 4));
    AHA_HIP_CHECK(hipMalloc(&ctr.p, (size_t)rows * kvh * 32 * 4));
    AHA_HIP_CHECK(hipMemsetAsync(ctr.p, 0, (size_t)rows * kvh * 32 * 4, st));
    b.part_o = (float*)po.p; b.part_ml = (float*)pml.p; b.head_ctr = (unsigned*)ctr.p;
  }
  if (form != 0) launch_kv_append_rows(b, rows, st);
  if (form != 2) launch_attn_decode_batch(b, rows, max_split, st, form == 0);
  hipError_t err = hipGetLastError();
  hipStreamSynchronize(st);
  AHA_HIP_CHECK(err);
  return AHA_OK;
  API_GUARD_END
}

int aha_hip_debug_spec_accept(const uint32_t* argmax, const int32_t* row_tok, int32_t rows, const int32_t* seq_tab, int32_t n_seqs,
                              int32_t layout, uint32_t* out, void* stream) {
  API_GUARD_BEGIN
  const char* who = "debug_spec_accept: ";
  auto bad = [&](const std::string& why) {
    set_error(who + why);
    return AHA_ERR_INVALID;
  };
  if (layout < 0 || layout > 1) return bad("layout must be 0 (consecutive rows) or 1 (own row and draft rows apart)");
  if (!argmax || !row_tok || !seq_tab || !out) return bad("null pointer");
  if (rows < 1 || rows > (1 << 24) || n_seqs < 1 || n_seqs > (1 << 24)) return bad("rows and n_seqs must be 1 .. 2^24");
  const int words = layout == 0 ? SPEC_SEQ_WORDS : ENG_SEQ_WORDS;
  for (int s = 0; s < n_seqs; ++s) {   // every row the kernel would read for sequence s lies inside the call's rows
    const int32_t* e = seq_tab + (size_t)s * words;
    const int64_t first = e[0], nd = layout == 0 ? e[SPEC_SEQ_NDRAFT] : e[ENG_SEQ_NDRAFT], k = std::min<int64_t>(nd, SPEC_MAX_DRAFT);
    const int64_t d0 = layout == 0 ? first + 1 : e[ENG_SEQ_DRAFT0];
    if (nd < 0) return bad("sequence " + std::to_string(s) + " has a negative draft count");
    if (first < 0 || first >= rows || (k > 0 && (d0 < 0 || d0 + k > rows)))
      return bad("sequence " + std::to_string(s) + " reaches rows outside 0 .. " + std::to_string(rows - 1));
  }
  hipStream_t st = (hipStream_t)stream;
  // the step's upload: the row table (the input token in GEN_ROW_TOK) with the sequence entries behind it
  std::vector<int32_t> tab((size_t)rows * GEN_ROW_WORDS + (size_t)n_seqs * words, 0);
  for (int r = 0; r < rows; ++r) tab[(size_t)r * GEN_ROW_WORDS + GEN_ROW_TOK] = row_tok[r];
  std::copy(seq_tab, seq_tab + (size_t)n_seqs * words, tab.begin() + (size_t)rows * GEN_ROW_WORDS);
  DevBuf d_tab;
  if (int rc = d_tab.upload(tab.data(), tab.size() * 4)) return rc;
  const int32_t* rt = (const int32_t*)d_tab.p;
  if (layout == 0) launch_spec_accept_rows(argmax, rt, rt + (size_t)rows * GEN_ROW_WORDS, n_seqs, out, st);
  else launch_spec_accept_split(argmax, rt, rt + (size_t)rows * GEN_ROW_WORDS, n_seqs, out, st);
  hipError_t err = hipGetLastError();
  hipStreamSynchronize(st);
  AHA_HIP_CHECK(err);
  return AHA_OK;
  API_GUARD_END
}

int aha_hip_debug_attn_decode_fused(const void* qkv, const void* q_norm_w, const void* k_norm_w, const float* rope, const uint64_t* page_ptrs,
                                    int32_t kv_len, int32_t nh, int32_t kvh, float eps, float scale, void* o, void* stream) {
  API_GUARD_BEGIN
  if (!qkv || !q_norm_w || !k_norm_w || !rope || !page_ptrs || !o || kv_len < 1 || !attn_batch_geometry_ok(nh, kvh)) {
    set_error("debug_attn_decode_fused: bad arguments (kv_len >= 1, nh % kvh == 0, group size <= 16)");
    return AHA_ERR_INVALID;
  }
  hipStream_t st = (hipStream_t)stream;
  const int nsplit = attn_decode_nsplit(kv_len, nh / kvh, 64);
  float *po = nullptr, *pml = nullptr;
  unsigned* ctr = nullptr;
  AHA_HIP_CHECK(hipMalloc((void**)&po, (size_t)nsplit * nh * 128 * 4));
  AHA_HIP_CHECK(hipMalloc((void**)&pml, (size_t)nsplit * nh * 2 * 4));
  AHA_HIP_CHECK(hipMalloc((void**)&ctr, (size_t)kvh * 32 * 4));
  AHA_HIP_CHECK(hipMemsetAsync(ctr, 0, (size_t)kvh * 32 * 4, st));
  AttnDecodeFusedArgs a{};
  a.qkv = qkv; a.q_norm_w = q_norm_w; a.k_norm_w = k_norm_w; a.rope = rope;
  a.kv.page_ptrs = page_ptrs; a.kv.layer_off = 0; a.kv.kvh = kvh; a.kv.d = 128;
  a.kv_start_v = kv_len - 1; a.kv_len_v = kv_len; a.part_o = po; a.part_ml = pml; a.o = o; a.head_ctr = ctr;
  a.ctr_target = nsplit > 1 ? (unsigned)nsplit : 0u; a.nh = nh; a.kvh = kvh; a.nsplit = nsplit; a.eps = eps; a.scale = scale;
  launch_attn_decode_fused(a, st);
  hipError_t err = hipGetLastError();
  hipStreamSynchronize(st);
  hipFree(po);
  hipFree(pml);
  hipFree(ctr);
  AHA_HIP_CHECK(err);
  return AHA_OK;
  API_GUARD_END
}

int aha_hip_attn_prefill(const void* q, const void* k, const void* v, void* o, int32_t S, int32_t L, int32_t nh,
                         int32_t kvh, int32_t d, int32_t kv_offset, int32_t causal, float scale, void* stream) {
  API_GUARD_BEGIN
  if ((d != 128 && d != 64) || L <= 0 || S <= 0 || nh % kvh || (d == 64 && nh != kvh)) {
    set_error("attn_prefill: head_dim must be 128, or 64 with nh == kvh (the audio encoder's geometry)");
    return AHA_ERR_UNSUPPORTED;
  }
  hipStream_t st = (hipStream_t)stream;
  TmpPages t;
  if (d == 128) {
    int rc = build_tmp_pages(t, k, v, L, kvh, d, st);
    if (rc) return rc;
  } else {   // head_dim 64: pages through the audio tower's own packer (K | V of a fused row)
    const int npages = (L + KV_PAGE_TOKENS - 1) / KV_PAGE_TOKENS;
    const size_t page_bytes = (size_t)2 * kvh * KV_PAGE_TOKENS * d * 2, row = (size_t)kvh * d * 2;
    AHA_HIP_CHECK(hipMalloc(&t.store, page_bytes * npages));
    AHA_HIP_CHECK(hipMemsetAsync(t.store, 0, page_bytes * npages, st));
    std::vector<uint64_t> ptrs(npages);
    for (int i = 0; i < npages; ++i) ptrs[i] = (uint64_t)(uintptr_t)t.store + (size_t)(npages - 1 - i) * page_bytes;
    AHA_HIP_CHECK(hipMalloc((void**)&t.d_ptrs, npages * 8));
    AHA_HIP_CHECK(hipMemcpy(t.d_ptrs, ptrs.data(), npages * 8, hipMemcpyHostToDevice));
    t.kv.page_ptrs = t.d_ptrs; t.kv.layer_off = 0; t.kv.kvh = kvh; t.kv.d = d;
    AHA_HIP_CHECK(hipMalloc(&t.fused, row * 2 * L));
    AHA_HIP_CHECK(hipMemcpy2DAsync(t.fused, row * 2, k, row, row, L, hipMemcpyDeviceToDevice, st));
    AHA_HIP_CHECK(hipMemcpy2DAsync((char*)t.fused + row, row * 2, v, row, row, L, hipMemcpyDeviceToDevice, st));
    launch_kv_pack_generic(t.fused, (int64_t)2 * kvh * d, 0, kvh * d, t.kv, L, kvh, d, st);
    AHA_HIP_CHECK(hipGetLastError());
  }
  AttnPrefillArgs a{};
  a.q = q; a.kv = t.kv; a.o = o; a.S = S; a.nh = nh; a.kvh = kvh; a.d = d; a.kv_offset = kv_offset; a.kv_total = L;
  a.causal = causal; a.scale = scale;
  launch_attn_prefill(a, st);
  if (const char* reps_env = getenv("AHA_ATTN_TIME")) {  // microbenchmark hook (scripts/bench_attn.py): kernel-only time
    const int reps = atoi(reps_env) > 0 ? atoi(reps_env) : 5;
    hipEvent_t e0, e1;
    hipEventCreate(&e0); hipEventCreate(&e1);
    hipEventRecord(e0, st);
    for (int i = 0; i < reps; ++i) launch_attn_prefill(a, st);
    hipEventRecord(e1, st);
    hipEventSynchronize(e1);
    float ms = 0.f;
    hipEventElapsedTime(&ms, e0, e1);
    fprintf(stderr, "[attn_prefill] S=%d L=%d nh=%d causal=%d: %.3f ms/launch\n", S, L, nh, causal, ms / reps);
    hipEventDestroy(e0); hipEventDestroy(e1);
  }
  hipError_t e = hipGetLastError();
  hipStreamSynchronize(st);   // (t's destructor frees the pages and the fused rows: after the stream has drained)
  AHA_HIP_CHECK(e);
  return AHA_OK;
  API_GUARD_END
}

int aha_hip_image_to_patches(const uint8_t* img_hwc, void* out, int32_t H, int32_t W, int32_t patch, int32_t merge,
                             const float mean[3], const float std[3], void* stream) {
  if (!img_hwc || !out || !mean || !std || patch <= 0 || merge <= 0 || H % (patch * merge) || W % (patch * merge)) {
    set_error("image_to_patches: H and W must be multiples of patch*merge");
    return AHA_ERR_INVALID;
  }
  launch_image_to_patches(img_hwc, out, H, W, patch, merge, mean, std, (hipStream_t)stream);
  AHA_HIP_CHECK(hipGetLastError());
  return AHA_OK;
}

int aha_hip_video_to_patches(const uint8_t* frames_thwc, void* out, int32_t T, int32_t H, int32_t W, int32_t patch, int32_t merge,
                             const float mean[3], const float std[3], void* stream) {
  if (!frames_thwc || !out || !mean || !std || T <= 0 || patch <= 0 || merge <= 0 || H % (patch * merge) || W % (patch * merge)) {
    set_error("video_to_patches: T > 0 frames, H and W multiples of patch*merge");
    return AHA_ERR_INVALID;
  }
  launch_video_to_patches(frames_thwc, out, T, H, W, patch, merge, mean, std, (hipStream_t)stream);
  AHA_HIP_CHECK(hipGetLastError());
  return AHA_OK;
}

int aha_hip_img_smart_resize(uint32_t h, uint32_t w, uint32_t factor, uint32_t min_pixels, uint32_t max_pixels, uint32_t* h_out,
                             uint32_t* w_out) {
  API_GUARD_BEGIN
  if (!h_out || !w_out) {
    set_error("null argument");
    return AHA_ERR_INVALID;
  }
  return img_smart_resize(h, w, factor, min_pixels, max_pixels, h_out, w_out);
  API_GUARD_END
}

int aha_hip_video_smart_resize(uint32_t num_frames, uint32_t h, uint32_t w, uint32_t temporal_factor, uint32_t factor, uint32_t min_pixels,
                               uint32_t max_pixels, uint32_t video_ratio, uint32_t* h_out, uint32_t* w_out) {
  API_GUARD_BEGIN
  if (!h_out || !w_out) {
    set_error("null argument");
    return AHA_ERR_INVALID;
  }
  return video_smart_resize(num_frames, h, w, temporal_factor, factor, min_pixels, max_pixels, video_ratio, h_out, w_out);
  API_GUARD_END
}
int aha_hip_video_sample_frames(uint32_t total_frames, float rate, uint32_t fps, uint32_t min_frames, uint32_t max_frames,
                                uint32_t* nframes_out, uint32_t* interval_out) {
  API_GUARD_BEGIN
  if (!nframes_out || !interval_out) {
    set_error("null argument");
    return AHA_ERR_INVALID;
  }
  return video_sample_frames(total_frames, rate, fps, min_frames, max_frames, nframes_out, interval_out);
  API_GUARD_END
}
int64_t aha_hip_video_timestamps(const uint32_t* frame_indices, size_t n, float fps, uint32_t t_merge_size, float* out, size_t cap) {
  API_GUARD_BEGIN
  return video_timestamps(frame_indices, n, fps, t_merge_size, out, cap);
  API_GUARD_END
}

int aha_hip_image_resize(const uint8_t* src_hwc, int32_t H, int32_t W, uint8_t* dst_hwc, int32_t new_h, int32_t new_w, void* stream) {
  API_GUARD_BEGIN
  if (!src_hwc || !dst_hwc || H <= 0 || W <= 0 || new_h <= 0 || new_w <= 0) {
    set_error("image_resize: bad arguments");
    return AHA_ERR_INVALID;
  }
  return image_resize(src_hwc, H, W, dst_hwc, new_h, new_w, (hipStream_t)stream);
  API_GUARD_END
}

int aha_hip_debug_resize_taps(int32_t n_in, int32_t n_out, int32_t* left, int32_t* count, float* weights, int64_t weights_cap) {
  API_GUARD_BEGIN
  if (n_in <= 0 || n_out <= 0 || !left || !count || !weights) {
    set_error("debug_resize_taps: bad arguments");
    return AHA_ERR_INVALID;
  }
  return debug_resize_taps(n_in, n_out, left, count, weights, weights_cap);
  API_GUARD_END
}

int64_t aha_hip_debug_resample_taps(int32_t orig, int32_t new_f, float* taps, int64_t cap, int32_t* width, int32_t* klen) {
  API_GUARD_BEGIN
  if (orig <= 0 || new_f <= 0 || !taps || !width || !klen) {
    set_error("debug_resample_taps: bad arguments");
    return AHA_ERR_INVALID;
  }
  return debug_resample_taps(orig, new_f, taps, cap, width, klen);
  API_GUARD_END
}

int aha_hip_get_rope_index_mm(const aha_model_desc* desc, const uint32_t* input_ids, size_t n_ids, const uint32_t* image_grid_thw,
                              int32_t n_images, const uint32_t* video_grid_thw, int32_t n_videos, int32_t* pos_out,
                              int64_t* rope_delta_out) {
  API_GUARD_BEGIN
  if (!desc || !input_ids || !pos_out || !rope_delta_out || (n_images > 0 && !image_grid_thw) || (n_videos > 0 && !video_grid_thw)) {
    set_error("aha_hip_get_rope_index: null argument");
    return AHA_ERR_INVALID;
  }
  if (n_images <= 0 && n_videos <= 0) {
    for (int a = 0; a < 3; ++a)
      for (size_t i = 0; i < n_ids; ++i) pos_out[a * n_ids + i] = (int32_t)i;
    *rope_delta_out = 0;
    return AHA_OK;
  }
  return rope_index_core(*desc, input_ids, n_ids, image_grid_thw, n_images, video_grid_thw, n_videos, pos_out, rope_delta_out);
  API_GUARD_END
}
int aha_hip_get_rope_index(const aha_model_desc* desc, const uint32_t* input_ids, size_t n_ids, const uint32_t* image_grid_thw,
                           int32_t n_images, int32_t* pos_out, int64_t* rope_delta_out) {
  return aha_hip_get_rope_index_mm(desc, input_ids, n_ids, image_grid_thw, n_images, nullptr, 0, pos_out, rope_delta_out);
}
int aha_hip_embed(aha_model* m, const uint32_t* input_ids, size_t n_ids, float* out) {
  API_GUARD_BEGIN
  if (!m) {
    set_error("null model");
    return AHA_ERR_INVALID;
  }
  if (int rc = engine_owns_cache(m, "embed")) return rc;
  return model_embed(m, input_ids, n_ids, out);
  API_GUARD_END
}
int aha_hip_embed_batch(aha_model* m, const uint32_t* input_ids, const size_t* seq_lens, size_t n_seqs, size_t max_tokens_per_pass,
                        float* out) {
  API_GUARD_BEGIN
  if (!m) {
    set_error("null model");
    return AHA_ERR_INVALID;
  }
  if (int rc = engine_owns_cache(m, "embed_batch")) return rc;
  return model_embed_batch(m, input_ids, seq_lens, n_seqs, max_tokens_per_pass, out);
  API_GUARD_END
}
// The device-free checks of the aha_hip_generate_batch* entries, in their fixed order: the sampling parameters, the top_logprobs /
// logprobs_out pairing and range, then the model handle and the engine's claim on the cache.  who: the entry's name, which prefixes its
// messages.  A new per-request option's argument check goes here.
enum LogprobRule { LP_ABSENT, LP_BOTH, LP_BOTH_OR_NEITHER };
static int gen_options_check(const char* who, const aha_model* m, size_t n_seqs, const GenOptions& o, bool params_required, LogprobRule lp) {
  auto refuse = [who](const std::string& why) {   // (nothing is built for a call that passes)
    set_error(std::string(who) + ": " + why);
    return AHA_ERR_INVALID;
  };
  const size_t n = std::min(n_seqs, (size_t)1 << 20);
  // the parameters first: they are checked before anything touches the model or the device
  if (params_required && n_seqs && !o.params) return refuse("null params");
  for (size_t j = 0; o.params && j < n; ++j) {   // params == NULL: every sequence greedy
    std::string why;
    if (sampling_params_check(o.params[j], &why)) return refuse("params of sequence " + std::to_string(j) + ": " + why);
  }
  if (lp == LP_BOTH && (!o.top_logprobs || !o.logprobs_out)) return refuse("null top_logprobs / logprobs_out");
  if (lp == LP_BOTH_OR_NEITHER && (o.top_logprobs == nullptr) != (o.logprobs_out == nullptr))
    return refuse("top_logprobs and logprobs_out go together (both NULL: no logprobs)");
  for (size_t j = 0; o.top_logprobs && j < n; ++j)
    if (o.top_logprobs[j] < -1 || o.top_logprobs[j] > AHA_MAX_TOP_LOGPROBS)
      return refuse("top_logprobs of sequence " + std::to_string(j) + " must be -1 (none) or 0 .. " + std::to_string(AHA_MAX_TOP_LOGPROBS) +
                    ", got " + std::to_string(o.top_logprobs[j]));
  if (!m) {
    set_error("null model");
    return AHA_ERR_INVALID;
  }
  return engine_owns_cache(m, who);
}

int aha_hip_generate_batch(aha_model* m, const uint32_t* input_ids, const size_t* seq_lens, size_t n_seqs, size_t max_new,
                           size_t max_tokens_per_pass, uint32_t* tokens_out, size_t* n_out, float* logits_out) {
  API_GUARD_BEGIN
  GenOptions o;
  o.logits_out = logits_out;
  if (int rc = gen_options_check("generate_batch", m, n_seqs, o, false, LP_ABSENT)) return rc;
  return model_generate_batch(m, input_ids, seq_lens, n_seqs, max_new, max_tokens_per_pass, o, tokens_out, n_out);
  API_GUARD_END
}
int aha_hip_generate_batch_sampled(aha_model* m, const uint32_t* input_ids, const size_t* seq_lens, size_t n_seqs,
                                   const aha_sampling_params* params, size_t max_new, size_t max_tokens_per_pass,
                                   uint32_t* tokens_out, size_t* n_out, float* step_logits_out) {
  API_GUARD_BEGIN
  GenOptions o;
  o.params = params, o.step_logits_out = step_logits_out;
  if (int rc = gen_options_check("generate_batch_sampled", m, n_seqs, o, true, LP_ABSENT)) return rc;
  return model_generate_batch(m, input_ids, seq_lens, n_seqs, max_new, max_tokens_per_pass, o, tokens_out, n_out);
  API_GUARD_END
}
int aha_hip_generate_batch_mm(aha_model* m, const uint32_t* input_ids, const size_t* seq_lens, size_t n_seqs, const aha_mm_input* const* mm,
                              const aha_sampling_params* params, size_t max_new, size_t max_tokens_per_pass, uint32_t* tokens_out,
                              size_t* n_out, float* step_logits_out) {
  API_GUARD_BEGIN
  GenOptions o;
  o.mm = mm, o.params = params, o.step_logits_out = step_logits_out;
  if (int rc = gen_options_check("generate_batch_mm", m, n_seqs, o, false, LP_ABSENT)) return rc;
  return model_generate_batch(m, input_ids, seq_lens, n_seqs, max_new, max_tokens_per_pass, o, tokens_out, n_out);
  API_GUARD_END
}
int aha_hip_generate_batch_logprobs(aha_model* m, const uint32_t* input_ids, const size_t* seq_lens, size_t n_seqs,
                                    const aha_mm_input* const* mm, const aha_sampling_params* params, const int32_t* top_logprobs,
                                    size_t max_new, size_t max_tokens_per_pass, uint32_t* tokens_out, size_t* n_out,
                                    float* step_logits_out, aha_token_logprobs* logprobs_out) {
  API_GUARD_BEGIN
  GenOptions o;
  o.mm = mm, o.params = params, o.step_logits_out = step_logits_out;
  o.top_logprobs = top_logprobs, o.logprobs_out = logprobs_out;
  if (int rc = gen_options_check("generate_batch_logprobs", m, n_seqs, o, false, LP_BOTH)) return rc;
  return model_generate_batch(m, input_ids, seq_lens, n_seqs, max_new, max_tokens_per_pass, o, tokens_out, n_out);
  API_GUARD_END
}
// aha_hip_generate_batch_adjusted, and aha_hip_generate_batch_masked (mask_fn set; without one it is exactly _adjusted, name included)
static int generate_batch_adjusted(aha_model* m, const uint32_t* input_ids, const size_t* seq_lens, size_t n_seqs,
                                   const aha_mm_input* const* mm, const aha_sampling_params* params, const aha_logit_adjust* adjust,
                                   const int32_t* top_logprobs, size_t max_new, size_t max_tokens_per_pass, aha_token_mask_fn mask_fn,
                                   void* mask_user, uint32_t* tokens_out, size_t* n_out, float* step_logits_out,
                                   aha_token_logprobs* logprobs_out) {
  API_GUARD_BEGIN
  GenOptions o;
  o.mm = mm, o.params = params, o.adjust = adjust, o.step_logits_out = step_logits_out;
  o.top_logprobs = top_logprobs, o.logprobs_out = logprobs_out;
  o.mask_fn = mask_fn, o.mask_user = mask_fn ? mask_user : nullptr;
  if (int rc = gen_options_check(mask_fn ? "generate_batch_masked" : "generate_batch_adjusted", m, n_seqs, o, false, LP_BOTH_OR_NEITHER)) return rc;
  return model_generate_batch(m, input_ids, seq_lens, n_seqs, max_new, max_tokens_per_pass, o, tokens_out, n_out);
  API_GUARD_END
}
int aha_hip_generate_batch_adjusted(aha_model* m, const uint32_t* input_ids, const size_t* seq_lens, size_t n_seqs,
                                    const aha_mm_input* const* mm, const aha_sampling_params* params, const aha_logit_adjust* adjust,
                                    const int32_t* top_logprobs, size_t max_new, size_t max_tokens_per_pass, uint32_t* tokens_out,
                                    size_t* n_out, float* step_logits_out, aha_token_logprobs* logprobs_out) {
  return generate_batch_adjusted(m, input_ids, seq_lens, n_seqs, mm, params, adjust, top_logprobs, max_new, max_tokens_per_pass, nullptr, nullptr,
                                 tokens_out, n_out, step_logits_out, logprobs_out);
}
int aha_hip_generate_batch_masked(aha_model* m, const uint32_t* input_ids, const size_t* seq_lens, size_t n_seqs,
                                  const aha_mm_input* const* mm, const aha_sampling_params* params, const aha_logit_adjust* adjust,
                                  const int32_t* top_logprobs, size_t max_new, size_t max_tokens_per_pass, aha_token_mask_fn mask_fn,
                                  void* mask_user, uint32_t* tokens_out, size_t* n_out, float* step_logits_out,
                                  aha_token_logprobs* logprobs_out) {
  return generate_batch_adjusted(m, input_ids, seq_lens, n_seqs, mm, params, adjust, top_logprobs, max_new, max_tokens_per_pass, mask_fn, mask_user,
                                 tokens_out, n_out, step_logits_out, logprobs_out);
}
int aha_hip_generate_batch_spec(aha_model* m, const uint32_t* input_ids, const size_t* seq_lens, size_t n_seqs, size_t max_new,
                                size_t max_tokens_per_pass, const aha_spec_config* spec, const uint32_t* predictions,
                                const size_t* prediction_lens, uint32_t* tokens_out, size_t* n_out, float* logits_out, size_t* n_proposed,
                                size_t* n_accepted, aha_spec_stats* stats) {
  API_GUARD_BEGIN
  if (int rc = spec_config_check(spec, "generate_batch_spec")) return rc;   // the config first, before anything touches the model
  if ((predictions == nullptr) != (prediction_lens == nullptr)) {
    set_error("generate_batch_spec: predictions and prediction_lens must both be set or both be null");
    return AHA_ERR_INVALID;
  }
  GenOptions o;
  o.logits_out = logits_out;
  o.spec = spec, o.predictions = predictions, o.prediction_lens = prediction_lens;
  o.n_proposed = n_proposed, o.n_accepted = n_accepted, o.stats = stats;
  if (int rc = gen_options_check("generate_batch_spec", m, n_seqs, o, false, LP_ABSENT)) return rc;
  return model_generate_batch(m, input_ids, seq_lens, n_seqs, max_new, max_tokens_per_pass, o, tokens_out, n_out);
  API_GUARD_END
}
int aha_hip_spec_propose(const aha_spec_config* spec, const uint32_t* context, size_t n_context, size_t n_prompt, const uint32_t* prediction,
                         size_t n_prediction, uint32_t* draft_out, size_t* n_draft) {
  API_GUARD_BEGIN
  if (int rc = spec_config_check(spec, "spec_propose")) return rc;
  if (!context || !draft_out || !n_draft || n_context == 0 || n_prompt > n_context) {
    set_error("spec_propose: null context / draft_out / n_draft, an empty context or n_prompt > n_context");
    return AHA_ERR_INVALID;
  }
  spec_propose(*spec, context, n_context, n_prompt, prediction, prediction ? n_prediction : 0, draft_out, n_draft);
  return AHA_OK;
  API_GUARD_END
}
int aha_hip_engine_create(aha_model* m, const aha_engine_config* cfg, aha_engine** out) {
  API_GUARD_BEGIN
  if (int rc = engine_config_check(cfg, nullptr, nullptr)) return rc;   // the config first: checked before the model is touched
  if (!m || !out) {
    set_error("engine_create: null model / out");
    return AHA_ERR_INVALID;
  }
  return engine_create(m, cfg, out);
  API_GUARD_END
}
void aha_hip_engine_destroy(aha_engine* e) {
  try {
    engine_destroy(e);
  } catch (...) {
  }
}
// The device-free checks of the aha_hip_engine_submit* entries: the parameters, top_logprobs (min_top: -1 where "no logprobs" is a
// legal value, 0 for _logprobs), then the handle.  who: the entry's name.
static int submit_options_check(const char* who, const aha_engine* e, const SubmitOptions& o, int32_t min_top) {
  auto refuse = [who](const std::string& why) {
    set_error(std::string(who) + ": " + why);
    return AHA_ERR_INVALID;
  };
  if (o.params) {   // the parameters first, as generate_batch_sampled checks them
    std::string why;
    if (sampling_params_check(*o.params, &why)) return refuse("params: " + why);
  }
  if (o.top_logprobs < min_top || o.top_logprobs > AHA_MAX_TOP_LOGPROBS)
    return refuse(std::string("top_logprobs must be ") + (min_top < 0 ? "-1 (none) or " : "") + "0 .. " + std::to_string(AHA_MAX_TOP_LOGPROBS) +
                  ", got " + std::to_string(o.top_logprobs));
  if (!e) return refuse("null engine");
  return AHA_OK;
}

int aha_hip_engine_submit(aha_engine* e, const uint32_t* input_ids, size_t n_ids, const aha_mm_input* mm, const aha_sampling_params* params,
                          size_t max_new, uint64_t* req_id) {
  API_GUARD_BEGIN
  SubmitOptions o;
  o.mm = mm, o.params = params;
  if (int rc = submit_options_check("engine_submit", e, o, -1)) return rc;
  return engine_submit(e, input_ids, n_ids, o, max_new, req_id);
  API_GUARD_END
}
int aha_hip_engine_submit_logprobs(aha_engine* e, const uint32_t* input_ids, size_t n_ids, const aha_mm_input* mm,
                                   const aha_sampling_params* params, size_t max_new, int32_t top_logprobs, uint64_t* req_id) {
  API_GUARD_BEGIN
  SubmitOptions o;
  o.mm = mm, o.params = params, o.top_logprobs = top_logprobs;
  if (int rc = submit_options_check("engine_submit_logprobs", e, o, 0)) return rc;
  return engine_submit(e, input_ids, n_ids, o, max_new, req_id);
  API_GUARD_END
}
int aha_hip_engine_submit_adjusted(aha_engine* e, const uint32_t* input_ids, size_t n_ids, const aha_mm_input* mm,
                                   const aha_sampling_params* params, const aha_logit_adjust* adjust, size_t max_new, int32_t top_logprobs,
                                   uint64_t* req_id) {
  API_GUARD_BEGIN
  SubmitOptions o;
  o.mm = mm, o.params = params, o.adjust = adjust, o.top_logprobs = top_logprobs;
  if (int rc = submit_options_check("engine_submit_adjusted", e, o, -1)) return rc;
  return engine_submit(e, input_ids, n_ids, o, max_new, req_id);
  API_GUARD_END
}
int aha_hip_engine_submit_masked(aha_engine* e, const uint32_t* input_ids, size_t n_ids, const aha_mm_input* mm,
                                 const aha_sampling_params* params, const aha_logit_adjust* adjust, const uint32_t* mask_words,
                                 size_t n_mask_words, size_t max_new, int32_t top_logprobs, uint64_t* req_id) {
  API_GUARD_BEGIN
  SubmitOptions o;
  o.mm = mm, o.params = params, o.adjust = adjust, o.top_logprobs = top_logprobs;
  o.mask = mask_words, o.n_mask_words = n_mask_words;
  if (int rc = submit_options_check("engine_submit_masked", e, o, -1)) return rc;
  return engine_submit(e, input_ids, n_ids, o, max_new, req_id);
  API_GUARD_END
}
int aha_hip_engine_submit_spec(aha_engine* e, const uint32_t* input_ids, size_t n_ids, const aha_mm_input* mm, size_t max_new,
                               const aha_spec_config* spec, const uint32_t* prediction, size_t n_prediction, uint64_t* req_id) {
  API_GUARD_BEGIN
  if (int rc = spec_config_check(spec, "engine_submit_spec")) return rc;   // the config first, as aha_hip_generate_batch_spec checks it
  SubmitOptions o;
  o.mm = mm, o.spec = spec;
  o.prediction = n_prediction ? prediction : nullptr, o.n_prediction = prediction ? n_prediction : 0;
  if (int rc = submit_options_check("engine_submit_spec", e, o, -1)) return rc;
  return engine_submit(e, input_ids, n_ids, o, max_new, req_id);
  API_GUARD_END
}
int aha_hip_engine_set_mask(aha_engine* e, uint64_t req_id, const uint32_t* words, size_t n_words) {
  API_GUARD_BEGIN
  if (!e) {
    set_error("engine_set_mask: null engine");
    return AHA_ERR_INVALID;
  }
  return engine_set_mask(e, req_id, words, n_words);
  API_GUARD_END
}
int aha_hip_engine_cancel(aha_engine* e, uint64_t req_id) {
  API_GUARD_BEGIN
  if (!e) {
    set_error("engine_cancel: null engine");
    return AHA_ERR_INVALID;
  }
  return engine_cancel(e, req_id);
  API_GUARD_END
}
int aha_hip_engine_step(aha_engine* e, aha_engine_event* ev, size_t cap, size_t* n_ev, float* logits_out) {
  API_GUARD_BEGIN
  if (!e) {
    set_error("engine_step: null engine");
    return AHA_ERR_INVALID;
  }
  return engine_step(e, ev, cap, n_ev, logits_out);
  API_GUARD_END
}
int aha_hip_engine_step_logprobs(aha_engine* e, aha_engine_event* ev, size_t cap, size_t* n_ev, float* logits_out,
                                 aha_token_logprobs* logprobs_out) {
  API_GUARD_BEGIN
  if (!e) {
    set_error("engine_step: null engine");
    return AHA_ERR_INVALID;
  }
  return engine_step(e, ev, cap, n_ev, logits_out, logprobs_out);
  API_GUARD_END
}
int aha_hip_engine_stats(const aha_engine* e, aha_engine_stats* out) {
  API_GUARD_BEGIN
  if (!e || !out) {
    set_error("engine_stats: null engine / out");
    return AHA_ERR_INVALID;
  }
  return engine_stats(e, out);
  API_GUARD_END
}
size_t aha_hip_engine_max_events(const aha_engine* e) {
  return e ? engine_max_events(e) : 0;
}
int aha_hip_engine_spec_stats(const aha_engine* e, aha_spec_stats* out) {
  API_GUARD_BEGIN
  if (!e || !out) {
    set_error("engine_spec_stats: null engine / out");
    return AHA_ERR_INVALID;
  }
  return engine_spec_stats(e, out);
  API_GUARD_END
}
int aha_hip_engine_request_spec(const aha_engine* e, uint64_t req_id, size_t* n_proposed, size_t* n_accepted) {
  API_GUARD_BEGIN
  if (!e || !n_proposed || !n_accepted) {
    set_error("engine_request_spec: null engine / n_proposed / n_accepted");
    return AHA_ERR_INVALID;
  }
  return engine_request_spec(e, req_id, n_proposed, n_accepted);
  API_GUARD_END
}
int aha_hip_engine_debug_ctr_base(aha_engine* e, uint32_t base) {
  if (!e) {
    set_error("engine_debug_ctr_base: null engine");
    return AHA_ERR_INVALID;
  }
  return engine_debug_ctr_base(e, base);
}
int aha_hip_config_parse(const char* model_dir, aha_model_desc* out) {
  API_GUARD_BEGIN
  if (!model_dir || !out) {
    set_error("aha_hip_config_parse: null argument");
    return AHA_ERR_INVALID;
  }
  return config_parse(model_dir, out);
  API_GUARD_END
}
int aha_hip_config_torch_dtype(const char* model_dir, char* out, size_t cap) {
  API_GUARD_BEGIN
  if (!model_dir || !out || cap == 0) {
    set_error("aha_hip_config_torch_dtype: null argument");
    return AHA_ERR_INVALID;
  }
  std::string s;
  const int rc = config_torch_dtype(model_dir, &s);
  if (rc) return rc;
  if (s.size() + 1 > cap) {
    set_error("aha_hip_config_torch_dtype: the buffer is too small");
    return AHA_ERR_INVALID;
  }
  memcpy(out, s.c_str(), s.size() + 1);
  return AHA_OK;
  API_GUARD_END
}
int aha_hip_weights_open(const char* model_dir, aha_weights** out) {
  API_GUARD_BEGIN
  if (!model_dir || !out) {
    set_error("aha_hip_weights_open: null argument");
    return AHA_ERR_INVALID;
  }
  return weights_open(model_dir, out);
  API_GUARD_END
}
size_t aha_hip_weights_count(const aha_weights* w) { return w ? w->views.size() : 0; }
int aha_hip_weights_get(const aha_weights* w, size_t index, aha_tensor_view* out) {
  if (!w || !out || index >= w->views.size()) {
    set_error("aha_hip_weights_get: bad handle or index");
    return AHA_ERR_INVALID;
  }
  *out = w->views[index];
  return AHA_OK;
}
void aha_hip_weights_close(aha_weights* w) { delete w; }
int aha_hip_model_load(aha_ctx* ctx, const char* model_dir, size_t kv_reserve_tokens, aha_model** out) {
  API_GUARD_BEGIN
  if (!ctx || !model_dir || !out) {
    set_error("aha_hip_model_load: null argument");
    return AHA_ERR_INVALID;
  }
  return model_load(ctx, model_dir, kv_reserve_tokens, out);
  API_GUARD_END
}

int aha_hip_set_allreduce(aha_model* m, aha_allreduce_fn fn, void* user) {
  if (!m) {
    set_error("null model");
    return AHA_ERR_INVALID;
  }
  m->allreduce_cb = fn;
  m->allreduce_user = user;
  return AHA_OK;
}
int aha_hip_set_seq_parallel(aha_model* m, aha_reduce_scatter_fn reduce_scatter, aha_all_gather_fn all_gather, void* user) {
  if (!m) {
    set_error("set_seq_parallel: null model");
    return AHA_ERR_INVALID;
  }
  if ((reduce_scatter == nullptr) != (all_gather == nullptr)) {
    set_error("set_seq_parallel: install both callbacks or neither");
    return AHA_ERR_INVALID;
  }
  m->reduce_scatter_cb = reduce_scatter;
  m->all_gather_cb = all_gather;
  m->sp_user = user;
  return AHA_OK;
}
int aha_hip_tp_unique_id(void* out128) {
  API_GUARD_BEGIN
  if (!out128) return AHA_ERR_INVALID;
  return tp_unique_id(out128);
  API_GUARD_END
}
int aha_hip_tp_init_rccl(aha_model* m, const void* unique_id128) {
  API_GUARD_BEGIN
  if (!m || !unique_id128) return AHA_ERR_INVALID;
  return tp_init_rccl(m, unique_id128);
  API_GUARD_END
}

int aha_hip_set_context_parallel(aha_model* m, int32_t rank, int32_t world, aha_all_gather_fn all_gather, void* user) {
  if (!m || world < 1 || world > 8 || rank < 0 || rank >= world) {
    set_error("set_context_parallel: rank in [0, world), world in 1..8");
    return AHA_ERR_INVALID;
  }
  if (m->tp_size > 1 && world > 1) {
    set_error("set_context_parallel: the model is tensor-parallel (sharded weights); context parallelism needs the full weights on every rank");
    return AHA_ERR_UNSUPPORTED;
  }
  if (m->desc.head_dim != 128 && world > 1) {
    set_error("set_context_parallel: head_dim 128 only");
    return AHA_ERR_UNSUPPORTED;
  }
  if (m->rccl_comm && (world != m->cp_size || rank != m->cp_rank)) {
    set_error("set_context_parallel: the RCCL communicator of this model was created for another (rank, world)");
    return AHA_ERR_STATE;
  }
  if (world != m->cp_size) m->pf_cap = 0;   // the prefill scratch carries the exchange's staging buffer: re-plan it on the next prefill
  m->cp_rank = rank;
  m->cp_size = world;
  m->cp_all_gather_cb = all_gather;
  m->cp_user = user;
  return AHA_OK;
}
int aha_hip_debug_cp_plan(int32_t n_tokens, int32_t world, int32_t rank, int32_t* out5) {
  if (!out5 || n_tokens <= 0) {
    set_error("debug_cp_plan: bad argument");
    return AHA_ERR_INVALID;
  }
  int o[5];
  if (debug_cp_plan(n_tokens, world, rank, o) != 0) return 1;   // not sharded (too few pages, world out of range)
  for (int i = 0; i < 5; ++i) out5[i] = o[i];
  return AHA_OK;
}
int aha_hip_cp_init_rccl(aha_model* m, const void* unique_id128) {
  API_GUARD_BEGIN
  if (!m || !unique_id128) return AHA_ERR_INVALID;
  return cp_init_rccl(m, unique_id128);
  API_GUARD_END
}

int aha_hip_debug_allreduce(aha_model* m, void* buf, size_t count) {
  API_GUARD_BEGIN
  if (!m || !buf) return AHA_ERR_INVALID;
  int rc;
  if (m->rccl_comm) {
    rc = rccl_allreduce(m, (float*)buf, count);
  } else if (m->allreduce_cb) {
    rc = m->allreduce_cb(buf, count, m->allreduce_user) ? AHA_ERR_STATE : AHA_OK;
  } else {
    set_error("no all-reduce installed");
    return AHA_ERR_STATE;
  }
  if (rc) return rc;
  AHA_HIP_CHECK(hipStreamSynchronize(m->stream));
  return AHA_OK;
  API_GUARD_END
}

int aha_hip_vision_encode(aha_model* m, const aha_mm_input* mm, void* out_dev, int64_t* n_tokens) {
  API_GUARD_BEGIN
  if (!m || !mm) {
    set_error("null argument");
    return AHA_ERR_INVALID;
  }
  return vision_encode(m, mm, out_dev, n_tokens);
  API_GUARD_END
}

int aha_hip_logmel(const float* samples, int64_t n_samples, float* out, void* stream) {
  API_GUARD_BEGIN
  if (!samples || !out || n_samples < 401) {
    set_error("logmel: need more than 400 samples");
    return AHA_ERR_INVALID;
  }
  return logmel_standalone(samples, &n_samples, 1, out, (hipStream_t)stream);
  API_GUARD_END
}

int aha_hip_logmel_batch(const float* samples, const int64_t* n_samples, size_t n_clips, float* out, void* stream) {
  API_GUARD_BEGIN
  if (!samples || !n_samples || !out || n_clips == 0 || n_clips > ((size_t)1 << 20)) {
    set_error("logmel_batch: null argument or no clips");
    return AHA_ERR_INVALID;
  }
  int64_t frames = 0;
  for (size_t j = 0; j < n_clips; ++j) {
    if (n_samples[j] < 401 || n_samples[j] > ((int64_t)1 << 34)) {
      set_error("logmel_batch: clip " + std::to_string(j) + ": need more than 400 samples");
      return AHA_ERR_INVALID;
    }
    frames += n_samples[j] / 160;
  }
  if (frames > ((int64_t)1 << 31) / 128) {
    set_error("logmel_batch: too many frames for one call");
    return AHA_ERR_INVALID;
  }
  return logmel_standalone(samples, n_samples, n_clips, out, (hipStream_t)stream);
  API_GUARD_END
}

int64_t aha_hip_audio_resample(aha_ctx* ctx, const float* pcm, int64_t n_frames, int32_t channels, int32_t orig_sr,
                               int32_t target_sr, float* out, int64_t out_cap) {
  API_GUARD_BEGIN
  if (!ctx || n_frames < 0 || channels < 1 || orig_sr <= 0 || target_sr <= 0 || (n_frames > 0 && !pcm)) {
    set_error("audio_resample: frequencies must be positive, channels >= 1");  // audio_utils.rs:225-227
    return AHA_ERR_INVALID;
  }
  return audio_resample(ctx, pcm, n_frames, channels, orig_sr, target_sr, out, out_cap);
  API_GUARD_END
}

int aha_hip_debug_audio_embeds(aha_model* m, float* out, size_t n) {
  API_GUARD_BEGIN
  if (!m || !out) {
    set_error("null argument");
    return AHA_ERR_INVALID;
  }
  return audio_debug_embeds(m, out, n);
  API_GUARD_END
}

int aha_hip_argmax(const float* x, int64_t n, uint32_t* out_dev, void* stream) {
  API_GUARD_BEGIN
  if (!x || !out_dev || n <= 0) {
    set_error("argmax: bad arguments");
    return AHA_ERR_INVALID;
  }
  hipStream_t st = (hipStream_t)stream;
  float* wv = nullptr;
  uint32_t* wi = nullptr;
  AHA_HIP_CHECK(hipMalloc((void**)&wv, 256 * 4));
  AHA_HIP_CHECK(hipMalloc((void**)&wi, 256 * 4));
  launch_argmax_f32(x, n, wv, wi, out_dev, st);
  hipError_t e = hipGetLastError();
  hipStreamSynchronize(st);
  hipFree(wv);
  hipFree(wi);
  AHA_HIP_CHECK(e);
  return AHA_OK;
  API_GUARD_END
}

int aha_hip_debug_image_embeds(aha_model* m, int which, float* out, size_t n) {
  API_GUARD_BEGIN
  if (!m || !out) {
    set_error("null argument");
    return AHA_ERR_INVALID;
  }
  return vision_debug_embeds(m, which, out, n);
  API_GUARD_END
}

}  // extern "C"
