// Host orchestration of the Qwen3 decoder stack on one MI355X.
//   create      <- Qwen3Model::new                      /root/reference/src/models/qwen3/model.rs:104-134
//   prefill     <- Qwen3Model::forward_hidden (S > 1)   /root/reference/src/models/qwen3/model.rs:146-189
//   decode step <- the same with S == 1, mask = None    (generate.rs:135-143 drives it once per token)
// The KV cache is paged (64-token pages, K / V blocks fragment-major, see common.h) and must be indistinguishable from
// the reference's Tensor::cat growth (modules.rs:558-566).
#include "model.h"
#include "mxfp8.h"

#include <math.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <chrono>
#include <deque>

#include "common.h"
#include "audio.h"
#include "sampler.h"
#include "vision.h"

namespace aha {

static thread_local std::string g_last_error;
void set_error(const std::string& msg) { g_last_error = msg; }
const char* last_error_cstr() { return g_last_error.c_str(); }

// ---------------------------------------------------------------------------------------------------------------
ProfScope::ProfScope(aha_model* m_, const char* cls, double bytes, double flops) : m(m_) {
  if (!m->profiling) return;
  auto it = m->prof_cls.find(cls);
  int c;
  if (it == m->prof_cls.end()) {
    c = (int)m->prof_names.size();
    m->prof_cls[cls] = c;
    m->prof_names.push_back(cls);
    m->prof_acc.emplace_back();
  } else {
    c = it->second;
  }
  ProfRec r;
  r.cls = c;
  r.bytes = bytes;
  r.flops = flops;
  hipEventCreate(&r.e0);
  hipEventCreate(&r.e1);
  hipEventRecord(r.e0, m->stream);
  idx = (int)m->prof.size();
  m->prof.push_back(r);
}
ProfScope::~ProfScope() {
  if (idx >= 0) hipEventRecord(m->prof[idx].e1, m->stream);
}
int prof_collect(aha_model* m) {
  if (m->prof.empty()) return AHA_OK;
  AHA_HIP_CHECK(hipStreamSynchronize(m->stream));
  for (auto& r : m->prof) {
    float ms = 0.f;
    hipEventElapsedTime(&ms, r.e0, r.e1);
    auto& a = m->prof_acc[r.cls];
    a.ms += ms;
    a.bytes += r.bytes;
    a.flops += r.flops;
    a.n += 1;
    hipEventDestroy(r.e0);
    hipEventDestroy(r.e1);
  }
  m->prof.clear();
  return AHA_OK;
}

// ---------------------------------------------------------------------------------------------------------------
int dev_alloc(aha_model* m, size_t bytes, void** out, bool zero) {
  void* p = nullptr;
  hipError_t e = hipMalloc(&p, bytes ? bytes : 16);
  if (e != hipSuccess) {
    set_error("hipMalloc of " + std::to_string(bytes) + " bytes failed: " + hipGetErrorString(e));
    return e == hipErrorOutOfMemory ? AHA_ERR_OOM : AHA_ERR_HIP;
  }
  if (zero) AHA_HIP_CHECK(hipMemsetAsync(p, 0, bytes, m->stream));
  m->owned.push_back(p);
  *out = p;
  return AHA_OK;
}

const aha_tensor_view* find_tensor(const aha_tensor_view* w, size_t nw, const std::string& name) {
  for (size_t i = 0; i < nw; ++i)
    if (w[i].name && name == w[i].name) return &w[i];
  return nullptr;
}

static inline uint16_t f32_to_bf16_host(float f) {
  uint32_t u;
  memcpy(&u, &f, 4);
  if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x40u);
  u += 0x7fffu + ((u >> 16) & 1u);
  return (uint16_t)(u >> 16);
}
static inline float f16_to_f32_host(uint16_t h) {
  const uint32_t s = (h >> 15) & 1u, e = (h >> 10) & 0x1fu, f = h & 0x3ffu;
  uint32_t u;
  if (e == 0) {
    if (f == 0) u = s << 31;
    else {
      int sh = 0;
      uint32_t ff = f;
      while (!(ff & 0x400u)) { ff <<= 1; ++sh; }
      u = (s << 31) | ((uint32_t)(127 - 15 - sh + 1) << 23) | ((ff & 0x3ffu) << 13);
    }
  } else if (e == 31) u = (s << 31) | 0x7f800000u | (f << 13);
  else u = (s << 31) | ((e + 112u) << 23) | (f << 13);
  float r;
  memcpy(&r, &u, 4);
  return r;
}

// host tensor (bf16 / f16 / f32) -> device bf16, viewed as (rows, cols) row-major, optionally zero-padded
int upload_tensor(aha_model* m, const aha_tensor_view* t, const std::vector<int64_t>& shape, void** out,
                  int64_t pad_rows_to, int64_t pad_cols_to) {
  int64_t n = 1;
  for (auto s : shape) n *= s;
  int64_t tn = 1;
  for (int i = 0; i < t->ndim; ++i) tn *= t->shape[i];
  if (tn != n) {
    std::string got;
    for (int i = 0; i < t->ndim; ++i) got += (i ? "," : "") + std::to_string(t->shape[i]);
    std::string want;
    for (size_t i = 0; i < shape.size(); ++i) want += (i ? "," : "") + std::to_string(shape[i]);
    set_error(std::string("tensor ") + t->name + " has shape (" + got + "), expected (" + want + ")");
    return AHA_ERR_SHAPE;
  }
  const int64_t cols = shape.back();
  const int64_t rows = n / cols;
  const int64_t prow = std::max(rows, pad_rows_to), pcol = std::max(cols, pad_cols_to);
  std::vector<uint16_t> tmp;
  const void* src = t->data;
  if (t->on_device && t->dtype != AHA_BF16) {
    set_error(std::string("tensor ") + t->name + ": device-resident weights must be bf16");
    return AHA_ERR_UNSUPPORTED;
  }
  if (t->dtype == AHA_F32) {
    tmp.resize(n);
    const float* f = (const float*)t->data;
    for (int64_t i = 0; i < n; ++i) tmp[i] = f32_to_bf16_host(f[i]);
    src = tmp.data();
  } else if (t->dtype == AHA_F16) {
    tmp.resize(n);
    const uint16_t* h = (const uint16_t*)t->data;
    for (int64_t i = 0; i < n; ++i) tmp[i] = f32_to_bf16_host(f16_to_f32_host(h[i]));
    src = tmp.data();
  } else if (t->dtype != AHA_BF16) {
    set_error(std::string("tensor ") + t->name + ": unsupported dtype");
    return AHA_ERR_UNSUPPORTED;
  }
  void* d = nullptr;
  const bool padded = prow != rows || pcol != cols;
  int rc = dev_alloc(m, (size_t)prow * pcol * 2, &d, padded);
  if (rc) return rc;
  if (!padded) AHA_HIP_CHECK(hipMemcpy(d, src, (size_t)n * 2, hipMemcpyDefault));
  else {
    AHA_HIP_CHECK(hipStreamSynchronize(m->stream));
    AHA_HIP_CHECK(hipMemcpy2D(d, (size_t)pcol * 2, src, (size_t)cols * 2, (size_t)cols * 2, (size_t)rows, hipMemcpyDefault));
  }
  *out = d;
  return AHA_OK;
}

static int need(const aha_tensor_view* w, size_t nw, const std::string& name, const aha_tensor_view** out) {
  *out = find_tensor(w, nw, name);
  if (!*out) {
    set_error("missing weight tensor: " + name);
    return AHA_ERR_MISSING_WEIGHT;
  }
  return AHA_OK;
}

// copy `rows` rows of a host bf16-convertible tensor into dst rows [row0, row0+rows) of a device (.., cols) bf16 matrix
static int upload_rows_into(aha_model* m, const aha_tensor_view* t, int64_t rows, int64_t cols, void* dst, int64_t row0) {
  int64_t tn = 1;
  for (int i = 0; i < t->ndim; ++i) tn *= t->shape[i];
  if (tn != rows * cols) {
    set_error(std::string("tensor ") + t->name + " has " + std::to_string(tn) + " elements, expected " + std::to_string(rows * cols));
    return AHA_ERR_SHAPE;
  }
  std::vector<uint16_t> tmp;
  const void* src = t->data;
  if (t->on_device && t->dtype != AHA_BF16) {
    set_error(std::string("tensor ") + t->name + ": device-resident weights must be bf16");
    return AHA_ERR_UNSUPPORTED;
  }
  if (t->dtype == AHA_F32) {
    tmp.resize(tn);
    for (int64_t i = 0; i < tn; ++i) tmp[i] = f32_to_bf16_host(((const float*)t->data)[i]);
    src = tmp.data();
  } else if (t->dtype == AHA_F16) {
    tmp.resize(tn);
    for (int64_t i = 0; i < tn; ++i) tmp[i] = f32_to_bf16_host(f16_to_f32_host(((const uint16_t*)t->data)[i]));
    src = tmp.data();
  } else if (t->dtype != AHA_BF16) {
    set_error(std::string("tensor ") + t->name + ": unsupported dtype");
    return AHA_ERR_UNSUPPORTED;
  }
  AHA_HIP_CHECK(hipMemcpy((char*)dst + (size_t)row0 * cols * 2, src, (size_t)tn * 2, hipMemcpyDefault));
  return AHA_OK;
}

// bf16 view of a checkpoint tensor (host tensors are converted into tmp when they are f32 / f16)
static int bf16_source(const aha_tensor_view* t, int64_t expect, std::vector<uint16_t>& tmp, const void** src) {
  int64_t tn = 1;
  for (int i = 0; i < t->ndim; ++i) tn *= t->shape[i];
  if (tn != expect) {
    set_error(std::string("tensor ") + t->name + " has " + std::to_string(tn) + " elements, expected " + std::to_string(expect));
    return AHA_ERR_SHAPE;
  }
  *src = t->data;
  if (t->on_device && t->dtype != AHA_BF16) {
    set_error(std::string("tensor ") + t->name + ": device-resident weights must be bf16");
    return AHA_ERR_UNSUPPORTED;
  }
  if (t->dtype == AHA_F32) {
    tmp.resize(tn);
    for (int64_t i = 0; i < tn; ++i) tmp[i] = f32_to_bf16_host(((const float*)t->data)[i]);
    *src = tmp.data();
  } else if (t->dtype == AHA_F16) {
    tmp.resize(tn);
    for (int64_t i = 0; i < tn; ++i) tmp[i] = f32_to_bf16_host(f16_to_f32_host(((const uint16_t*)t->data)[i]));
    *src = tmp.data();
  } else if (t->dtype != AHA_BF16) {
    set_error(std::string("tensor ") + t->name + ": unsupported dtype");
    return AHA_ERR_UNSUPPORTED;
  }
  return AHA_OK;
}
// copy the (nr x nc) block at (r0, c0) of a (rows x cols) checkpoint matrix into dst rows [dr0, dr0+nr) of a (.. x nc) matrix
static int upload_block(aha_model* m, const aha_tensor_view* t, int64_t rows, int64_t cols, int64_t r0, int64_t nr, int64_t c0,
                        int64_t nc, void* dst, int64_t dr0) {
  std::vector<uint16_t> tmp;
  const void* src;
  int rc = bf16_source(t, rows * cols, tmp, &src);
  if (rc) return rc;
  AHA_HIP_CHECK(hipMemcpy2D((char*)dst + (size_t)dr0 * nc * 2, (size_t)nc * 2, (const char*)src + ((size_t)r0 * cols + c0) * 2,
                            (size_t)cols * 2, (size_t)nc * 2, (size_t)nr, hipMemcpyDefault));
  return AHA_OK;
}

// gate/up -> one (2I, H) matrix of alternating 16-row blocks: [gate 0..15 | up 0..15 | gate 16..31 | up 16..31 | ...]
static int upload_gate_up(aha_model* m, const aha_tensor_view* g, const aha_tensor_view* u, int64_t I_full, int64_t row0, int64_t I,
                          int64_t H, void** out) {
  if (I % 16) {
    set_error("intermediate_size must be a multiple of 16");
    return AHA_ERR_UNSUPPORTED;
  }
  void* d = nullptr;
  int rc = dev_alloc(m, (size_t)2 * I * H * 2, &d);
  if (rc) return rc;
  for (int which = 0; which < 2; ++which) {
    const aha_tensor_view* t = which ? u : g;
    int64_t tn = 1;
    for (int i = 0; i < t->ndim; ++i) tn *= t->shape[i];
    if (tn != I_full * H) {
      set_error(std::string("tensor ") + t->name + " has wrong size");
      return AHA_ERR_SHAPE;
    }
    std::vector<uint16_t> tmp;
    const void* src = t->data;
    if (t->on_device && t->dtype != AHA_BF16) {
      set_error(std::string("tensor ") + t->name + ": device-resident weights must be bf16");
      return AHA_ERR_UNSUPPORTED;
    }
    if (t->dtype == AHA_F32) {
      tmp.resize(tn);
      for (int64_t i = 0; i < tn; ++i) tmp[i] = f32_to_bf16_host(((const float*)t->data)[i]);
      src = tmp.data();
    } else if (t->dtype == AHA_F16) {
      tmp.resize(tn);
      for (int64_t i = 0; i < tn; ++i) tmp[i] = f32_to_bf16_host(f16_to_f32_host(((const uint16_t*)t->data)[i]));
      src = tmp.data();
    } else if (t->dtype != AHA_BF16) {
      set_error("unsupported dtype");
      return AHA_ERR_UNSUPPORTED;
    }
    const size_t blk = (size_t)16 * H * 2;
    AHA_HIP_CHECK(hipMemcpy2D((char*)d + which * blk, 2 * blk, (const char*)src + (size_t)row0 * H * 2, blk, blk, (size_t)(I / 16),
                              hipMemcpyDefault));
  }
  *out = d;
  return AHA_OK;
}

// ---------------------------------------------------------------------------------------------------------------
// paged KV cache
static int alloc_slab(aha_model* m) {
  void* p = nullptr;
  const size_t bytes = (size_t)m->layer_stride * m->desc.num_hidden_layers;
  hipError_t e = hipMalloc(&p, bytes);
  if (e != hipSuccess) {
    set_error("KV slab hipMalloc of " + std::to_string(bytes) + " bytes failed: " + hipGetErrorString(e));
    return e == hipErrorOutOfMemory ? AHA_ERR_OOM : AHA_ERR_HIP;
  }
  // pages must never hold NaN bit patterns: masked P (= 0) still multiplies the V slots of the page tail
  AHA_HIP_CHECK(hipMemsetAsync(p, 0, bytes, m->stream));
  m->slabs.push_back(p);
  std::vector<uint64_t> pages(m->pages_per_slab);
  for (size_t i = 0; i < m->pages_per_slab; ++i) pages[i] = (uint64_t)(uintptr_t)p + i * m->page_bytes;
  if (m->scramble_pages) {
    uint64_t s = 0x9e3779b97f4a7c15ull * (m->slabs.size() + 1);
    for (size_t i = pages.size(); i > 1; --i) {
      s = s * 6364136223846793005ull + 1442695040888963407ull;
      std::swap(pages[i - 1], pages[(s >> 33) % i]);
    }
  }
  // free list is popped from the back
  for (size_t i = pages.size(); i > 0; --i) m->free_pages.push_back(pages[i - 1]);
  return AHA_OK;
}

int model_ensure_pages(aha_model* m, size_t tokens) {
  const size_t needp = (tokens + KV_PAGE_TOKENS - 1) / KV_PAGE_TOKENS;
  if (needp <= m->n_pages) return AHA_OK;
  if (needp > m->page_table_cap) {
    size_t cap = std::max<size_t>(1024, m->page_table_cap);
    while (cap < needp) cap *= 2;
    uint64_t* nd = nullptr;
    AHA_HIP_CHECK(hipMalloc((void**)&nd, cap * sizeof(uint64_t)));
    AHA_HIP_CHECK(hipStreamSynchronize(m->stream));
    if (m->d_page_ptrs) AHA_HIP_CHECK(hipFree(m->d_page_ptrs));
    m->d_page_ptrs = nd;
    m->page_table_cap = cap;
    if (m->n_pages)
      AHA_HIP_CHECK(hipMemcpy(m->d_page_ptrs, m->h_page_ptrs.data(), m->n_pages * sizeof(uint64_t), hipMemcpyHostToDevice));
  }
  const size_t first_new = m->n_pages;
  while (m->n_pages < needp) {
    if (m->free_pages.empty()) {
      int rc = alloc_slab(m);
      if (rc) return rc;
    }
    const uint64_t p = m->free_pages.back();
    m->free_pages.pop_back();
    if (m->h_page_ptrs.size() <= m->n_pages) m->h_page_ptrs.resize(m->n_pages + 1);
    if (m->n_pages == 0) {  // a lone page is a progression of any step
      m->lin_p0 = p;
      m->lin_step = (int64_t)m->page_bytes;
      m->lin_pages = 1;
    } else if (m->lin_pages == m->n_pages) {  // unbroken so far: the second page sets the step, every later one has to keep it
      if (m->n_pages == 1) m->lin_step = (int64_t)(p - m->lin_p0);
      if (m->lin_step != 0 && p == m->lin_p0 + (uint64_t)((int64_t)m->n_pages * m->lin_step)) m->lin_pages = m->n_pages + 1;
    }
    m->h_page_ptrs[m->n_pages++] = p;
  }
  AHA_HIP_CHECK(hipMemcpyAsync(m->d_page_ptrs + first_new, m->h_page_ptrs.data() + first_new,
                               (m->n_pages - first_new) * sizeof(uint64_t), hipMemcpyHostToDevice, m->stream));
  // h_page_ptrs is pageable: the async copy above is staged synchronously by the runtime, so the vector may be reused
  return AHA_OK;
}

KvLayer model_kv_layer(aha_model* m, int layer) {
  KvLayer kv;
  kv.page_ptrs = m->d_page_ptrs;
  kv.layer_off = (uint64_t)layer * m->layer_stride;
  kv.kvh = m->desc.num_key_value_heads;
  kv.d = m->desc.head_dim;
  return kv;
}

// ---- KV hand-back (include/aha_hip.h aha_hip_kv_export / aha_hip_kv_import) ---------------------------------------------------
// One block per (page, layer, head, K|V): 16 KB = the head's fragment-major K (or V) block of that page, copied as bytes between
// the page (page_ptrs[page] + layer * layer_stride + block offset) and the packed buffer [layer][page][head][K | V].
constexpr int KV_BLOCK_BYTES = KV_PAGE_TOKENS * 128 * 2;
__global__ __launch_bounds__(256) void kv_pack_kernel(const uint64_t* __restrict__ page_ptrs, uint64_t layer_stride, int kvh_local,
                                                      char* __restrict__ buf, int buf_heads, int buf_head0, int local_head0, int n_pages,
                                                      int to_pages) {
  const int page = (int)blockIdx.x, layer = (int)blockIdx.y, h = (int)blockIdx.z >> 1, kv = (int)blockIdx.z & 1;
  char* pg = reinterpret_cast<char*>(page_ptrs[page] + (uint64_t)layer * layer_stride) +
             ((size_t)kv * kvh_local + (size_t)(local_head0 + h)) * KV_BLOCK_BYTES;
  char* bf = buf + ((((size_t)layer * n_pages + page) * buf_heads + (size_t)(buf_head0 + h)) * 2 + kv) * KV_BLOCK_BYTES;
  const u32x4_t* src = reinterpret_cast<const u32x4_t*>(to_pages ? bf : pg);
  u32x4_t* dst = reinterpret_cast<u32x4_t*>(to_pages ? pg : bf);
  u32x4_t v[KV_BLOCK_BYTES / 16 / 256];
#pragma unroll
  for (int i = 0; i < KV_BLOCK_BYTES / 16 / 256; ++i) v[i] = src[threadIdx.x + i * 256];
#pragma unroll
  for (int i = 0; i < KV_BLOCK_BYTES / 16 / 256; ++i) dst[threadIdx.x + i * 256] = v[i];
}

int model_kv_export(aha_model* m, void* out_dev, size_t out_bytes, size_t* bytes_needed, size_t* n_tokens, int64_t* rope_delta) {
  const aha_model_desc& c = m->desc;
  if (c.head_dim != 128) {
    set_error("kv_export: head_dim 128 only");
    return AHA_ERR_UNSUPPORTED;
  }
  const size_t pages = (m->cache_len + KV_PAGE_TOKENS - 1) / KV_PAGE_TOKENS;
  const size_t need_bytes = (size_t)c.num_hidden_layers * pages * c.num_key_value_heads * 2 * KV_BLOCK_BYTES;
  if (bytes_needed) *bytes_needed = need_bytes;
  if (n_tokens) *n_tokens = m->cache_len;
  if (rope_delta) *rope_delta = m->rope_delta;
  if (!out_dev || pages == 0) return AHA_OK;
  if (out_bytes < need_bytes) {
    set_error("kv_export: the buffer holds " + std::to_string(out_bytes) + " bytes, " + std::to_string(need_bytes) + " are needed");
    return AHA_ERR_INVALID;
  }
  AHA_HIP_CHECK(hipSetDevice(m->ctx->device));
  hipLaunchKernelGGL(kv_pack_kernel, dim3((unsigned)pages, (unsigned)c.num_hidden_layers, (unsigned)c.num_key_value_heads * 2), dim3(256), 0,
                     m->stream, m->d_page_ptrs, m->layer_stride, c.num_key_value_heads, (char*)out_dev, c.num_key_value_heads, 0, 0, (int)pages, 0);
  AHA_HIP_CHECK(hipGetLastError());
  AHA_HIP_CHECK(hipStreamSynchronize(m->stream));   // the caller hands the buffer to a collective on another stream
  return AHA_OK;
}

int model_kv_import(aha_model* m, const void* in_dev, size_t in_bytes, int src_heads, int src_head0, int dst_head0, int n_heads, size_t n_tokens,
                    int64_t rope_delta) {
  const aha_model_desc& c = m->desc;
  if (c.head_dim != 128) {
    set_error("kv_import: head_dim 128 only");
    return AHA_ERR_UNSUPPORTED;
  }
  if (m->tp_size > 1) {   // the hand-back ends in an UN-sharded model (decode stays single-GPU); a sharded destination would need a head map
    set_error("kv_import: the destination model is tensor-parallel (tp_size " + std::to_string(m->tp_size) + "); import into an un-sharded model");
    return AHA_ERR_UNSUPPORTED;
  }
  if (!in_dev || n_heads <= 0 || src_head0 < 0 || dst_head0 < 0 || src_head0 + n_heads > src_heads || dst_head0 + n_heads > c.num_key_value_heads) {
    set_error("kv_import: head ranges out of bounds (buffer holds " + std::to_string(src_heads) + " heads, the model " +
              std::to_string(c.num_key_value_heads) + ")");
    return AHA_ERR_INVALID;
  }
  if (n_tokens == 0) return AHA_OK;
  const size_t pages = (n_tokens + KV_PAGE_TOKENS - 1) / KV_PAGE_TOKENS;
  // the kernel reads layers x pages x src_heads x (K | V) blocks of 16 KB from in_dev: the caller states what the buffer holds
  const size_t need_bytes = (size_t)c.num_hidden_layers * pages * (size_t)src_heads * 2 * KV_BLOCK_BYTES;
  if (in_bytes < need_bytes) {
    set_error("kv_import: the buffer holds " + std::to_string(in_bytes) + " bytes, " + std::to_string(need_bytes) + " are needed for " +
              std::to_string(n_tokens) + " tokens of " + std::to_string(src_heads) + " heads");
    return AHA_ERR_INVALID;
  }
  AHA_HIP_CHECK(hipSetDevice(m->ctx->device));
  int rc = model_ensure_pages(m, n_tokens);
  if (rc) return rc;
  hipLaunchKernelGGL(kv_pack_kernel, dim3((unsigned)pages, (unsigned)c.num_hidden_layers, (unsigned)n_heads * 2), dim3(256), 0, m->stream,
                     m->d_page_ptrs, m->layer_stride, c.num_key_value_heads, (char*)in_dev, src_heads, src_head0, dst_head0, (int)pages, 1);
  AHA_HIP_CHECK(hipGetLastError());
  AHA_HIP_CHECK(hipStreamSynchronize(m->stream));   // the caller may free / reuse the buffer
  m->cache_len = n_tokens;
  m->rope_delta = rope_delta;
  m->rope_delta_valid = true;
  m->have_logits = false;        // whatever logits an earlier forward left on the device belong to another cache
  m->logits_assembled = false;
  return AHA_OK;
}

static int assemble_logits(aha_model* m);

// D11 candidates: see kernels_sample.hip.  Works on the logits the last forward_initial / forward_step / decode_greedy left
// on the device; the caller slices `ctx` the way use_repeat_penalty does (sample.rs:47-53: the last repeat_last_n generated ids).
int model_sample_candidates(aha_model* m, const uint32_t* ctx, size_t n_ctx, float repeat_penalty, float temperature, int k,
                            float* vals_out, uint32_t* idx_out, float* max_out, float* sumexp_out) {
  const int V = m->desc.vocab_size;
  if (!m->have_logits) {
    set_error("sample_candidates: no forward call has produced logits yet");
    return AHA_ERR_STATE;
  }
  if (!sample_shape_ok(V, k)) {
    set_error("sample_candidates: k must be in [1, 64] (and vocab * k within the stage-2 capacity)");
    return AHA_ERR_UNSUPPORTED;
  }
  if (!(repeat_penalty > 0.f) || (n_ctx && !ctx) || !vals_out || !idx_out) {
    set_error("sample_candidates: bad argument");
    return AHA_ERR_INVALID;
  }
  const int nw = sample_stage1_waves(V);
  // device scratch: cand_val (+ intermediates) | part_m | part_s | out block {vals[64] f32, ms[2] f32, idx[64] u32}; cand_idx separately.
  // One pinned host block carries the context up and the 520-byte out block down (pageable copies cost ~30 us each).
  constexpr size_t OUT_WORDS = 64 + 2 + 64;
  if (!m->d_samp_f) {
    const size_t nc = ((size_t)nw + 16) * 64;  // stage-1 candidates + the 16 x 64 intermediates behind them
    const size_t nf = nc + 2 * (size_t)nw + OUT_WORDS, nu = nc;
    void *pw = nullptr, *pf = nullptr, *pu = nullptr;
    if (int rc = dev_alloc(m, (size_t)V * 4, &pw, false)) return rc;
    if (int rc = dev_alloc(m, nf * 4, &pf, false)) return rc;
    if (int rc = dev_alloc(m, nu * 4, &pu, false)) return rc;
    m->d_samp_work = (float*)pw;
    m->d_samp_f = (float*)pf;
    m->d_samp_u = (unsigned*)pu;
  }
  if (!m->h_samp || n_ctx > m->samp_ctx_cap) {
    const size_t cap = std::max<size_t>(1024, n_ctx * 2);
    void* pd = nullptr;
    if (int rc = dev_alloc(m, cap * 4, &pd, false)) return rc;  // a smaller predecessor stays in m->owned until destroy
    uint32_t* ph = nullptr;
    AHA_HIP_CHECK(hipHostMalloc((void**)&ph, (cap + OUT_WORDS) * 4));
    if (m->h_samp) hipHostFree(m->h_samp);
    m->h_samp = ph;
    m->d_samp_ctx = (uint32_t*)pd;
    m->samp_ctx_cap = cap;
  }
  if (int rc = assemble_logits(m)) return rc;
  const float* src = m->d_logits;
  if (repeat_penalty != 1.0f && n_ctx > 0) {  // sample.rs:47 `repeat_penalty == 1.0` => logits unchanged
    memcpy(m->h_samp, ctx, n_ctx * 4);
    AHA_HIP_CHECK(hipMemcpyAsync(m->d_samp_ctx, m->h_samp, n_ctx * 4, hipMemcpyHostToDevice, m->stream));
    AHA_HIP_CHECK(hipMemcpyAsync(m->d_samp_work, m->d_logits, (size_t)V * 4, hipMemcpyDeviceToDevice, m->stream));
    launch_repeat_penalty(m->d_logits, m->d_samp_work, m->d_samp_ctx, (int)n_ctx, repeat_penalty, V, m->stream);
    src = m->d_samp_work;
  }
  // `&logits / temperature` in LogitsProcessor::sample is an affine by 1/T computed in f64 and applied in f32
  const float inv_temp = temperature > 0.f ? (float)(1.0 / (double)temperature) : 1.0f;
  float* cand_val = m->d_samp_f;
  float* part_m = cand_val + ((size_t)nw + 16) * 64;
  float* part_s = part_m + nw;
  float* out_val = part_s + nw;
  float* out_ms = out_val + 64;
  unsigned* out_idx = reinterpret_cast<unsigned*>(out_ms + 2);
  unsigned* cand_idx = m->d_samp_u;
  launch_topk_candidates(src, V, k, inv_temp, cand_val, cand_idx, part_m, part_s, out_val, out_idx, out_ms, m->stream);
  AHA_HIP_CHECK(hipGetLastError());
  uint32_t* h_out = m->h_samp + m->samp_ctx_cap;
  AHA_HIP_CHECK(hipMemcpyAsync(h_out, out_val, OUT_WORDS * 4, hipMemcpyDeviceToHost, m->stream));
  AHA_HIP_CHECK(hipStreamSynchronize(m->stream));
  memcpy(vals_out, h_out, (size_t)k * 4);
  memcpy(idx_out, h_out + 66, (size_t)k * 4);
  if (max_out) memcpy(max_out, h_out + 64, 4);
  if (sumexp_out) memcpy(sumexp_out, h_out + 65, 4);
  return AHA_OK;
}

int model_last_logits(aha_model* m, float* logits_out) {
  if (!m->have_logits) {
    set_error("last_logits: no forward call has produced logits yet");
    return AHA_ERR_STATE;
  }
  if (int rc = assemble_logits(m)) return rc;
  AHA_HIP_CHECK(hipMemcpyAsync(m->h_logits, m->d_logits, (size_t)m->desc.vocab_size * 4, hipMemcpyDeviceToHost, m->stream));
  AHA_HIP_CHECK(hipStreamSynchronize(m->stream));
  memcpy(logits_out, m->h_logits, (size_t)m->desc.vocab_size * 4);
  return AHA_OK;
}

int model_clear_cache(aha_model* m) {
  // QKNormAttention::clear_kv_cache (modules.rs:581-583): the cache becomes empty; pages go back to the pool
  for (size_t i = m->n_pages; i > 0; --i) m->free_pages.push_back(m->h_page_ptrs[i - 1]);
  m->n_pages = 0;
  m->lin_pages = 0;
  m->cache_len = 0;
  m->rope_delta = 0;
  m->rope_delta_valid = false;
  return AHA_OK;
}

// Exact 13-bit copies (kernels_gemv_pk13.hip).  model_free_packed drops them all: the matrices are about to change, or the model goes.
static void model_free_packed(aha_model* m, const char* why) {
  for (Pk13Entry& e : m->pk13) {
    if (e.slot->p) {
      hipFree(e.slot->p);
      e.status = why;
    }
    *e.slot = Pk13Copy{};
  }
}

// Called once, at the end of model_create: the four layer matrices and lm_head of an unsharded model get a copy each if the matrix is
// large enough, in whole units, finite, with weights below the format's window in at most PK13_MAX_EXC rows (the exception rows, which the
// matvec then computes from the bf16 matrix), and the device has the copies' bytes plus a tenth more free -- else the model keeps reading
// bf16, and aha_hip_pk13_status says why.  AHA_WPACK=0 makes no copies.
static int model_pack_weights(aha_model* m) {
  const aha_model_desc& c = m->desc;
  struct Mat { const void* w; int N, K; };
  std::vector<Mat> mats;
  const int H = c.hidden_size, I = c.intermediate_size, nq = c.num_attention_heads * c.head_dim, nkv = c.num_key_value_heads * c.head_dim;
  for (int li = 0; li < c.num_hidden_layers; ++li) {
    LayerWeights& L = m->layers[li];
    const std::string p = "layers." + std::to_string(li) + ".";
    m->pk13.push_back({p + "self_attn.q_proj/k_proj/v_proj.weight", &L.p_wqkv, ""});
    mats.push_back({L.wqkv, nq + 2 * nkv, H});
    m->pk13.push_back({p + "self_attn.o_proj.weight", &L.p_wo, ""});
    mats.push_back({L.wo, H, nq});
    m->pk13.push_back({p + "mlp.gate_proj/up_proj.weight", &L.p_wgu, ""});
    mats.push_back({L.wgu, 2 * I, H});
    m->pk13.push_back({p + "mlp.down_proj.weight", &L.p_wdown, ""});
    mats.push_back({L.wdown, H, I});
  }
  m->pk13.push_back({c.tie_word_embeddings ? "embed_tokens.weight (tied lm_head)" : "lm_head.weight", &m->p_lm_head, ""});
  mats.push_back({m->lm_head, m->lm_rows, H});
  auto all = [&](const char* why) {
    for (Pk13Entry& e : m->pk13) {
      if (e.status.empty()) e.status = why;
      if (!e.slot->p) *e.slot = Pk13Copy{};
    }
    return AHA_OK;
  };
  const char* env = getenv("AHA_WPACK");
  if (env && atoi(env) == 0) return all("off (AHA_WPACK=0)");
  if (m->tp_size > 1 || m->cp_size > 1) return all("sharded model");
  std::vector<size_t> cand;
  for (size_t i = 0; i < mats.size(); ++i) {
    if (!gemv_pk13_shape_ok(mats[i].N, mats[i].K)) m->pk13[i].status = "K is not a multiple of 4096 (or above 32768)";
    else if ((int64_t)mats[i].N * mats[i].K < ((int64_t)1 << 24)) m->pk13[i].status = "fewer than 2^24 elements";
    else cand.push_back(i);
  }
  if (cand.empty()) return AHA_OK;
  hipStream_t st = m->stream;
  std::vector<Pk13Stats> h(cand.size());
  {
    Pk13Stats* d = nullptr;
    if (hipMalloc((void**)&d, cand.size() * sizeof(Pk13Stats)) != hipSuccess) {
      (void)hipGetLastError();
      return all("not enough device memory");
    }
    hipError_t e = hipMemsetAsync(d, 0, cand.size() * sizeof(Pk13Stats), st);
    for (size_t k = 0; k < cand.size() && e == hipSuccess; ++k) launch_pk13_stats(mats[cand[k]].w, mats[cand[k]].N, mats[cand[k]].K, d + k, st);
    if (e == hipSuccess) e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(h.data(), d, cand.size() * sizeof(Pk13Stats), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    hipFree(d);
    AHA_HIP_CHECK(e);
  }
  std::vector<size_t> take;
  std::vector<std::string> row_note(mats.size());   // the status of a matrix that is packed with exception rows
  size_t bytes = 0;
  for (size_t k = 0; k < cand.size(); ++k) {
    Pk13Copy& pk = *m->pk13[cand[k]].slot;
    // finite weights below the window in at most PK13_MAX_EXC rows: packed all the same, and the matvec reads those rows from bf16
    pk.nrows = h[k].bad ? pk13_exception_rows(h[k], pk.rows) : 0;
    if (h[k].nonfinite || pk.nrows > PK13_MAX_EXC) {
      m->pk13[cand[k]].status = std::to_string(h[k].bad) + " weights outside the window (Inf, NaN, or more than 30 binades below the matrix maximum)";
      pk = Pk13Copy{};
      continue;
    }
    if (h[k].bad) {
      std::string& why = row_note[cand[k]];
      why = std::to_string(h[k].bad) + " weights outside the window: packed, rows";
      for (int i = 0; i < pk.nrows; ++i) why += (i ? ", " : " ") + std::to_string(pk.rows[i]);
      why += " read from bf16";
    }
    pk.w = mats[cand[k]].w;
    pk.bh = pk13_base(h[k].max_e2);
    take.push_back(cand[k]);
    bytes += pk13_bytes(mats[cand[k]].N, mats[cand[k]].K);
  }
  size_t free_b = 0, total_b = 0;
  if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) {
    (void)hipGetLastError();
    free_b = 0;
  }
  if (take.empty()) return AHA_OK;
  if ((double)free_b < 1.1 * (double)bytes) return all("not enough device memory");
  for (size_t i : take) {
    if (hipMalloc(&m->pk13[i].slot->p, pk13_bytes(mats[i].N, mats[i].K)) != hipSuccess) {
      (void)hipGetLastError();
      m->pk13[i].slot->p = nullptr;
      model_free_packed(m, "not enough device memory");
      return all("not enough device memory");
    }
    launch_pk13_pack(mats[i].w, mats[i].N, mats[i].K, m->pk13[i].slot->bh, m->pk13[i].slot->p, st);
    m->pk13[i].status = row_note[i].empty() ? "packed" : row_note[i];
  }
  hipError_t e = hipGetLastError();
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  AHA_HIP_CHECK(e);
  return AHA_OK;
}

// aha_hip_model_quantize_weights (include/aha_hip.h): every check first, then every allocation, then the matrices one by one -- W becomes
// W' in place (the quantiser reads an element before it writes it), its (q, scales) copy lands in the matrix's slot.
int model_quantize_weights(aha_model* m, int32_t format, uint32_t flags) {
  const aha_model_desc& c = m->desc;
  if (format != AHA_WQ_MXFP8_E4M3 && format != AHA_WQ_MXFP4_E2M1) {
    set_error("quantize_weights: unknown format " + std::to_string(format) + " (AHA_WQ_MXFP8_E4M3 = 1, AHA_WQ_MXFP4_E2M1 = 2)");
    return AHA_ERR_INVALID;
  }
  if (flags & ~(uint32_t)AHA_WQ_LM_HEAD) {
    set_error("quantize_weights: unknown flag bits " + std::to_string(flags & ~(uint32_t)AHA_WQ_LM_HEAD) + " (AHA_WQ_LM_HEAD = 1)");
    return AHA_ERR_INVALID;
  }
  if (m->engine) {
    set_error("quantize_weights: the model has an engine (aha_hip_engine_destroy first)");
    return AHA_ERR_STATE;
  }
  if (m->wq_format != AHA_WQ_NONE) {
    if (m->wq_format == format && m->wq_flags == flags) return AHA_OK;
    set_error("quantize_weights: the model is already quantised with format " + std::to_string(m->wq_format) + ", flags " +
              std::to_string(m->wq_flags));
    return AHA_ERR_STATE;
  }
  if (m->cache_len != 0) {
    set_error("quantize_weights: the cache holds " + std::to_string(m->cache_len) + " tokens (aha_hip_clear_cache first)");
    return AHA_ERR_STATE;
  }
  if (m->tp_size > 1 || m->cp_size > 1) {
    set_error("quantize_weights: tensor- and context-parallel models are not supported");
    return AHA_ERR_UNSUPPORTED;
  }
  if ((c.arch != AHA_ARCH_QWEN3 && c.arch != AHA_ARCH_QWEN3VL && c.arch != AHA_ARCH_QWEN3ASR) || c.head_dim != 128) {
    set_error("quantize_weights: Qwen3, Qwen3-VL and Qwen3-ASR with head_dim 128 only (the models of generate_batch)");
    return AHA_ERR_UNSUPPORTED;
  }
  struct Mat { std::string name; void* w; int N, K; WQuant* slot; };
  std::vector<Mat> mats;
  const int H = c.hidden_size, I = c.intermediate_size, nq = c.num_attention_heads * 128, nkv = c.num_key_value_heads * 128;
  for (int li = 0; li < c.num_hidden_layers; ++li) {
    LayerWeights& L = m->layers[li];
    const std::string p = "layers." + std::to_string(li) + ".";
    mats.push_back({p + "self_attn.q_proj/k_proj/v_proj.weight", L.wqkv, nq + 2 * nkv, H, &L.q_wqkv});
    mats.push_back({p + "self_attn.o_proj.weight", L.wo, H, nq, &L.q_wo});
    mats.push_back({p + "mlp.gate_proj/up_proj.weight", L.wgu, 2 * I, H, &L.q_wgu});
    mats.push_back({p + "mlp.down_proj.weight", L.wdown, H, I, &L.q_wdown});
  }
  if (flags & AHA_WQ_LM_HEAD)
    mats.push_back({c.tie_word_embeddings ? "embed_tokens.weight (tied lm_head)" : "lm_head.weight", m->lm_head, c.vocab_size, H, &m->q_lm_head});
  for (const Mat& t : mats)
    if (t.K % MX_BLOCK) {
      set_error("quantize_weights: " + t.name + " has K = " + std::to_string(t.K) + ", not a multiple of 32 (the MX block)");
      return AHA_ERR_UNSUPPORTED;
    }
  AHA_HIP_CHECK(hipSetDevice(m->ctx->device));
  hipStream_t st = m->stream;
  const bool fp4 = format == AHA_WQ_MXFP4_E2M1;
  {   // every matrix finite (and inside the format's range) before any is touched
    int* d_flag = nullptr;
    std::vector<int> h_flag(mats.size(), 0);
    AHA_HIP_CHECK(hipMalloc((void**)&d_flag, mats.size() * sizeof(int)));
    hipError_t e = hipMemsetAsync(d_flag, 0, mats.size() * sizeof(int), st);
    for (size_t i = 0; i < mats.size() && e == hipSuccess; ++i) {
      if (fp4) launch_mxfp4_check(mats[i].w, (int64_t)mats[i].N * mats[i].K, d_flag + i, st);
      else launch_mxfp8_check(mats[i].w, (int64_t)mats[i].N * mats[i].K, d_flag + i, st);
    }
    if (e == hipSuccess) e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(h_flag.data(), d_flag, mats.size() * sizeof(int), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    hipFree(d_flag);
    AHA_HIP_CHECK(e);
    for (size_t i = 0; i < mats.size(); ++i)
      if (h_flag[i]) {
        set_error("quantize_weights: " + mats[i].name + " holds a weight that is not finite (or is " +
                  (fp4 ? "above 1.5 * 2^127" : "1.9375 * 2^127 or more") + " in magnitude); no matrix was modified");
        return AHA_ERR_INVALID;
      }
  }
  std::vector<void*> got;
  std::vector<WQuant> wq(mats.size());
  for (size_t i = 0; i < mats.size(); ++i) {
    const size_t bytes[2] = {(size_t)mats[i].N * mats[i].K / (fp4 ? 2 : 1), mxfp8_scale_words(mats[i].N, mats[i].K) * 4};
    for (int k = 0; k < 2; ++k) {
      void* p = nullptr;
      const hipError_t e = hipMalloc(&p, bytes[k]);
      if (e != hipSuccess) {
        (void)hipGetLastError();
        for (void* q : got) hipFree(q);
        set_error("quantize_weights: hipMalloc of " + std::to_string(bytes[k]) + " bytes for the copy of " + mats[i].name + " failed: " +
                  hipGetErrorString(e) + "; the model is unchanged");
        return e == hipErrorOutOfMemory ? AHA_ERR_OOM : AHA_ERR_HIP;
      }
      got.push_back(p);
      if (k == 0) wq[i].q = p;
      else wq[i].scales = (uint32_t*)p;
    }
  }
  // the matrices change from here on: a quantised model never reads the exact copies of what they were
  if (const hipError_t es = hipStreamSynchronize(st); es != hipSuccess) {
    for (void* q : got) hipFree(q);
    AHA_HIP_CHECK(es);
  }
  model_free_packed(m, "freed by quantize_weights");
  for (size_t i = 0; i < mats.size(); ++i) {
    if (fp4) launch_mxfp4_quantize(mats[i].w, mats[i].N, mats[i].K, wq[i].q, wq[i].scales, mats[i].w, st);
    else launch_mxfp8_quantize(mats[i].w, mats[i].N, mats[i].K, wq[i].q, wq[i].scales, mats[i].w, st);
  }
  hipError_t e = hipGetLastError();
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  for (void* p : got) m->owned.push_back(p);   // freed with the model whatever happened
  AHA_HIP_CHECK(e);
  for (size_t i = 0; i < mats.size(); ++i) *mats[i].slot = wq[i];
  m->wq_format = format;
  m->wq_flags = flags;
  m->have_logits = false;
  return AHA_OK;
}

// ---------------------------------------------------------------------------------------------------------------
int model_create(aha_ctx* ctx, const aha_model_desc* desc, const aha_tensor_view* w, size_t nw, aha_model** out) {
  if (!ctx || !desc || !out || (!w && nw)) {
    set_error("model_create: null argument");
    return AHA_ERR_INVALID;
  }
  const aha_model_desc& cd = *desc;
  if (cd.head_dim != 128) {
    set_error("only head_dim == 128 is supported by the decoder kernels (Qwen3 family)");
    return AHA_ERR_UNSUPPORTED;
  }
  if (cd.hidden_size <= 0 || cd.intermediate_size <= 0 || cd.num_hidden_layers <= 0 || cd.num_attention_heads <= 0 ||
      cd.num_key_value_heads <= 0 || cd.vocab_size <= 0 || cd.n_stop_tokens < 0 || cd.n_stop_tokens > 8 ||
      (cd.arch == AHA_ARCH_QWEN3VL && (cd.vis_spatial_merge_size <= 0 || cd.vis_patch_size <= 0 || cd.vis_num_heads <= 0))) {
    set_error("model_create: sizes must be positive (and at most 8 stop tokens)");   // they divide below: a 0 would be SIGFPE
    return AHA_ERR_INVALID;
  }
  if (cd.num_attention_heads % cd.num_key_value_heads || cd.num_attention_heads / cd.num_key_value_heads > 16) {
    set_error("unsupported GQA group size");
    return AHA_ERR_UNSUPPORTED;
  }
  if (cd.hidden_size % 8 || cd.intermediate_size % 16) {
    set_error("hidden_size must be a multiple of 8 and intermediate_size of 16");
    return AHA_ERR_UNSUPPORTED;
  }
  // the towers' LayerNorm (launch_layernorm_rows) holds a row of at most 8192 elements in 16-byte pieces: a wider or ragged row would be
  // normalised over a prefix only
  auto ln_covers = [](int64_t dim) { return dim > 0 && dim % 8 == 0 && dim <= 8192; };
  if (cd.arch == AHA_ARCH_QWEN3VL && find_tensor(w, nw, "model.visual.patch_embed.proj.weight")) {
    const int64_t m4 = (int64_t)cd.vis_hidden_size * cd.vis_spatial_merge_size * cd.vis_spatial_merge_size;
    if (!ln_covers(cd.vis_hidden_size) || !ln_covers(m4)) {
      set_error("vision tower: hidden_size " + std::to_string(cd.vis_hidden_size) + " and hidden_size * spatial_merge_size^2 = " + std::to_string(m4) +
                " must be multiples of 8 and at most 8192 (the LayerNorm kernel's row)");
      return AHA_ERR_UNSUPPORTED;
    }
  }
  if (cd.arch == AHA_ARCH_QWEN3ASR && !ln_covers(cd.aud_d_model)) {
    set_error("audio tower: d_model " + std::to_string(cd.aud_d_model) + " must be a multiple of 8 and at most 8192 (the LayerNorm kernel's row)");
    return AHA_ERR_UNSUPPORTED;
  }
  AHA_HIP_CHECK(hipSetDevice(ctx->device));
  aha_model* m = new aha_model();
  m->ctx = ctx;
  m->desc = cd;
  m->stream = ctx->stream;
  if (const char* e = getenv("AHA_DECODE_FUSED")) m->decode_fused = atoi(e) != 0;
  int rc = AHA_OK;
  auto fail = [&](int code) {
    model_destroy(m);
    return code;
  };
  // tensor parallelism: from here on m->desc / the locals below hold THIS RANK's share
  const int T = cd.tp_size > 1 ? cd.tp_size : 1, R = T > 1 ? cd.tp_rank : 0;
  if (T > 1 && (R < 0 || R >= T || cd.num_key_value_heads % T || cd.num_attention_heads % T || cd.intermediate_size % (16 * T))) {
    set_error("tp_size must divide num_key_value_heads, num_attention_heads and intermediate_size/16; 0 <= tp_rank < tp_size");
    return fail(AHA_ERR_INVALID);
  }
  m->tp_rank = R;
  m->tp_size = T;
  const int nq_full = cd.num_attention_heads * cd.head_dim, nkv_full = cd.num_key_value_heads * cd.head_dim, I_full = cd.intermediate_size;
  m->desc.num_attention_heads /= T;
  m->desc.num_key_value_heads /= T;
  m->desc.intermediate_size /= T;
  const aha_model_desc& c = m->desc;  // local sizes from here on
  const int H = c.hidden_size, I = I_full / T, d = c.head_dim;
  const int nq = nq_full / T, nkv = nkv_full / T;

  // name prefixes: Qwen3 "model." optional (qwen3/model.rs:105-109); Qwen3-VL "model.language_model." (qwen3vl/model.rs:847-870)
  std::string pre;
  if (c.arch == AHA_ARCH_QWEN3VL) pre = "model.language_model.";
  else if (c.arch == AHA_ARCH_QWEN3ASR) pre = "thinker.model.";  // qwen3_asr/model.rs:318,378
  else pre = find_tensor(w, nw, "model.embed_tokens.weight") ? "model." : "";

  const aha_tensor_view* t = nullptr;
  if ((rc = need(w, nw, pre + "embed_tokens.weight", &t))) return fail(rc);
  if ((rc = upload_tensor(m, t, {c.vocab_size, H}, &m->embed))) return fail(rc);
  // lm_head under tensor parallelism: rank r streams vocab rows [r V/T, (r+1) V/T); the tied
  // case needs no copy (a row window of the embedding table, which every rank holds in full for the gather)
  m->lm_rows = c.vocab_size;
  m->lm_row0 = 0;
  if (T > 1 && c.vocab_size % T == 0) {
    m->lm_rows = c.vocab_size / T;
    m->lm_row0 = R * m->lm_rows;
  }
  if (c.tie_word_embeddings) m->lm_head = (char*)m->embed + (size_t)m->lm_row0 * H * 2;
  else {
    // HF stores lm_head at top level; the reference's Qwen3 (non-VL) branch would look it up under the prefix
    // (qwen3/model.rs:124) -- accept either.
    t = find_tensor(w, nw, c.arch == AHA_ARCH_QWEN3ASR ? "thinker.lm_head.weight" : "lm_head.weight");
    if (!t) t = find_tensor(w, nw, pre + "lm_head.weight");
    if (!t) {
      set_error("missing weight tensor: lm_head.weight");
      return fail(AHA_ERR_MISSING_WEIGHT);
    }
    if (m->lm_rows == c.vocab_size) {
      if ((rc = upload_tensor(m, t, {c.vocab_size, H}, &m->lm_head))) return fail(rc);
    } else {
      if ((rc = dev_alloc(m, (size_t)m->lm_rows * H * 2, &m->lm_head))) return fail(rc);
      if ((rc = upload_block(m, t, c.vocab_size, H, m->lm_row0, m->lm_rows, 0, H, m->lm_head, 0))) return fail(rc);
    }
  }
  if ((rc = need(w, nw, pre + "norm.weight", &t))) return fail(rc);
  if ((rc = upload_tensor(m, t, {H}, &m->final_norm))) return fail(rc);

  m->layers.resize(c.num_hidden_layers);
  for (int li = 0; li < c.num_hidden_layers; ++li) {
    const std::string p = pre + "layers." + std::to_string(li) + ".";
    LayerWeights& L = m->layers[li];
    const aha_tensor_view *tq, *tk, *tv, *tg, *tu;
    if ((rc = need(w, nw, p + "self_attn.q_proj.weight", &tq))) return fail(rc);
    if ((rc = need(w, nw, p + "self_attn.k_proj.weight", &tk))) return fail(rc);
    if ((rc = need(w, nw, p + "self_attn.v_proj.weight", &tv))) return fail(rc);
    if ((rc = dev_alloc(m, (size_t)(nq + 2 * nkv) * H * 2, &L.wqkv))) return fail(rc);
    // column-parallel q/k/v (this rank's heads), row-parallel o_proj (the matching input columns)
    if ((rc = upload_block(m, tq, nq_full, H, (int64_t)R * nq, nq, 0, H, L.wqkv, 0))) return fail(rc);
    if ((rc = upload_block(m, tk, nkv_full, H, (int64_t)R * nkv, nkv, 0, H, L.wqkv, nq))) return fail(rc);
    if ((rc = upload_block(m, tv, nkv_full, H, (int64_t)R * nkv, nkv, 0, H, L.wqkv, nq + nkv))) return fail(rc);
    if ((rc = need(w, nw, p + "self_attn.o_proj.weight", &t))) return fail(rc);
    if ((rc = dev_alloc(m, (size_t)H * nq * 2, &L.wo))) return fail(rc);
    if ((rc = upload_block(m, t, H, nq_full, 0, H, (int64_t)R * nq, nq, L.wo, 0))) return fail(rc);
    // column-parallel gate/up (this rank's intermediate columns), row-parallel down_proj
    if ((rc = need(w, nw, p + "mlp.gate_proj.weight", &tg))) return fail(rc);
    if ((rc = need(w, nw, p + "mlp.up_proj.weight", &tu))) return fail(rc);
    if ((rc = upload_gate_up(m, tg, tu, I_full, (int64_t)R * I, I, H, &L.wgu))) return fail(rc);
    if ((rc = need(w, nw, p + "mlp.down_proj.weight", &t))) return fail(rc);
    if ((rc = dev_alloc(m, (size_t)H * I * 2, &L.wdown))) return fail(rc);
    if ((rc = upload_block(m, t, H, I_full, 0, H, (int64_t)R * I, I, L.wdown, 0))) return fail(rc);
    if ((rc = need(w, nw, p + "input_layernorm.weight", &t))) return fail(rc);
    if ((rc = upload_tensor(m, t, {H}, &L.in_norm))) return fail(rc);
    if ((rc = need(w, nw, p + "post_attention_layernorm.weight", &t))) return fail(rc);
    if ((rc = upload_tensor(m, t, {H}, &L.post_norm))) return fail(rc);
    if ((rc = need(w, nw, p + "self_attn.q_norm.weight", &t))) return fail(rc);
    if ((rc = upload_tensor(m, t, {d}, &L.q_norm))) return fail(rc);
    if ((rc = need(w, nw, p + "self_attn.k_norm.weight", &t))) return fail(rc);
    if ((rc = upload_tensor(m, t, {d}, &L.k_norm))) return fail(rc);
  }

  // rope constants.  inv_freq_i = 1 / theta^(2i/d) in f32 with powf (rope.rs:7-13); the M-RoPE axis of slot i follows
  // apply_interleaved_mrope (rope.rs:454-476): H overwrites i = 1,4,.. < 3*sec[1], W overwrites i = 2,5,.. < 3*sec[2].
  {
    std::vector<float> inv(d / 2);
    std::vector<int32_t> axis(d / 2, 0);
    for (int i = 0; i < d / 2; ++i) {
      inv[i] = 1.0f / powf(c.rope_theta, (float)(2 * i) / (float)d);
      if (c.mrope_section[0] + c.mrope_section[1] + c.mrope_section[2] > 0) {
        if (i % 3 == 1 && i < 3 * c.mrope_section[1]) axis[i] = 1;
        if (i % 3 == 2 && i < 3 * c.mrope_section[2]) axis[i] = 2;
      }
    }
    void* p;
    if ((rc = dev_alloc(m, inv.size() * 4, &p))) return fail(rc);
    m->d_inv_freq = (float*)p;
    if ((rc = dev_alloc(m, axis.size() * 4, &p))) return fail(rc);
    m->d_axis_map = (int32_t*)p;
    hipMemcpy(m->d_inv_freq, inv.data(), inv.size() * 4, hipMemcpyHostToDevice);
    hipMemcpy(m->d_axis_map, axis.data(), axis.size() * 4, hipMemcpyHostToDevice);
    // `attn_weights * scaling` is a Candle affine op: the f64 scalar is cast to the tensor dtype first [unverified],
    // so the effective scale is bf16(1/sqrt(d)) (modules.rs:476,783; oracle/qwen3.py attn_scale)
    const float s = 1.0f / sqrtf((float)d);
    uint32_t u;
    memcpy(&u, &s, 4);
    u += 0x7fffu + ((u >> 16) & 1u);
    u &= 0xffff0000u;
    memcpy(&m->attn_scale, &u, 4);
  }

  // KV pages
  m->page_bytes = (uint64_t)2 * c.num_key_value_heads * KV_PAGE_TOKENS * d * 2;
  m->pages_per_slab = 64;
  m->layer_stride = m->pages_per_slab * m->page_bytes;
  if (c.kv_reserve_tokens > 0) {
    if ((rc = model_ensure_pages(m, c.kv_reserve_tokens))) return fail(rc);
    model_clear_cache(m);
  }

  // step state + decode scratch
  void* p;
  if ((rc = dev_alloc(m, sizeof(StepState), &p, true))) return fail(rc);
  m->d_state = (StepState*)p;
  if (hipHostMalloc((void**)&m->h_state, sizeof(StepState)) != hipSuccess ||
      hipHostMalloc((void**)&m->h_logits, (size_t)c.vocab_size * 4) != hipSuccess) {
    set_error("model_create: pinned host allocation failed");
    return fail(AHA_ERR_HIP);
  }
  if (hipHostMalloc((void**)&m->h_ring, (RING_CAP + 16) * 4, hipHostMallocMapped | hipHostMallocCoherent) != hipSuccess ||
      hipHostGetDevicePointer((void**)&m->h_ring_dev, m->h_ring, 0) != hipSuccess) {
    set_error("hipHostMalloc (decode token ring) failed");
    return fail(AHA_ERR_OOM);
  }
  memset(m->h_ring, 0, (RING_CAP + 16) * 4);
  m->h_done = m->h_ring + RING_CAP;
  m->h_done_dev = m->h_ring_dev + RING_CAP;
  m->token_log_cap = 1 << 16;
  if ((rc = dev_alloc(m, m->token_log_cap * 4, &p))) return fail(rc);
  m->d_token_log = (uint32_t*)p;
  if ((rc = dev_alloc(m, (size_t)H * 2, &m->d_x))) return fail(rc);
  if ((rc = dev_alloc(m, (size_t)(nq + 2 * nkv) * 2, &m->d_qkv))) return fail(rc);
  if ((rc = dev_alloc(m, (size_t)nq * 2, &m->d_q))) return fail(rc);
  if ((rc = dev_alloc(m, (size_t)nq * 2, &m->d_attn))) return fail(rc);
  if ((rc = dev_alloc(m, (size_t)I * 2, &m->d_act))) return fail(rc);
  if ((rc = dev_alloc(m, (size_t)H * 2, &m->d_hlast, true))) return fail(rc);
  if ((rc = dev_alloc(m, (size_t)H * 4, &p))) return fail(rc);
  m->d_partial = (float*)p;
  if ((rc = dev_alloc(m, (size_t)c.vocab_size * 4, &p))) return fail(rc);
  m->d_logits = (float*)p;
  const int nt = std::max(std::max(std::max(gemv_num_tiles(c.vocab_size, H), gemv_mxfp8_num_tiles(c.vocab_size, H)), gemv_mxfp4_num_tiles(c.vocab_size, H)), std::max(gemv_pk13_num_tiles(c.vocab_size, H), 512));
  if ((rc = dev_alloc(m, (size_t)nt * 4, &p))) return fail(rc);
  m->d_blk_max = (float*)p;
  if ((rc = dev_alloc(m, (size_t)nt * 4, &p))) return fail(rc);
  m->d_blk_idx = (uint32_t*)p;
  if ((rc = dev_alloc(m, (size_t)m->max_nsplit * 4 * c.num_attention_heads * d * 4, &p))) return fail(rc);
  m->d_part_o = (float*)p;
  if ((rc = dev_alloc(m, (size_t)m->max_nsplit * 4 * c.num_attention_heads * 2 * 4, &p))) return fail(rc);
  m->d_part_ml = (float*)p;
  if ((rc = dev_alloc(m, 128 * 4, &p, true))) return fail(rc);
  m->d_rope = (float*)p;

  // split-arrival counters of the fused decode attention (kernels.h DECODE_SYNC_BYTES): zeroed once, only ever grow; all
  // accesses are agent-scope atomics
  if ((rc = dev_alloc(m, DECODE_SYNC_BYTES, &p, true))) return fail(rc);
  m->d_bar = (unsigned*)p;
  // per-tile arrival counters of the persistent prefill GEMM (kernels_gemm_sk.hip): zeroed once, every launch leaves them zero
  if ((rc = dev_alloc(m, SK_MAX_COUNTERS * 4, &m->d_sk_ctrs, true))) return fail(rc);

  if (c.arch == AHA_ARCH_QWEN3VL) {
    if ((rc = vision_create(m, w, nw))) return fail(rc);
  }
  if (c.arch == AHA_ARCH_QWEN3ASR) {
    if ((rc = audio_create(m, w, nw))) return fail(rc);
  }
  if ((rc = model_pack_weights(m))) return fail(rc);
  if (hipStreamSynchronize(m->stream) != hipSuccess) {
    set_error(std::string("model_create: ") + hipGetErrorString(hipGetLastError()));
    return fail(AHA_ERR_HIP);
  }
  *out = m;
  return AHA_OK;
}

void model_destroy(aha_model* m) {
  if (!m) return;
  if (m->engine) engine_destroy(m->engine);   // an engine left open goes with its model (its handle is dead afterwards)
  hipStreamSynchronize(m->stream);
  for (auto& r : m->prof) { hipEventDestroy(r.e0); hipEventDestroy(r.e1); }
  vision_destroy(m);
  audio_destroy(m);
  tp_destroy(m);
  model_free_packed(m, "freed");
  for (void* p : m->owned) hipFree(p);
  for (void* p : m->pf_owned) hipFree(p);
  if (m->p_pass_tab) hipFree(m->p_pass_tab);
  if (m->p_pool) hipFree(m->p_pool);
  if (m->h_pass_stage) hipHostFree(m->h_pass_stage);
  for (void* p : m->slabs) hipFree(p);
  if (m->d_page_ptrs) hipFree(m->d_page_ptrs);
  if (m->h_state) hipHostFree(m->h_state);
  if (m->h_ring) hipHostFree(m->h_ring);
  if (m->h_logits) hipHostFree(m->h_logits);
  if (m->h_samp) hipHostFree(m->h_samp);
  delete m;
}

// ---------------------------------------------------------------------------------------------------------------
static int ensure_prefill_scratch(aha_model* m, size_t S) {
  if (S <= m->pf_cap) return AHA_OK;
  AHA_HIP_CHECK(hipStreamSynchronize(m->stream));
  for (void* p : m->pf_owned) hipFree(p);
  m->pf_owned.clear();
  m->pf_cap = 0;
  const aha_model_desc& c = m->desc;
  const size_t cap = (S + 255) / 256 * 256;
  const size_t H = c.hidden_size, I = c.intermediate_size, nq = (size_t)c.num_attention_heads * c.head_dim,
               nkv = (size_t)c.num_key_value_heads * c.head_dim;
  auto al = [&](size_t bytes, void** out) -> int {
    void* p = nullptr;
    hipError_t e = hipMalloc(&p, bytes);
    if (e != hipSuccess) {
      set_error(std::string("prefill scratch hipMalloc failed: ") + hipGetErrorString(e));
      return e == hipErrorOutOfMemory ? AHA_ERR_OOM : AHA_ERR_HIP;
    }
    m->pf_owned.push_back(p);
    *out = p;
    return AHA_OK;
  };
  int rc;
  if ((rc = al(cap * 4, (void**)&m->p_ids))) return rc;
  if ((rc = al(cap * 3 * 4, (void**)&m->p_pos))) return rc;
  if ((rc = al(cap * 128 * 2, &m->p_rope))) return rc;
  if ((rc = al(cap * H * 2, &m->p_x))) return rc;
  if ((rc = al((cap + 64) * H * 2, &m->p_h))) return rc;   // + padding rows of the sequence-parallel all-gather (T * ceil(S/T) >= S)
  if ((rc = al(cap * (nq + 2 * nkv) * 2, &m->p_qkv))) return rc;
  if ((rc = al(cap * nq * 2, &m->p_q))) return rc;
  if ((rc = al(cap * nq * 2, &m->p_attn))) return rc;
  if ((rc = al(cap * I * 2, &m->p_act))) return rc;
  if (m->tp_size > 1 && (rc = al((cap + 64) * H * 4, (void**)&m->p_partial))) return rc;
  if (m->tp_size > 1 && (rc = al((cap + 64) * H * 2, &m->p_hstage))) return rc;
  if (m->cp_size > 1) {   // one layer's K / V of every rank's pages: cp_size x (max pages of a rank) x kv heads x (K | V) 16-KB blocks
    const size_t pages = cap / KV_PAGE_TOKENS + 1, pmax = pages / m->cp_size + 4;
    m->cp_stage_bytes = std::max((size_t)m->cp_size * pmax * nkv / 128 * 2 * KV_BLOCK_BYTES, (size_t)m->cp_size * H * 2);
    if ((rc = al(m->cp_stage_bytes, &m->p_cp_stage))) return rc;
  }   // chunked all-gather: [chunk][rank][rows of the chunk]
  m->gemm_ws_bytes = std::min((size_t)12 * cap * H * 4, (size_t)1 << 30);  // split-K slabs (up to 8 slices of an N = hidden GEMM, 6 of the qkv one)
  if ((rc = al(m->gemm_ws_bytes, &m->p_gemm_ws))) return rc;
  m->pf_cap = cap;
  return AHA_OK;
}

static int push_state(aha_model* m, uint32_t token, const int64_t pos[3], size_t kv_start, size_t kv_len) {
  StepState* s = m->h_state;
  s->token = token;
  for (int i = 0; i < 3; ++i) s->pos[i] = (int32_t)pos[i];
  s->kv_start = (int32_t)kv_start;
  s->kv_len = (int32_t)kv_len;
  s->next_token = 0;
  s->step = 0;
  AHA_HIP_CHECK(hipMemcpyAsync(m->d_state, s, sizeof(StepState), hipMemcpyHostToDevice, m->stream));
  return AHA_OK;
}

static void gemv_row_parallel(aha_model* m, GemvArgs g);

// One batch-1 matvec of the single-sequence path (g.N output rows: I for GEMV_SILU_MUL).  A matrix with an MXFP8 copy is read from it
// where the plan takes the shape (gemv_mxfp8_by_plan: the matrices for which FP8 measured faster; the two kernels give the same bits, so
// the choice is invisible in the output; aha_hip_debug_fp8_single overrides it either way) -- sharded models never have a copy.
// Profile class gemv_fp8 at 1.03125 bytes per weight, gemv at 2; act_bytes: the activation traffic.  An MXFP4 copy goes the same way
// through a switch, a plan and a class of its own: aha_hip_debug_fp4_single, gemv_mxfp4_by_plan, gemv_fp4 at 0.53125 bytes per weight.
static bool fp8_single(const aha_model* m, const WQuant& wq, int rows, int K, GemvEpi epi) {
  return wq.q != nullptr && m->wq_format == AHA_WQ_MXFP8_E4M3 && m->tp_size <= 1 && (m->fp8_single == 2 || (m->fp8_single == 1 && gemv_mxfp8_by_plan(rows, K, epi)));
}
static bool fp4_single(const aha_model* m, const WQuant& wq, int rows, int K, GemvEpi epi) {
  return wq.q != nullptr && m->wq_format == AHA_WQ_MXFP4_E2M1 && m->tp_size <= 1 && (m->fp4_single == 2 || (m->fp4_single == 1 && gemv_mxfp4_by_plan(rows, K, epi)));
}
// An exact 13-bit copy (a bf16 model only: quantising frees them) goes the same way through aha_hip_debug_pk13_single and gemv_pk13_by_plan,
// and stays in class gemv with the 1.625 bytes per weight it reads: the same matrix, the same bits.
static bool pk13_single(const aha_model* m, const Pk13Copy& pk, int rows, int K, GemvEpi epi) {
  return pk.p != nullptr && m->wq_format == AHA_WQ_NONE && m->tp_size <= 1 && gemv_pk13_shape_ok(rows, K) &&
         (m->pk13_single == 2 || (m->pk13_single == 1 && gemv_pk13_by_plan(rows, K, epi)));
}
static void decode_gemv(aha_model* m, const GemvArgs& g, GemvEpi epi, const WQuant& wq, const Pk13Copy& pk, double act_bytes) {
  const double weights = (epi == GEMV_SILU_MUL ? 2.0 : 1.0) * g.N * g.K;
  const int rows = (epi == GEMV_SILU_MUL ? 2 : 1) * g.N;
  const bool fp8 = fp8_single(m, wq, rows, g.K, epi), fp4 = fp4_single(m, wq, rows, g.K, epi), p13 = pk13_single(m, pk, rows, g.K, epi);
  ProfScope ps(m, fp8 ? "gemv_fp8" : fp4 ? "gemv_fp4" : "gemv", weights * (fp8 ? 1.03125 : fp4 ? 0.53125 : p13 ? 1.625 : 2.0) + act_bytes, 2.0 * weights);
  if (fp8) launch_gemv_mxfp8(g, wq.q, wq.scales, epi, m->stream);
  else if (fp4) launch_gemv_mxfp4(g, wq.q, wq.scales, epi, m->stream);
  else if (p13) {
    GemvArgs gw = g;
    gw.W = pk.w;   // read only for the exception rows
    launch_gemv_pk13(gw, pk.p, pk.bh, pk.rows, pk.nrows, epi, m->stream);
  }
  else if (epi == GEMV_RESIDUAL) gemv_row_parallel(m, g);
  else launch_gemv(g, epi, m->stream);
}
// (max, index) partials the lm_head matvec of enqueue_lm_head writes: the grid of the kernel that runs
static int lm_head_partials(const aha_model* m) {
  const int N = m->lm_rows, K = m->desc.hidden_size;
  if (fp8_single(m, m->q_lm_head, N, K, GEMV_LOGITS)) return gemv_mxfp8_num_tiles(N, K);
  if (fp4_single(m, m->q_lm_head, N, K, GEMV_LOGITS)) return gemv_mxfp4_num_tiles(N, K);
  if (pk13_single(m, m->p_lm_head, N, K, GEMV_LOGITS)) return gemv_pk13_num_tiles(N, K);
  return gemv_num_tiles(N, K);
}

// final RMSNorm (qwen3/model.rs:186) fused into the lm_head matvec of the LAST position only (model.rs:187,142),
// f32 logits + argmax partials -> d_state->next_token
static void enqueue_lm_head(aha_model* m, const void* x_last, bool argmax = true) {
  const aha_model_desc& c = m->desc;
  GemvArgs g{};
  g.W = m->lm_head;
  g.x = x_last;
  g.norm_w = m->final_norm;
  g.eps = c.rms_norm_eps;
  g.N = m->lm_rows;
  g.K = c.hidden_size;
  g.y_f32 = m->d_logits + m->lm_row0;
  g.blk_max = m->d_blk_max;
  g.blk_idx = m->d_blk_idx;
  g.h_out = m->d_hlast;
  decode_gemv(m, g, GEMV_LOGITS, m->q_lm_head, m->p_lm_head, c.hidden_size * 2 + m->lm_rows * 4.0);
  if (!argmax) return;   // the caller reduces the partials itself (step_tail_kernel)
  ProfScope ps(m, "argmax", 0, 0);
  const int ntiles = lm_head_partials(m);
  if (m->lm_rows == c.vocab_size) {
    launch_argmax_partials(m->d_blk_max, m->d_blk_idx, ntiles, &m->d_state->next_token, m->stream);
    return;
  }
  // vocab-parallel: each rank contributes its (max, global index) pair to a zeroed 2T-float vector; the all-reduce (sum)
  // is then an all-gather; the pick keeps the smallest index among equal maxima (candle argmax = first maximal index)
  launch_argmax_pair(m->d_blk_max, m->d_blk_idx, ntiles, m->lm_row0, m->d_partial, m->tp_rank, m->tp_size, m->stream);
  const int rc = model_allreduce(m, m->d_partial, (size_t)2 * m->tp_size);
  if (rc && !m->async_rc) m->async_rc = rc;
  launch_argmax_pick(m->d_partial, m->tp_size, &m->d_state->next_token, m->stream);
}

static void gemv_trace_dump(aha_model* m);

// vocab-parallel lm_head: every rank zeroes the slices it does not own and the all-reduce assembles the full vector
static int assemble_logits(aha_model* m) {
  const aha_model_desc& c = m->desc;
  if (m->lm_rows == c.vocab_size || m->logits_assembled) return AHA_OK;
  if (m->lm_row0 > 0) AHA_HIP_CHECK(hipMemsetAsync(m->d_logits, 0, (size_t)m->lm_row0 * 4, m->stream));
  const int tail0 = m->lm_row0 + m->lm_rows;
  if (tail0 < c.vocab_size) AHA_HIP_CHECK(hipMemsetAsync(m->d_logits + tail0, 0, (size_t)(c.vocab_size - tail0) * 4, m->stream));
  const int rc = model_allreduce(m, m->d_logits, (size_t)c.vocab_size);
  if (rc) return rc;
  m->logits_assembled = true;
  return AHA_OK;
}

static int fetch_outputs(aha_model* m, float* logits_out, uint32_t* argmax_out) {
  const aha_model_desc& c = m->desc;
  m->have_logits = true;
  m->logits_assembled = false;
  if (logits_out) {
    const int rc = assemble_logits(m);
    if (rc) return rc;
  }
  if (logits_out) AHA_HIP_CHECK(hipMemcpyAsync(m->h_logits, m->d_logits, (size_t)c.vocab_size * 4, hipMemcpyDeviceToHost, m->stream));
  AHA_HIP_CHECK(hipMemcpyAsync(&m->h_state->next_token, &m->d_state->next_token, 4, hipMemcpyDeviceToHost, m->stream));
  AHA_HIP_CHECK(hipStreamSynchronize(m->stream));
  if (m->d_gemv_trace) gemv_trace_dump(m);
  if (m->d_attn_trace) {
    const int L = m->desc.num_hidden_layers;
    std::vector<unsigned long long> t((size_t)L * 12);
    if (hipMemcpy(t.data(), m->d_attn_trace, t.size() * 8, hipMemcpyDeviceToHost) == hipSuccess) {
      for (int b = 0; b < 2; ++b) {
        double v[5] = {};
        int n = 0;
        for (int li = 1; li < L; ++li) {
          const unsigned long long* p = t.data() + (size_t)li * 12 + b * 6;
          if (p[0] == 0 || p[4] == 0) continue;
          for (int k = 0; k < 5; ++k) v[k] += (p[k + 1] > p[k] ? (double)(p[k + 1] - p[k]) : 0.0) * 0.01;
          ++n;
        }
        if (n) fprintf(stderr, "[attn trace] block %d: prologue %.2f | pages %.2f | merge+publish %.2f | arrive %.2f | final merge %.2f us\n", b, v[0] / n, v[1] / n, v[2] / n, v[3] / n, v[4] / n);
      }
      // the stamps are absolute: who started first, and when each block's arrival was known, counted from the earlier start
      double dstart = 0.0, arr[2] = {};
      int n = 0;
      for (int li = 1; li < L; ++li) {
        const unsigned long long* p = t.data() + (size_t)li * 12;
        if (p[0] == 0 || p[4] == 0 || p[6] == 0 || p[10] == 0) continue;
        const unsigned long long t0 = std::min(p[0], p[6]);
        dstart += ((double)p[6] - (double)p[0]) * 0.01;
        arr[0] += (double)(p[4] - t0) * 0.01;
        arr[1] += (double)(p[10] - t0) * 0.01;
        ++n;
      }
      if (n) fprintf(stderr, "[attn trace] start of block 1 - start of block 0 %+.2f | arrival after the earlier start: block 0 %.2f | block 1 %.2f us\n", dstart / n, arr[0] / n, arr[1] / n);
    }
  }
  if (logits_out) memcpy(logits_out, m->h_logits, (size_t)c.vocab_size * 4);
  if (argmax_out) *argmax_out = m->h_state->next_token;
  return AHA_OK;
}


// ---- tensor-parallel seam ---------------------------------------------------------------------------------------------
// Row-parallel projections (o_proj, down_proj): with tp_size > 1 each rank holds a K slice, produces un-rounded f32
// partial sums, the partials are all-reduced, and only then does the reference's rounding chain run
// (Linear output -> bf16, + residual -> bf16).  Summing in f32 keeps the result equal to the single-GPU one up to f32
// summation order.
int model_allreduce(aha_model* m, float* buf, size_t count) {
  if (m->tp_size <= 1) return AHA_OK;
  ProfScope ps(m, "allreduce", (double)count * 4, 0);
  if (m->rccl_comm) return rccl_allreduce(m, buf, count);
  if (!m->allreduce_cb) {
    set_error("tp_size > 1 but no all-reduce was installed (aha_hip_set_allreduce / aha_hip_tp_init_rccl)");
    return AHA_ERR_STATE;
  }
  AHA_HIP_CHECK(hipStreamSynchronize(m->stream));
  if (m->allreduce_cb(buf, count, m->allreduce_user) != 0) {
    set_error("all-reduce callback failed");
    return AHA_ERR_STATE;
  }
  return AHA_OK;
}
// Sequence-parallel prefill (include/aha_hip.h aha_hip_set_seq_parallel): in-place reduce-scatter of f32 partial sums over
// row slices, in-place all-gather of bf16 rows.  RCCL communicator if the library owns one, else the host callbacks.
static bool seq_parallel_on(const aha_model* m) {
  static const bool env_on = [] { const char* e = getenv("AHA_TP_SP"); return e ? atoi(e) != 0 : true; }();
  return env_on && m->tp_size > 1 && (m->rccl_comm || (m->reduce_scatter_cb && m->all_gather_cb));
}
static int model_reduce_scatter(aha_model* m, float* buf, size_t count_per_rank) {
  ProfScope ps(m, "reduce_scatter", (double)count_per_rank * m->tp_size * 4, 0);
  if (m->rccl_comm) return rccl_reduce_scatter(m, buf, count_per_rank);
  AHA_HIP_CHECK(hipStreamSynchronize(m->stream));
  if (m->reduce_scatter_cb(buf, count_per_rank, m->sp_user) != 0) {
    set_error("reduce-scatter callback failed");
    return AHA_ERR_STATE;
  }
  return AHA_OK;
}
static int model_all_gather(aha_model* m, void* buf, size_t bytes_per_rank) {
  ProfScope ps(m, "all_gather", (double)bytes_per_rank * m->tp_size, 0);
  if (m->rccl_comm) return rccl_all_gather(m, buf, bytes_per_rank);
  AHA_HIP_CHECK(hipStreamSynchronize(m->stream));
  if (m->all_gather_cb(buf, bytes_per_rank, m->sp_user) != 0) {
    set_error("all-gather callback failed");
    return AHA_ERR_STATE;
  }
  return AHA_OK;
}
static void gemv_row_parallel(aha_model* m, GemvArgs g) {
  if (m->tp_size <= 1) {
    launch_gemv(g, GEMV_RESIDUAL, m->stream);
    return;
  }
  g.y_f32 = m->d_partial;
  launch_gemv(g, GEMV_PARTIAL_F32, m->stream);
  const int rc = model_allreduce(m, m->d_partial, (size_t)g.N);
  if (rc && !m->async_rc) m->async_rc = rc;
  launch_residual_add_f32(g.y, m->d_partial, g.N, m->stream);
}
// rows_per_rank > 0 selects the sequence-parallel form: the partial sums are reduce-scattered over row slices and only this
// rank's rows [tp_rank * rows_per_rank, ...) of the residual stream are updated (the caller all-gathers the NORMALISED rows).
// Column chunks of a sequence-parallel row-parallel projection ("chunk ... to overlap with GEMMs").  The
// projection is cut along N (output columns) -- NOT along the rows, so that rank r keeps owning the contiguous rows
// [r * rows_per_rank, ...) -- into `nch` GEMMs whose f32 partial sums land in separate (rows_pad x N / nch) blocks; the reduce-scatter
// of block j (count_per_rank = rows_per_rank * N / nch: rank r receives its rows of that column block) runs on the communication
// stream while the matrix cores compute block j + 1.  Same sums in the same order as the unchunked form: every output element is one
// K-sum and one sum over ranks either way (tests/test_tp_gpu.py compares both with the all-reduce path bit for bit).  At cfg 5
// (S = 40 980, T = 8) a projection's reduce-scatter moves 7/8 x 671 MB per rank against ~1.2 ms of GEMM per 1024-column block.
static int tp_overlap_chunks(const aha_model* m, const GemmArgs& g) {
  const char* e = getenv("AHA_TP_OVERLAP_CHUNKS");
  const char* er = getenv("AHA_TP_OVERLAP_MIN_ROWS");
  int nch = e ? atoi(e) : 4;
  const int min_rows = er ? atoi(er) : 2048;
  if (nch > 8) nch = 8;
  if (nch <= 1 || g.M < min_rows) return 1;
  while (nch > 1 && (g.N % nch != 0 || (g.N / nch) % 256 != 0)) --nch;
  return nch;
}
static int ensure_comm_stream(aha_model* m) {
  if (m->comm_stream) return AHA_OK;
  // RCCL's kernels run on the communication stream BESIDE the next column block's GEMM.  A grid of one-tile blocks fills every CU with
  // a 512-register wave per SIMD + 128 KiB of LDS, so nothing else can be placed until a block retires; the persistent GEMM kernel takes
  // a worker count instead (kernels_gemm_sk.hip).  Leave 16 CUs (two per XCD) to the collective unless the caller chose a number
  // (aha_hip_set_gemm_reserved_cus / AHA_GEMM_RESERVE_CUS); process-wide while this model's communicator lives.
  // The setting is restored when this model's communicator is torn down (tp_rccl.hip): un-sharded models and op-level GEMMs of the same
  // process are planned on all CUs again from then on (round-4 advisor).
  // (reference-counted: several models of one process may each hold a share, kernels_gemm_sk.hip acquire_gemm_cu_reservation)
  m->reserved_cus_set = acquire_gemm_cu_reservation(16);
  int lo = 0, hi = 0;
  AHA_HIP_CHECK(hipDeviceGetStreamPriorityRange(&lo, &hi));   // (numerically lowest = highest priority)
  AHA_HIP_CHECK(hipStreamCreateWithPriority(&m->comm_stream, hipStreamNonBlocking, hi));
  for (auto& ev : m->ev_gemm) AHA_HIP_CHECK(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
  for (auto& ev : m->ev_ag) AHA_HIP_CHECK(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
  AHA_HIP_CHECK(hipEventCreateWithFlags(&m->ev_comm, hipEventDisableTiming));
  return AHA_OK;
}

// rows_per_rank > 0 selects the sequence-parallel form: the partial sums are reduce-scattered over row slices and only this
// rank's rows [tp_rank * rows_per_rank, ...) of the residual stream are updated (the caller all-gathers the NORMALISED rows).
static int gemm_row_parallel(aha_model* m, GemmArgs g, int rows_per_rank = 0) {
  if (m->tp_size <= 1) {
    launch_gemm(g, m->stream);
    return AHA_OK;
  }
  void* xres = g.C;
  const int nch = rows_per_rank > 0 ? tp_overlap_chunks(m, g) : 1;
  if (nch > 1) {
    const int N = g.N, Nc = N / nch;
    const size_t rows_pad = (size_t)rows_per_rank * m->tp_size;
    const bool on_comm_stream = m->rccl_comm != nullptr;   // host-callback seam (tests): the callback synchronises, no overlap to set up
    int rc;
    if (on_comm_stream && (rc = ensure_comm_stream(m))) return rc;
    // an error inside the loop must not leave the compute stream free to overwrite p_partial while the communication stream still
    // reads it: join the streams before returning
    auto fail = [&](int code) {
      if (on_comm_stream && hipEventRecord(m->ev_comm, m->comm_stream) == hipSuccess) (void)hipStreamWaitEvent(m->stream, m->ev_comm, 0);
      return code;
    };
    for (int j = 0; j < nch; ++j) {
      GemmArgs gj = g;
      gj.W = (const bf16_t*)g.W + (int64_t)j * Nc * g.ldw;
      gj.C = m->p_partial + (size_t)j * rows_pad * Nc;
      gj.N = Nc;
      gj.ldc = Nc;
      gj.residual = nullptr;
      gj.norm_w = nullptr;
      gj.act = ACT_PARTIAL_F32;
      launch_gemm(gj, m->stream);
      float* bj = m->p_partial + (size_t)j * rows_pad * Nc;
      if (on_comm_stream) {
        // (no ProfScope here: it would time m->stream, and this collective runs on the communication stream; the wait for it is
        // what the compute stream sees -- the "rs_wait" scope below)
        if (hipEventRecord(m->ev_gemm[j], m->stream) != hipSuccess || hipStreamWaitEvent(m->comm_stream, m->ev_gemm[j], 0) != hipSuccess) {
          set_error("gemm_row_parallel: event hand-off to the communication stream failed");
          return fail(AHA_ERR_HIP);
        }
        if ((rc = rccl_reduce_scatter(m, bj, (size_t)rows_per_rank * Nc, m->comm_stream))) return fail(rc);
      } else if ((rc = model_reduce_scatter(m, bj, (size_t)rows_per_rank * Nc))) {
        return rc;
      }
    }
    if (on_comm_stream) {
      ProfScope ps(m, "rs_wait", (double)rows_pad * N * 4, 0);   // what the compute stream waits for the overlapped reduce-scatters
      AHA_HIP_CHECK(hipEventRecord(m->ev_comm, m->comm_stream));
      AHA_HIP_CHECK(hipStreamWaitEvent(m->stream, m->ev_comm, 0));
    }
    const int64_t r0 = (int64_t)m->tp_rank * rows_per_rank, r1 = std::min<int64_t>(g.M, r0 + rows_per_rank);
    for (int j = 0; j < nch && r1 > r0; ++j)
      launch_residual_add_f32_cols((char*)xres + (r0 * N + (int64_t)j * Nc) * 2, N, m->p_partial + (size_t)j * rows_pad * Nc + r0 * Nc, Nc, r1 - r0,
                                   Nc, m->stream);
    return AHA_OK;
  }
  g.C = m->p_partial;
  g.residual = nullptr;
  g.act = ACT_PARTIAL_F32;
  launch_gemm(g, m->stream);
  if (rows_per_rank > 0) {
    int rc = model_reduce_scatter(m, m->p_partial, (size_t)rows_per_rank * g.N);
    if (rc) return rc;
    const int64_t r0 = (int64_t)m->tp_rank * rows_per_rank, r1 = std::min<int64_t>(g.M, r0 + rows_per_rank);
    if (r1 > r0)
      launch_residual_add_f32((char*)xres + r0 * g.N * 2, m->p_partial + r0 * g.N, (r1 - r0) * g.N, m->stream);
    return AHA_OK;
  }
  int rc = model_allreduce(m, m->p_partial, (size_t)g.M * g.N);
  if (rc) return rc;
  launch_residual_add_f32(xres, m->p_partial, (int64_t)g.M * g.N, m->stream);
  return AHA_OK;
}
// RMSNorm of the prefill rows into p_h.  Sequence-parallel: each rank normalises its own row slice and the bf16 rows are
// all-gathered (the slices are the only valid rows of the residual stream on their rank).
static int prefill_norm(aha_model* m, const void* w, int S, int rows_per_rank) {
  const aha_model_desc& c = m->desc;
  const int H = c.hidden_size;
  if (rows_per_rank <= 0) {
    ProfScope ps(m, "elem", (double)S * H * 4, 0);
    launch_rmsnorm_rows(m->p_x, w, m->p_h, S, H, H, H, c.rms_norm_eps, m->stream);
    return AHA_OK;
  }
  const int64_t r0 = (int64_t)m->tp_rank * rows_per_rank, r1 = std::min<int64_t>(S, r0 + rows_per_rank);
  if (r1 > r0) {
    ProfScope ps(m, "elem", (double)(r1 - r0) * H * 4, 0);
    launch_rmsnorm_rows((const char*)m->p_x + r0 * H * 2, w, (char*)m->p_h + r0 * H * 2, r1 - r0, H, H, H, c.rms_norm_eps, m->stream);
  }
  return model_all_gather(m, m->p_h, (size_t)rows_per_rank * H * 2);
}

// Sequence-parallel column-parallel projection with the all-gather of its input in row chunks, overlapped with the GEMM (round 4; the
// round-3 verdict: "the all-gather of the normalised rows is still one serial call in front of each column-parallel GEMM").
// Every rank's row slice [r * spr, + spr) is cut at the same offsets into chunks of w rows (a multiple of 256: whole row tiles); chunk c
// of all ranks is gathered into its own block of the staging buffer, laid out [rank][rows of the chunk] as ncclAllGather delivers it, on
// the communication stream, while the matrix cores run chunk c - 1: ONE grouped GEMM launch per chunk (launch_gemm_grouped: T row
// segments of the staging block -> the token-order rows r * spr + off .. of the output).  Rows are independent in a GEMM, so every
// output element is the same K-ordered sum as in the unchunked form (tests/test_tp_gpu.py: bit-identical logits and KV).
// cfg 5 on 8 GPUs: the gather moves 7/8 x 336 MB per rank in front of 0.25 ms (qkv) / 0.95 ms (gate+up) of GEMM per rank.
static int tp_ag_chunk_rows(const aha_model* m, int S, int spr) {
  const char* e = getenv("AHA_TP_AG_CHUNKS");
  const char* er = getenv("AHA_TP_AG_MIN_ROWS");
  const int nch = std::min(e ? atoi(e) : 4, 8), min_rows = er ? atoi(er) : 4096;
  if (nch <= 1 || S < min_rows) return 0;
  const int w = ((spr + nch - 1) / nch + 255) / 256 * 256;
  return w < spr ? w : 0;   // one chunk: nothing to overlap
}
static int norm_gather_gemm(aha_model* m, const void* norm_w, const GemmArgs& g, int S, int spr) {
  const aha_model_desc& c = m->desc;
  const int H = c.hidden_size, T = m->tp_size;
  const int w = spr > 0 ? tp_ag_chunk_rows(m, S, spr) : 0;
  if (w <= 0) {
    int rc = prefill_norm(m, norm_w, S, spr);
    if (rc) return rc;
    ProfScope ps(m, "gemm", ((double)g.M * g.K + (double)g.N * g.K + (double)g.M * g.ldc) * 2, 2.0 * g.M * g.N * g.K);
    launch_gemm(g, m->stream);
    return AHA_OK;
  }
  const int64_t r0 = (int64_t)m->tp_rank * spr, r1 = std::min<int64_t>(S, r0 + spr);
  if (r1 > r0) {
    ProfScope ps(m, "elem", (double)(r1 - r0) * H * 4, 0);
    launch_rmsnorm_rows((const char*)m->p_x + r0 * H * 2, norm_w, (char*)m->p_h + r0 * H * 2, r1 - r0, H, H, H, c.rms_norm_eps, m->stream);
  }
  const bool on_comm = m->rccl_comm != nullptr;   // host-callback seam (tests): the callback synchronises, nothing to overlap
  int rc;
  if (on_comm) {
    if ((rc = ensure_comm_stream(m))) return rc;
    AHA_HIP_CHECK(hipEventRecord(m->ev_comm, m->stream));            // the normalised rows are ready
    AHA_HIP_CHECK(hipStreamWaitEvent(m->comm_stream, m->ev_comm, 0));
  }
  const int nch = (spr + w - 1) / w;
  auto join = [&](int code) {   // on an error: the compute stream must not run ahead of collectives still reading / writing the staging
    if (on_comm && hipEventRecord(m->ev_comm, m->comm_stream) == hipSuccess) (void)hipStreamWaitEvent(m->stream, m->ev_comm, 0);
    return code;
  };
  auto gather = [&](int ci) -> int {
    const int off = ci * w, wc = std::min(w, spr - off);
    char* stage = (char*)m->p_hstage + (size_t)T * off * H * 2;
    const size_t bytes = (size_t)wc * H * 2;
    // this rank's rows of the chunk into its slot (rows past the end of the sequence -- the last rank's padding -- carry whatever the
    // buffer holds: their outputs are clipped by the GEMM)
    hipStream_t cs = on_comm ? m->comm_stream : m->stream;
    AHA_HIP_CHECK(hipMemcpyAsync(stage + (size_t)m->tp_rank * bytes, (const char*)m->p_h + (r0 + off) * H * 2, bytes, hipMemcpyDeviceToDevice, cs));
    if (on_comm) {
      if ((rc = rccl_all_gather(m, stage, bytes, m->comm_stream))) return rc;
      AHA_HIP_CHECK(hipEventRecord(m->ev_ag[ci], m->comm_stream));
      return AHA_OK;
    }
    return model_all_gather(m, stage, bytes);
  };
  if (on_comm)
    for (int ci = 0; ci < nch; ++ci)
      if ((rc = gather(ci))) return join(rc);
  for (int ci = 0; ci < nch; ++ci) {
    const int off = ci * w, wc = std::min(w, spr - off);
    if (on_comm) {
      ProfScope ps(m, "ag_wait", (double)T * wc * H * 2, 0);   // what the compute stream waits for chunk ci of the gather
      AHA_HIP_CHECK(hipStreamWaitEvent(m->stream, m->ev_ag[ci], 0));
    } else if ((rc = gather(ci))) {
      return rc;
    }
    GemmArgs gc = g;
    gc.A = (const char*)m->p_hstage + (size_t)T * off * H * 2;
    gc.M = wc;
    gc.groups = T; gc.a_gstride = wc; gc.c_gstride = spr; gc.c_row0 = off; gc.m_total = S;
    ProfScope ps(m, "gemm", ((double)T * wc * g.K + (double)g.N * g.K + (double)T * wc * g.ldc) * 2, 2.0 * T * wc * g.N * g.K);
    launch_gemm_grouped(gc, m->stream);
  }
  return AHA_OK;
}

// ---- context-parallel prefill (round 4) ----------------------------------------------------------------------------------------------
// MI355X has 288 GB per GPU and the 8B checkpoint is 16 GB: for the long-context prefill of BASELINE cfg 5 every rank can hold the FULL
// weights, own a share of the prompt's ROWS, and run every GEMM / norm / rope on its own rows with no collective at all -- a GEMM's rows
// are independent.  The one op that couples rows is causal attention, which needs the K / V of every earlier position: per layer, the
// ranks all-gather the layer's K / V pages (8B: 147 456 B per position and layer -> 40 980 tokens = 168 MB per layer, 7/8 of it inbound
// per rank, against 2 x 294 MB of bf16 all-gather + 2 x 587 MB of f32 reduce-scatter per layer and rank in the tensor-parallel form).
// Ownership: the prompt's KV pages (64 tokens) are cut into 2 x world contiguous chunks; rank r owns chunks r and 2 x world - 1 - r (the
// "zigzag" that balances causal attention: an early chunk with few visible keys rides with a late one with many), so every page is
// written by exactly one rank, chunk boundaries are page boundaries, and rank 0 owns the LAST rows -- it ends the prefill holding the
// last hidden row, and, like every rank, the complete KV cache: decode continues on it without a hand-back.
// Results: every output row is computed by the same kernels on the same values as in the single-GPU prefill; with the GEMM plan pinned
// (plans depend on M) the logits and the cache are bit-identical to it (tests/test_cp_gpu.py).
struct CpPlan { int world, pmax; int a0[8], an[8], b0[8], bn[8]; };   // rank r's two page ranges [a0, a0 + an), [b0, b0 + bn)
struct RowSeg { int r0, len, l0; };                                     // prompt rows [r0, r0 + len) = rows [l0, l0 + len) of the rank's activation buffers
static bool cp_make_plan(int S, int world, int rank, CpPlan* p, std::vector<RowSeg>* segs) {
  const int P = (S + KV_PAGE_TOKENS - 1) / KV_PAGE_TOKENS, nc = 2 * world;
  if (world < 2 || world > 8 || P < 2 * nc) return false;   // at least two pages per chunk
  auto edge = [&](int j) { return (int)((int64_t)j * P / nc); };
  p->world = world;
  p->pmax = 0;
  for (int r = 0; r < world; ++r) {
    p->a0[r] = edge(r); p->an[r] = edge(r + 1) - edge(r);
    p->b0[r] = edge(nc - 1 - r); p->bn[r] = edge(nc - r) - edge(nc - 1 - r);
    p->pmax = std::max(p->pmax, p->an[r] + p->bn[r]);
  }
  segs->clear();
  for (int k = 0; k < 2; ++k) {
    const int pg0 = k ? p->b0[rank] : p->a0[rank], n = k ? p->bn[rank] : p->an[rank];
    const int r0 = pg0 * KV_PAGE_TOKENS, r1 = std::min(S, (pg0 + n) * KV_PAGE_TOKENS);
    segs->push_back(RowSeg{r0, r1 - r0, 0});
  }
  return true;
}
int debug_cp_plan(int S, int world, int rank, int* out5) {   // host only (tests): {r0_a, len_a, r0_b, len_b, pmax}; -1: this prompt is not sharded
  CpPlan p{};
  std::vector<RowSeg> segs;
  if (rank < 0 || rank >= world || !cp_make_plan(S, world, rank, &p, &segs)) return -1;
  out5[0] = segs[0].r0; out5[1] = segs[0].len; out5[2] = segs[1].r0; out5[3] = segs[1].len; out5[4] = p.pmax;
  return 0;
}
// staging slot s = rank * pmax + j  <->  the j-th page rank owns; one block copies 4 KB of the page's layer slice (kv heads x (K | V) x 16 KB)
__global__ __launch_bounds__(256) void kv_cp_copy_kernel(const uint64_t* __restrict__ page_ptrs, uint64_t layer_off, int slice_bytes,
                                                         char* __restrict__ stage, CpPlan p, int only_rank, int skip_rank, int to_pages) {
  const int rank = (int)blockIdx.x / p.pmax, j = (int)blockIdx.x % p.pmax;
  if ((only_rank >= 0 && rank != only_rank) || rank == skip_rank) return;
  int page;
  if (j < p.an[rank]) page = p.a0[rank] + j;
  else if (j < p.an[rank] + p.bn[rank]) page = p.b0[rank] + (j - p.an[rank]);
  else return;
  char* pg = reinterpret_cast<char*>(page_ptrs[page] + layer_off) + (size_t)blockIdx.y * 4096;
  char* sg = stage + (size_t)blockIdx.x * slice_bytes + (size_t)blockIdx.y * 4096;
  const u32x4_t v = *reinterpret_cast<const u32x4_t*>((to_pages ? sg : pg) + threadIdx.x * 16);
  *reinterpret_cast<u32x4_t*>((to_pages ? pg : sg) + threadIdx.x * 16) = v;
}
static int cp_all_gather(aha_model* m, void* buf, size_t bytes_per_rank) {
  if (m->rccl_comm) return rccl_all_gather(m, buf, bytes_per_rank, m->stream);
  AHA_HIP_CHECK(hipStreamSynchronize(m->stream));
  if (!m->cp_all_gather_cb || m->cp_all_gather_cb(buf, bytes_per_rank, m->cp_user) != 0) {
    set_error("context-parallel all-gather callback failed");
    return AHA_ERR_STATE;
  }
  return AHA_OK;
}
// after the layer's rope + KV append on the owned rows: every rank's pages of this layer to every rank
static int cp_gather_kv(aha_model* m, int li, const CpPlan& p) {
  const KvLayer kv = model_kv_layer(m, li);
  const int slice = m->desc.num_key_value_heads * 2 * KV_BLOCK_BYTES;
  const size_t per_rank = (size_t)p.pmax * slice;
  if ((size_t)p.world * per_rank > m->cp_stage_bytes) {
    set_error("context-parallel staging buffer too small");
    return AHA_ERR_STATE;
  }
  ProfScope ps(m, "cp_kv_gather", (double)p.world * per_rank, 0);
  const dim3 grid((unsigned)(p.world * p.pmax), (unsigned)(slice / 4096));
  hipLaunchKernelGGL(kv_cp_copy_kernel, grid, dim3(256), 0, m->stream, kv.page_ptrs, (uint64_t)kv.layer_off, slice, (char*)m->p_cp_stage, p, m->cp_rank, -1, 0);
  int rc = cp_all_gather(m, m->p_cp_stage, per_rank);
  if (rc) return rc;
  hipLaunchKernelGGL(kv_cp_copy_kernel, grid, dim3(256), 0, m->stream, kv.page_ptrs, (uint64_t)kv.layer_off, slice, (char*)m->p_cp_stage, p, -1, m->cp_rank, 1);
  return AHA_OK;
}

// ---- decode: one token through all layers; every length-dependent value is read from d_state on the device ----
// First kernel of a decode step: the token's embedding row (Qwen3Model::embedding_token_id, qwen3/model.rs:191-193) and
// the step's rope table -- cos/sin of pos[axis]*inv_freq, cast to the model dtype as apply_rotary_pos_emb does
// (rope.rs:96-132, 454-476), computed ONCE per step here instead of once per layer and block in the attention kernel.
__global__ void embed_state_kernel(const bf16_t* __restrict__ table, const StepState* __restrict__ st, bf16_t* __restrict__ out, int H,
                                   const float* __restrict__ inv_freq, const int32_t* __restrict__ axis_map, float* __restrict__ rope) {
  const u32x4_t* src = reinterpret_cast<const u32x4_t*>(table + (size_t)st->token * H);
  u32x4_t* dst = reinterpret_cast<u32x4_t*>(out);
  for (int i = threadIdx.x + blockIdx.x * blockDim.x; i < H / 8; i += blockDim.x * gridDim.x) dst[i] = src[i];
  if (blockIdx.x == 0 && threadIdx.x < 64) {
    const int i = threadIdx.x;
    const float ang = (float)st->pos[axis_map[i]] * inv_freq[i];
    rope[i] = rbf(cosf(ang));
    rope[64 + i] = rbf(sinf(ang));
  }
}
__global__ void advance_state_kernel(StepState* st, uint32_t* token_log, uint32_t* host_ring, uint32_t* host_done) {
  const uint32_t t = st->next_token;
  const int32_t step = st->step;
  token_log[step & 0xffff] = t;
  st->step = step + 1;
  st->token = t;
  st->pos[0] += 1;
  st->pos[1] += 1;
  st->pos[2] += 1;
  st->kv_start += 1;
  st->kv_len += 1;
  // publish to the host: token first, then the count (release at system scope: the host reads the count, then the slot)
  __hip_atomic_store(host_ring + ((uint32_t)step % RING_CAP), t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  __hip_atomic_store(host_done, (uint32_t)step + 1u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

// Tail of a step of the device-resident greedy loop (model_decode_greedy): argmax_partials_kernel + advance_state_kernel + the NEXT step's
// embed_state_kernel in one launch -- three single-block launches, each waiting on one or two dependent round trips, were 12.6 us of the
// 8B step.  Same values: the argmax rule (larger value, then smaller index) is a total order, so the order of the reduction is free;
// thread 0 then does advance_state_kernel's updates and stores verbatim; the embedding row and the rope table of the advanced position
// are embed_state_kernel's expressions on the values thread 0 has just written (handed over through LDS).  d_x and d_rope were last
// read by the lm_head matvec and the step's last attention launch, both earlier in the stream.
__global__ __launch_bounds__(256) void step_tail_kernel(const float* __restrict__ pv, const uint32_t* __restrict__ pi, int n, StepState* st,
                                                        const bf16_t* __restrict__ table, bf16_t* __restrict__ out, int H,
                                                        const float* __restrict__ inv_freq, const int32_t* __restrict__ axis_map,
                                                        float* __restrict__ rope, uint32_t* token_log, uint32_t* host_ring,
                                                        uint32_t* host_done) {
  __shared__ float sv[4];
  __shared__ uint32_t si[4];
  __shared__ uint32_t s_token;
  __shared__ int32_t s_pos[3];
  auto combine = [](float& bv, uint32_t& bi, float v, uint32_t i) {
    if (v > bv || (v == bv && i < bi)) { bv = v; bi = i; }
  };
  float bv = -INFINITY;
  uint32_t bi = 0xffffffffu;
  for (int i = threadIdx.x; i < n; i += 256) combine(bv, bi, pv[i], pi[i]);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ov = __shfl_xor(bv, o, 64);
    const uint32_t oi = __shfl_xor(bi, o, 64);
    combine(bv, bi, ov, oi);
  }
  if ((threadIdx.x & 63) == 0) { sv[threadIdx.x >> 6] = bv; si[threadIdx.x >> 6] = bi; }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < 4; ++w) combine(bv, bi, sv[w], si[w]);
    const uint32_t t = bi;
    const int32_t step = st->step;
    const int32_t p0 = st->pos[0] + 1, p1 = st->pos[1] + 1, p2 = st->pos[2] + 1;
    st->next_token = t;
    token_log[step & 0xffff] = t;
    st->step = step + 1;
    st->token = t;
    st->pos[0] = p0;
    st->pos[1] = p1;
    st->pos[2] = p2;
    st->kv_start += 1;
    st->kv_len += 1;
    // publish to the host: token first, then the count (release at system scope: the host reads the count, then the slot)
    __hip_atomic_store(host_ring + ((uint32_t)step % RING_CAP), t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    __hip_atomic_store(host_done, (uint32_t)step + 1u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    s_token = t;
    s_pos[0] = p0; s_pos[1] = p1; s_pos[2] = p2;
  }
  __syncthreads();
  // the next step's embed_state_kernel
  const u32x4_t* src = reinterpret_cast<const u32x4_t*>(table + (size_t)s_token * H);
  u32x4_t* dst = reinterpret_cast<u32x4_t*>(out);
  for (int i = threadIdx.x; i < H / 8; i += 256) dst[i] = src[i];
  if (threadIdx.x < 64) {
    const int i = threadIdx.x;
    const float ang = (float)s_pos[axis_map[i]] * inv_freq[i];
    rope[i] = rbf(cosf(ang));
    rope[64 + i] = rbf(sinf(ang));
  }
}

// AHA_GEMV_TRACE=1: in-kernel timeline of the decode matvecs (launch-per-op path), dumped by fetch_outputs.  The bf16 kernel only:
// gemv_mxfp8_kernel and gemv_mxfp4_kernel have no trace stamps, so a launch that decode_gemv sends to either leaves its slot as it was
// (gemv_trace_dump says so).  Nor has gemv_kernel_pk13: AHA_WPACK=0 or aha_hip_debug_pk13_single(m, 0) traces the bf16 kernel on the same weights.
static unsigned long long* gemv_trace_slot(aha_model* m, int launch_idx) {
  static const char* e = getenv("AHA_GEMV_TRACE");
  if (!e || !atoi(e)) return nullptr;
  const size_t n = (size_t)(4 * m->desc.num_hidden_layers + 1) * 18;
  if (!m->d_gemv_trace) {
    void* p = nullptr;
    if (dev_alloc(m, n * 8, &p, true) != AHA_OK) return nullptr;
    m->d_gemv_trace = (unsigned long long*)p;
  }
  return m->d_gemv_trace + (size_t)launch_idx * 18;
}

static void gemv_trace_dump(aha_model* m) {
  const int L = m->desc.num_hidden_layers, nl = 4 * L + 1;
  std::vector<unsigned long long> t((size_t)nl * 18);
  if (hipMemcpy(t.data(), m->d_gemv_trace, t.size() * 8, hipMemcpyDeviceToHost) != hipSuccess) return;
  static const char* names[4] = {"qkv", "o_proj", "gate_up", "down"};
  if (m->fp8_single && m->wq_format == AHA_WQ_MXFP8_E4M3 && L > 0 && m->layers[0].q_wqkv.q)
    fprintf(stderr, "[gemv trace] the model has MXFP8 copies: launches of gemv_mxfp8_kernel are not traced, their slots are stale or empty "
                    "(aha_hip_debug_fp8_single(m, 0) traces the bf16 kernel on the same weights)\n");
  if (m->fp4_single && m->wq_format == AHA_WQ_MXFP4_E2M1 && L > 0 && m->layers[0].q_wqkv.q)
    fprintf(stderr, "[gemv trace] the model has MXFP4 copies: launches of gemv_mxfp4_kernel are not traced, their slots are stale or empty "
                    "(aha_hip_debug_fp4_single(m, 0) traces the bf16 kernel on the same weights)\n");
  for (int k = 0; k < 4; ++k) {
    double d[3][5] = {}, gap = 0, span = 0;
    int n = 0;
    for (int li = 1; li < L; ++li) {
      const unsigned long long* p = t.data() + (size_t)(li * 4 + k) * 18;
      const unsigned long long* prev = p - 18;
      if (p[0] == 0 || prev[4] == 0) continue;
      for (int b = 0; b < 3; ++b)
        for (int j = 0; j < 4; ++j) d[b][j] += (double)(p[b * 6 + j + 1] - p[b * 6 + j]) * 0.01;
      unsigned long long pend = std::max(prev[4], std::max(prev[6 + 4], prev[12 + 4]));
      unsigned long long start = std::min(p[0], std::min(p[6], p[12]));
      unsigned long long end = std::max(p[4], std::max(p[6 + 4], p[12 + 4]));
      gap += (double)(start - pend) * 0.01;   // previous launch's last consume -> this launch's first instruction
      span += (double)(end - start) * 0.01;
      ++n;
    }
    if (!n) continue;
    fprintf(stderr, "[gemv trace] %-8s span %.2f us, gap since previous launch's last consume %.2f us |", names[k], span / n, gap / n);
    for (int b = 0; b < 3; ++b)
      fprintf(stderr, " blk%d: issue %.2f prologue %.2f first-consume %.2f rest %.2f |", b, d[b][0] / n, d[b][1] / n, d[b][2] / n, d[b][3] / n);
    fprintf(stderr, "\n");
  }
}

// embed = false: d_x and the rope table of this step were written by the previous step's tail.  tail = true (device-resident loop, whole
// vocabulary on this rank): the step ends with step_tail_kernel instead of the argmax launch (and the caller's advance_state_kernel).
static bool decode_tail_fused(const aha_model* m) { return m->lm_rows == m->desc.vocab_size; }
static void enqueue_decode_step(aha_model* m, size_t kv_len_after, bool embed = true, bool tail = false) {
  const aha_model_desc& c = m->desc;
  const int H = c.hidden_size, I = c.intermediate_size, d = c.head_dim, nh = c.num_attention_heads, kvh = c.num_key_value_heads;
  const int nq = nh * d, nkv = kvh * d;
  hipStream_t st = m->stream;
  if (embed) {
    ProfScope ps(m, "elem", H * 4.0, 0);
    hipLaunchKernelGGL(embed_state_kernel, dim3(1), dim3(256), 0, st, (const bf16_t*)m->embed, m->d_state, (bf16_t*)m->d_x, H,
                       m->d_inv_freq, m->d_axis_map, m->d_rope);
  }
  const int npages = (int)((kv_len_after + KV_PAGE_TOKENS - 1) / KV_PAGE_TOKENS);
  // KV splits of the fused decode attention: one block (4 waves = 4 KV units) per `div` pages
  static const char* e_div = getenv("AHA_ATTN_PAGES_PER_BLOCK");
  const int div = e_div ? std::max(1, atoi(e_div)) : 4;
  int nsplit = (npages + div - 1) / div;
  nsplit = std::max(1, std::min(std::min(nsplit, m->max_nsplit), 1024 / (nh / kvh)));  // g * nsplit <= 1024: LDS tables of the split merge
  for (int li = 0; li < c.num_hidden_layers; ++li) {
    const LayerWeights& L = m->layers[li];
    {  // h = RMSNorm(x); qkv = h Wqkv^T                      (qwen3/model.rs:79, modules.rs:538-552)
      GemvArgs g{};
      g.W = L.wqkv; g.x = m->d_x; g.norm_w = L.in_norm; g.eps = c.rms_norm_eps; g.y = m->d_qkv; g.N = nq + 2 * nkv; g.K = H;
      g.trace = gemv_trace_slot(m, li * 4 + 0);
      decode_gemv(m, g, GEMV_STORE, L.q_wqkv, L.p_wqkv, g.K * 4.0 + g.N * 2.0);
    }
    if (m->decode_fused) {
      // q/k norm + rope + KV append + attention over the paged cache (modules.rs:544-574, 757-813), then
      // x = x + attn Wo^T with the KV-split partials merged in the matvec prologue (modules.rs:577, qwen3/model.rs:81)
      AttnDecodeFusedArgs a{};
      a.qkv = m->d_qkv; a.q_norm_w = L.q_norm; a.k_norm_w = L.k_norm; a.rope = m->d_rope;
      a.kv = model_kv_layer(m, li); a.kv_start_v = (int)kv_len_after - 1; a.kv_len_v = (int)kv_len_after;
      // pages 0 .. npages - 1, the append slot's included, are lin_p0 + i * lin_step (the scramble knob is there to exercise the page
      // table: it keeps the table form even where one or two shuffled pages still are a progression)
      if ((size_t)npages <= m->lin_pages && !m->scramble_pages) {
        a.lin_page0 = m->lin_p0 + a.kv.layer_off;
        a.lin_step = m->lin_step;
      }
      m->last_attn_form = a.lin_step != 0 ? 1 : 0;
      a.part_o = m->d_part_o; a.part_ml = m->d_part_ml; a.nh = nh; a.kvh = kvh; a.nsplit = nsplit; a.eps = c.rms_norm_eps;
      a.scale = m->attn_scale; a.o = m->d_attn; a.head_ctr = m->d_bar + DECODE_HEAD_CTR_WORD;
      if (nsplit > 1) m->head_ctr_base += (unsigned)nsplit;  // a single split never touches the counter
      a.ctr_target = m->head_ctr_base;
      static const char* e_at = getenv("AHA_ATTN_TRACE");
      if (e_at && atoi(e_at)) {
        if (!m->d_attn_trace) {
          void* tp = nullptr;
          if (dev_alloc(m, (size_t)c.num_hidden_layers * 12 * 8, &tp, true) == AHA_OK) m->d_attn_trace = (unsigned long long*)tp;
        }
        if (m->d_attn_trace) a.trace = m->d_attn_trace + (size_t)li * 12;
      }
      GemvArgs g{};
      g.W = L.wo; g.x = m->d_attn; g.residual = m->d_x; g.y = m->d_x; g.N = H; g.K = nq;
      g.trace = gemv_trace_slot(m, li * 4 + 1);
      const double attn_bytes = (double)kv_len_after * 2 * nkv * 2 + (nq + 2 * nkv) * 2.0 + nsplit * nq * 4.0;
      {
        ProfScope ps(m, "attn_decode", attn_bytes, 4.0 * kv_len_after * nq);
        launch_attn_decode_fused(a, st);
      }
      decode_gemv(m, g, GEMV_RESIDUAL, L.q_wo, L.p_wo, g.K * 2.0 + g.N * 4.0);
    } else {  // three-launch variant (A/B knob AHA_DECODE_FUSED=0)
      {  // q/k norm + rope + append                            (modules.rs:544-566)
        RopeArgs r{};
        r.qkv = m->d_qkv; r.ld = nq + 2 * nkv; r.q_norm_w = L.q_norm; r.k_norm_w = L.k_norm;
        r.pos = m->d_state->pos; r.pos_ld = 1; r.inv_freq = m->d_inv_freq; r.axis_map = m->d_axis_map;
        r.q_out = m->d_q; r.kv = model_kv_layer(m, li); r.kv_start = &m->d_state->kv_start;
        r.S = 1; r.nh = nh; r.kvh = kvh; r.d = d; r.eps = c.rms_norm_eps;
        ProfScope ps(m, "elem", (nq + 2 * nkv) * 4.0, 0);
        launch_qknorm_rope(r, st);
      }
      {  // attention over the paged cache                       (modules.rs:567-574, 757-813)
        AttnDecodeArgs a{};
        a.q = m->d_q; a.kv = model_kv_layer(m, li); a.kv_len = &m->d_state->kv_len; a.part_o = m->d_part_o; a.part_ml = m->d_part_ml;
        a.o = m->d_attn; a.nh = nh; a.kvh = kvh; a.d = d; a.nsplit = nsplit; a.scale = m->attn_scale;
        ProfScope ps(m, "attn_decode", (double)kv_len_after * 2 * nkv * 2 + nq * 4.0, 4.0 * kv_len_after * nq);
        launch_attn_decode(a, st);
      }
      {  // x = x + attn Wo^T                                    (modules.rs:577, qwen3/model.rs:81)
        GemvArgs g{};
        g.W = L.wo; g.x = m->d_attn; g.residual = m->d_x; g.y = m->d_x; g.N = H; g.K = nq;
        decode_gemv(m, g, GEMV_RESIDUAL, L.q_wo, L.p_wo, g.K * 2.0 + g.N * 4.0);
      }
    }
    {  // act = silu(h Wg^T) * (h Wu^T), h = RMSNorm(x)        (qwen3/model.rs:83, modules.rs:81-84)
      GemvArgs g{};
      g.W = L.wgu; g.W2 = nullptr; g.x = m->d_x; g.norm_w = L.post_norm; g.eps = c.rms_norm_eps; g.y = m->d_act; g.N = I; g.K = H;
      g.trace = gemv_trace_slot(m, li * 4 + 2);
      decode_gemv(m, g, GEMV_SILU_MUL, L.q_wgu, L.p_wgu, H * 4.0 + I * 2.0);
    }
    {  // x = x + act Wd^T                                     (modules.rs:85, qwen3/model.rs:86)
      GemvArgs g{};
      g.W = L.wdown; g.x = m->d_act; g.residual = m->d_x; g.y = m->d_x; g.N = H; g.K = I;
      g.trace = gemv_trace_slot(m, li * 4 + 3);
      decode_gemv(m, g, GEMV_RESIDUAL, L.q_wdown, L.p_wdown, g.K * 2.0 + g.N * 4.0);
    }
  }
  if (!tail) {
    enqueue_lm_head(m, m->d_x);
    return;
  }
  enqueue_lm_head(m, m->d_x, false);
  ProfScope ps(m, "argmax", H * 4.0, 0);
  hipLaunchKernelGGL(step_tail_kernel, dim3(1), dim3(256), 0, st, m->d_blk_max, m->d_blk_idx, lm_head_partials(m), m->d_state,
                     (const bf16_t*)m->embed, (bf16_t*)m->d_x, H, m->d_inv_freq, m->d_axis_map, m->d_rope, m->d_token_log, m->h_ring_dev,
                     m->h_done_dev);
}

int model_forward_step(aha_model* m, uint32_t token, size_t offset, float* logits_out, uint32_t* argmax_out) {
  const aha_model_desc& c = m->desc;
  if (token >= (uint32_t)c.vocab_size) {
    set_error("token id out of range");
    return AHA_ERR_INVALID;
  }
  AHA_HIP_CHECK(hipSetDevice(m->ctx->device));
  int rc = model_ensure_pages(m, m->cache_len + 1);
  if (rc) return rc;
  // rope position: seqlen_offset (+ rope_delta for Qwen3-VL, qwen3vl/model.rs:1235-1264); cache slot: current length
  int64_t p = (int64_t)offset + m->rope_delta;
  if (c.arch == AHA_ARCH_QWEN3VL && !m->rope_delta_valid) {
    // first forward after clear_cache: get_rope_index on the ids alone -> position 0, delta 0 (model.rs:1229-1236)
    p = 0;
    m->rope_delta = 0;
    m->rope_delta_valid = true;
  }
  const int64_t pos[3] = {p, p, p};
  if ((rc = push_state(m, token, pos, m->cache_len, m->cache_len + 1))) return rc;
  enqueue_decode_step(m, m->cache_len + 1);
  m->cache_len += 1;
  AHA_HIP_CHECK(hipGetLastError());
  if (m->async_rc) { const int e = m->async_rc; m->async_rc = 0; return e; }
  return fetch_outputs(m, logits_out, argmax_out);
}

// Diagnostic (include/aha_hip.h aha_hip_debug_graph_step): what a hipGraph replay of ONE decode step would cost against enqueueing
// its launches, at the current cache length.  Both variants run `replays` times with the SAME kernel arguments (lengths travel as
// kernel arguments here, so a captured step can only be replayed for the length it was captured at): the attention's split-arrival
// target is stale after the first repetition in BOTH, the step's results are not meaningful, and the cache is cleared afterwards --
// the comparison isolates the launch path (stream launches vs one graph launch), nothing else.
int model_debug_graph_step(aha_model* m, int replays, double* us_launches, double* us_graph) {
  if (replays <= 0 || m->cache_len == 0 || m->tp_size > 1 || m->profiling) {
    set_error("debug_graph_step: needs a non-empty cache, tp_size 1, profiling off, replays > 0");
    return AHA_ERR_STATE;
  }
  AHA_HIP_CHECK(hipSetDevice(m->ctx->device));
  int rc = model_ensure_pages(m, m->cache_len + 1);
  if (rc) return rc;
  const int64_t pos[3] = {(int64_t)m->cache_len, (int64_t)m->cache_len, (int64_t)m->cache_len};
  if ((rc = push_state(m, 0, pos, m->cache_len, m->cache_len + 1))) return rc;
  hipEvent_t e0, e1;
  AHA_HIP_CHECK(hipEventCreate(&e0));
  AHA_HIP_CHECK(hipEventCreate(&e1));
  const unsigned base = m->head_ctr_base;
  auto step_with_fixed_args = [&] {
    m->head_ctr_base = base;   // the same arguments every repetition (see above)
    enqueue_decode_step(m, m->cache_len + 1);
  };
  for (int i = 0; i < 3; ++i) step_with_fixed_args();
  AHA_HIP_CHECK(hipEventRecord(e0, m->stream));
  for (int i = 0; i < replays; ++i) step_with_fixed_args();
  AHA_HIP_CHECK(hipEventRecord(e1, m->stream));
  AHA_HIP_CHECK(hipStreamSynchronize(m->stream));
  float ms = 0.f;
  AHA_HIP_CHECK(hipEventElapsedTime(&ms, e0, e1));
  if (us_launches) *us_launches = 1e3 * ms / replays;
  hipGraph_t graph = nullptr;
  hipGraphExec_t exec = nullptr;
  AHA_HIP_CHECK(hipStreamBeginCapture(m->stream, hipStreamCaptureModeThreadLocal));
  step_with_fixed_args();
  AHA_HIP_CHECK(hipStreamEndCapture(m->stream, &graph));
  AHA_HIP_CHECK(hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0));
  for (int i = 0; i < 3; ++i) AHA_HIP_CHECK(hipGraphLaunch(exec, m->stream));
  AHA_HIP_CHECK(hipEventRecord(e0, m->stream));
  for (int i = 0; i < replays; ++i) AHA_HIP_CHECK(hipGraphLaunch(exec, m->stream));
  AHA_HIP_CHECK(hipEventRecord(e1, m->stream));
  AHA_HIP_CHECK(hipStreamSynchronize(m->stream));
  AHA_HIP_CHECK(hipEventElapsedTime(&ms, e0, e1));
  if (us_graph) *us_graph = 1e3 * ms / replays;
  hipGraphExecDestroy(exec);
  hipGraphDestroy(graph);
  hipEventDestroy(e0);
  hipEventDestroy(e1);
  // leave a consistent model behind: arrival counters back to zero, cache cleared
  AHA_HIP_CHECK(hipMemsetAsync(m->d_bar, 0, DECODE_SYNC_BYTES, m->stream));
  m->head_ctr_base = 0;
  AHA_HIP_CHECK(hipStreamSynchronize(m->stream));
  return model_clear_cache(m);
}

int model_decode_greedy(aha_model* m, uint32_t first_token, size_t offset, size_t max_new, uint32_t* out) {
  const aha_model_desc& c = m->desc;
  if (max_new == 0) return 0;
  if (first_token >= (uint32_t)c.vocab_size) {
    set_error("token id out of range");
    return AHA_ERR_INVALID;
  }
  AHA_HIP_CHECK(hipSetDevice(m->ctx->device));
  int rc = model_ensure_pages(m, m->cache_len + max_new);
  if (rc) return rc;
  const int64_t p = (int64_t)offset + m->rope_delta;
  const int64_t pos[3] = {p, p, p};
  if ((rc = push_state(m, first_token, pos, m->cache_len, m->cache_len + 1))) return rc;
  // Bounded run-ahead: the host keeps at most `ahead` steps queued beyond the last token it has SEEN (the last kernel of a step
  // publishes the token to pinned host memory), so a stop token costs at most `ahead` further steps of GPU time -- and nothing
  // waits on the stream while tokens keep coming: the queue never drains, the host never blocks the device.  (Round 2 enqueued
  // chunks of 32 steps and looked for a stop token after each: up to 31 dead steps, ~100 ms at 8B speed.)
  static const size_t ahead = [] { const char* e = getenv("AHA_DECODE_RUNAHEAD"); return (size_t)std::max(1, std::min(64, e ? atoi(e) : 4)); }();
  m->h_state->step = 0;
  AHA_HIP_CHECK(hipMemcpyAsync(&m->d_state->step, &m->h_state->step, 4, hipMemcpyHostToDevice, m->stream));
  __atomic_store_n(m->h_done, 0u, __ATOMIC_RELEASE);
  size_t produced = 0, enq = 0, seen = 0;
  bool stop = false;
  const size_t base_len = m->cache_len;
  // Tensor parallelism: every step holds collectives, so all ranks must enqueue the SAME number of steps.  The run-ahead rule above
  // depends on when this host thread happens to read h_done (one rank may have seen the stop token and queue nothing while another
  // queues `ahead` more steps and then waits for ever in their all-reduces).  Under TP the schedule is therefore a function of the
  // token sequence alone: whole groups of `ahead` steps, the next group only after every token of the last one has been read.
  const bool lockstep = m->tp_size > 1;
  const bool fused_tail = decode_tail_fused(m);
  while (seen < max_new && !stop) {
    size_t want = 0;
    if (!lockstep) want = enq < max_new && enq - seen < ahead ? std::min(max_new - enq, ahead - (enq - seen)) : 0;
    else if (seen == enq) want = std::min(max_new - enq, ahead);
    for (size_t i = 0; i < want; ++i) {
      // one tail launch per step: it also writes the next step's d_x and rope table (the one after the last queued step is never used);
      // only the first step of the call embeds its own token (push_state above)
      enqueue_decode_step(m, base_len + enq + 1, !fused_tail || enq == 0, fused_tail);
      if (!fused_tail)
        hipLaunchKernelGGL(advance_state_kernel, dim3(1), dim3(1), 0, m->stream, m->d_state, m->d_token_log, m->h_ring_dev, m->h_done_dev);
      ++enq;
    }
    AHA_HIP_CHECK(hipGetLastError());
    if (m->async_rc) { const int e = m->async_rc; m->async_rc = 0; hipStreamSynchronize(m->stream); return e; }
    size_t done = __atomic_load_n(m->h_done, __ATOMIC_ACQUIRE);
    for (unsigned spins = 0; done == seen; ++spins) {   // the next token: ~one step of GPU time away at most
      if ((spins & 1023u) == 1023u && hipStreamQuery(m->stream) == hipSuccess && __atomic_load_n(m->h_done, __ATOMIC_ACQUIRE) == seen) {
        set_error("decode loop: the stream drained without publishing a token");
        return AHA_ERR_STATE;
      }
      done = __atomic_load_n(m->h_done, __ATOMIC_ACQUIRE);
    }
    for (; seen < done && !stop; ++seen) {
      const uint32_t t = __atomic_load_n(m->h_ring + (seen % RING_CAP), __ATOMIC_RELAXED);
      out[produced++] = t;
      for (int e = 0; e < c.n_stop_tokens; ++e)
        if (t == c.stop_tokens[e]) stop = true;
    }
  }
  // steps queued past a stop token still run (at most `ahead` - 1 of them): their KV slots lie beyond the cache length kept below
  // and are overwritten by the next append; wait for them so nothing of this call is in flight when it returns
  AHA_HIP_CHECK(hipStreamSynchronize(m->stream));
  m->steps_executed = (int64_t)enq;
  m->cache_len = base_len + produced;  // inputs consumed: first_token and the first produced-1 generated tokens
  m->have_logits = produced > 0 || m->have_logits;
  if (produced > 0) m->logits_assembled = false;
  return (int)produced;
}

// ---- prefill ---------------------------------------------------------------------------------------------------
// The decoder layers of every prefill: forward_initial_impl's (one prompt; context-, tensor- or sequence-parallel) and a packed pass's
// (packed_layers: independent sequences, single GPU).  What differs between the callers is this struct and the callable that runs between
// the qkv GEMM and o_proj -- q/k-norm + RoPE + KV append and the attention, which need the rows' cache positions.
struct PrefillRows {
  int M;               // rows in the activation buffers (a context-parallel rank: its own rows)
  int S;               // rows of the whole prompt: the sequence-parallel row slices are cut from it
  int spr;             // sequence-parallel tensor parallelism: rank r owns rows [r * spr, (r+1) * spr) between the GEMMs; 0 = off
  bool norm_in_gemm;   // the RMSNorm that follows o_proj / down_proj + residual rides on the GEMM call (GemmArgs::norm_w: inside the
                       // split-K reduce pass where the plan has one, a separate launch otherwise -- the same values); single GPU only
  bool vis;            // visual rows: DeepStack adds feature k after layer k < n_deepstack (qwen3vl/model.rs:806-822), which changes the
                       // rows between down_proj and the next layer's norm -- on those layers the norm does not ride on down_proj
};

// A prefill GEMM's profile entry: A, W and C once, C twice with a residual (read + write), half of N's columns out of a gate+up pair
struct GemmProf : ProfScope {
  static double out_elems(const GemmArgs& g) {
    return g.residual ? 2.0 * g.M * g.N : g.act == ACT_SILU_MUL_PAIRS ? (double)g.M * (g.N / 2) : (double)g.M * g.N;
  }
  GemmProf(aha_model* m, const GemmArgs& g)
      : ProfScope(m, "gemm", ((double)g.M * g.K + (double)g.N * g.K + out_elems(g)) * 2, 2.0 * g.M * g.N * g.K) {}
};

// rope_attn(li, L): layer li's q/k-norm + RoPE + KV append out of p_qkv and its attention into p_attn; returns an error code
template <class RopeAttn>
static int prefill_layers(aha_model* m, const PrefillRows& pr, RopeAttn&& rope_attn) {
  const aha_model_desc& c = m->desc;
  const int H = c.hidden_size, I = c.intermediate_size, nq = c.num_attention_heads * c.head_dim, nkv = c.num_key_value_heads * c.head_dim;
  const int M = pr.M;
  hipStream_t st = m->stream;
  int rc;
  bool in_norm_done = false;
  for (int li = 0; li < c.num_hidden_layers; ++li) {
    const LayerWeights& L = m->layers[li];
    {
      GemmArgs g{};
      g.A = m->p_h; g.W = L.wqkv; g.C = m->p_qkv; g.M = M; g.N = nq + 2 * nkv; g.K = H; g.lda = H; g.ldw = H; g.ldc = g.N; g.act = ACT_NONE;
      if (pr.spr > 0) {   // sequence-parallel: norm of this rank's rows, all-gather in chunks, GEMM per chunk (norm_gather_gemm)
        if ((rc = norm_gather_gemm(m, L.in_norm, g, pr.S, pr.spr))) return rc;
      } else {
        if (!in_norm_done && (rc = prefill_norm(m, L.in_norm, M, 0))) return rc;
        GemmProf ps(m, g);
        launch_gemm(g, st);
      }
    }
    in_norm_done = false;
    if ((rc = rope_attn(li, L))) return rc;
    {
      GemmArgs g{};
      g.A = m->p_attn; g.W = L.wo; g.C = m->p_x; g.residual = m->p_x; g.M = M; g.N = H; g.K = nq; g.lda = nq; g.ldw = nq; g.ldc = H; g.act = ACT_NONE;
      if (pr.norm_in_gemm) { g.norm_w = L.post_norm; g.norm_out = m->p_h; g.norm_eps = c.rms_norm_eps; }
      GemmProf ps(m, g);
      if ((rc = gemm_row_parallel(m, g, pr.spr))) return rc;
    }
    {
      GemmArgs g{};
      g.A = m->p_h; g.W = L.wgu; g.C = m->p_act; g.M = M; g.N = 2 * I; g.K = H; g.lda = H; g.ldw = H; g.ldc = I; g.act = ACT_SILU_MUL_PAIRS;
      if (pr.spr > 0) {
        if ((rc = norm_gather_gemm(m, L.post_norm, g, pr.S, pr.spr))) return rc;
      } else {
        if (!pr.norm_in_gemm && (rc = prefill_norm(m, L.post_norm, M, 0))) return rc;
        GemmProf ps(m, g);
        launch_gemm(g, st);
      }
    }
    {
      GemmArgs g{};
      g.A = m->p_act; g.W = L.wdown; g.C = m->p_x; g.residual = m->p_x; g.M = M; g.N = H; g.K = I; g.lda = I; g.ldw = I; g.ldc = H; g.act = ACT_NONE;
      if (pr.norm_in_gemm && li + 1 < c.num_hidden_layers && !(pr.vis && vision_has_deepstack(m, li))) {
        g.norm_w = m->layers[li + 1].in_norm; g.norm_out = m->p_h; g.norm_eps = c.rms_norm_eps;
        in_norm_done = true;
      }
      GemmProf ps(m, g);
      if ((rc = gemm_row_parallel(m, g, pr.spr))) return rc;
    }
    // (context-parallel: the visual rows of other ranks all land on the scratch row behind this rank's rows)
    if (pr.vis && (rc = vision_deepstack_add(m, li, m->p_x))) return rc;
  }
  return AHA_OK;
}

static int forward_initial_impl(aha_model* m, const uint32_t* ids, size_t n, size_t offset, const aha_mm_input* mm,
                                float* logits_out, uint32_t* argmax_out, bool hidden_only) {
  const aha_model_desc& c = m->desc;
  if (!ids || n == 0) {
    set_error("forward_initial: empty input_ids");
    return AHA_ERR_INVALID;
  }
  for (size_t i = 0; i < n; ++i)
    if (ids[i] >= (uint32_t)c.vocab_size) {
      set_error("token id out of range at position " + std::to_string(i));
      return AHA_ERR_INVALID;
    }
  const bool has_audio = mm && ((mm->audio_features && mm->n_frames > 0) || (mm->audio_samples && mm->n_samples > 0));
  if (has_audio && (c.arch != AHA_ARCH_QWEN3ASR || !m->audio)) {
    set_error("audio input given but this model has no audio tower");
    return AHA_ERR_UNSUPPORTED;
  }
  if (n == 1 && !mm) return model_forward_step(m, ids[0], offset, logits_out, argmax_out);
  AHA_HIP_CHECK(hipSetDevice(m->ctx->device));
  // AHA_PREFILL_TRACE=1: host wall clock of this call's stages on stderr (where the prefill's host side spends its time: the launches
  // themselves are asynchronous)
  static const bool ptrace = [] { const char* e = getenv("AHA_PREFILL_TRACE"); return e && atoi(e) != 0; }();
  const auto pt0 = std::chrono::steady_clock::now();
  auto pstamp = [&](const char* what) {
    if (ptrace) fprintf(stderr, "[prefill trace] %-28s %8.1f us\n", what, std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - pt0).count());
  };
  const int S = (int)n;
  const int H = c.hidden_size, d = c.head_dim, nh = c.num_attention_heads, kvh = c.num_key_value_heads;
  const int nq = nh * d, nkv = kvh * d;
  hipStream_t st = m->stream;
  int rc;
  if ((rc = ensure_prefill_scratch(m, n))) return rc;
  GemmWorkspaceScope ws_scope(m->p_gemm_ws, m->gemm_ws_bytes, m->d_sk_ctrs);  // split-K slabs / persistent-kernel chunks of this thread's GEMM launches
  if ((rc = model_ensure_pages(m, m->cache_len + n))) return rc;

  // Context-parallel prefill (cp_make_plan above): this rank owns two row chunks of the prompt.  Its activation buffers are COMPACT --
  // buffer row l0 + i holds prompt row r0 + i of a segment -- so every norm and GEMM below runs ONCE over all of the rank's rows; only
  // rope / KV append and attention, which need the rows' cache positions, run per segment.  A fresh cache only (offset 0), prompts of at
  // least AHA_CP_MIN_ROWS tokens, no audio rows; otherwise every rank simply computes the whole prompt (same results).
  const int kv_off = (int)m->cache_len;
  std::vector<RowSeg> segs;
  CpPlan cpp{};
  const char* e_cp = getenv("AHA_CP_MIN_ROWS");   // (read per call, like the AHA_TP_* thresholds: every rank's host sets it before the call)
  const int cp_min_rows = e_cp ? atoi(e_cp) : 2048;
  const bool cp = m->cp_size > 1 && m->tp_size <= 1 && kv_off == 0 && d == 128 && S >= cp_min_rows && !has_audio &&
                  (m->rccl_comm || m->cp_all_gather_cb) && cp_make_plan(S, m->cp_size, m->cp_rank, &cpp, &segs);
  if (!cp) segs.assign(1, RowSeg{0, S, 0});
  int Mloc = 0;
  for (RowSeg& sg : segs) { sg.l0 = Mloc; Mloc += sg.len; }
  struct MapGuard {   // the vision tower's scatter / DeepStack rows go through m->cp_row_map while this prefill runs
    aha_model* m;
    ~MapGuard() { m->cp_row_map.clear(); }
  } map_guard{m};
  if (cp) {
    m->cp_row_map.assign((size_t)S, Mloc);   // rows of other ranks -> the scratch row behind this rank's rows
    for (const RowSeg& sg : segs)
      for (int i = 0; i < sg.len; ++i) m->cp_row_map[(size_t)sg.r0 + i] = sg.l0 + i;
  }

  // positions: 1-D arange(offset, offset+S) on all three rows (rope.rs:599-604), or get_rope_index for Qwen3-VL
  std::vector<int32_t> pos(3 * (size_t)S);
  const bool has_image = mm && (mm->n_images > 0 || mm->n_videos > 0 || mm->image_embeds);   // images and / or videos
  if (has_image && (c.arch != AHA_ARCH_QWEN3VL || !m->vision)) {
    set_error("image input given but this model has no vision tower (arch / model.visual.* weights)");
    return AHA_ERR_UNSUPPORTED;
  }
  if (c.arch == AHA_ARCH_QWEN3VL) {
    if ((rc = vl_rope_index(m, ids, n, offset, has_image ? mm : nullptr, pos.data()))) return rc;
  } else {
    for (int a = 0; a < 3; ++a)
      for (int i = 0; i < S; ++i) pos[(size_t)a * S + i] = (int32_t)(offset + i);
  }
  const int64_t p0[3] = {pos[0], pos[S], pos[2 * (size_t)S]};
  std::vector<uint32_t> ids_loc;
  std::vector<int32_t> pos_loc;
  const uint32_t* ids_up = ids;
  const int32_t* pos_up = pos.data();
  if (cp) {   // this rank's rows of the ids and of the three position rows
    ids_loc.resize((size_t)Mloc);
    pos_loc.resize(3 * (size_t)Mloc);
    for (const RowSeg& sg : segs) {
      std::copy(ids + sg.r0, ids + sg.r0 + sg.len, ids_loc.begin() + sg.l0);
      for (int a = 0; a < 3; ++a)
        std::copy(pos.begin() + (size_t)a * S + sg.r0, pos.begin() + (size_t)a * S + sg.r0 + sg.len, pos_loc.begin() + (size_t)a * Mloc + sg.l0);
    }
    ids_up = ids_loc.data();
    pos_up = pos_loc.data();
  }
  AHA_HIP_CHECK(hipMemcpyAsync(m->p_ids, ids_up, (size_t)Mloc * 4, hipMemcpyHostToDevice, st));
  AHA_HIP_CHECK(hipMemcpyAsync(m->p_pos, pos_up, 3 * (size_t)Mloc * 4, hipMemcpyHostToDevice, st));
  if ((rc = push_state(m, ids[n - 1], p0, m->cache_len, m->cache_len + n))) return rc;
  pstamp("ids / positions enqueued");
  AHA_HIP_CHECK(hipStreamSynchronize(st));  // pos / ids are pageable host memory
  pstamp("... and landed");

  {
    ProfScope ps(m, "elem", (double)Mloc * H * 4, 0);
    launch_embed_gather(m->embed, m->p_ids, m->p_x, Mloc, H, st);
  }
  if (has_image) {
    // ViT -> masked_scatter of image embeds into the <|image_pad|> rows (qwen3vl/model.rs:1166-1190)
    if ((rc = vision_forward_and_scatter(m, ids, n, mm, m->p_x))) return rc;
    pstamp("vision tower enqueued");
  }
  if (has_audio) {
    // audio tower -> masked_scatter into the <|audio_pad|> rows (qwen3_asr/model.rs:343-358)
    const AudRequest r{mm, ids, n, 0, -1};
    if ((rc = audio_forward_requests(m, &r, 1, m->p_x))) return rc;
  }
  if (d == 128) launch_rope_table(m->p_pos, Mloc, m->d_inv_freq, m->d_axis_map, Mloc, m->p_rope, st);   // cos / sin once for all layers
  auto rows = [](const void* base, int64_t r0, int64_t row_elems) { return (void*)((char*)base + r0 * row_elems * 2); };   // bf16 rows
  // A context-parallel rank's two chunks (early + late, adjacent local rows) go out as ONE attention launch: each alone is a few hundred
  // blocks -- block rounds and ramp, not tile work, set its time (profiles/r05_shard_rank_time.txt) -- together the early chunk's
  // short blocks fill the late chunk's last round (kernels_attn.hip, AttnPrefillArgs::S2).
  const bool one_launch = segs.size() == 2 && segs[1].l0 == segs[0].l0 + segs[0].len && segs[1].r0 > segs[0].r0;
  const size_t n_attn = one_launch ? 1 : segs.size();   // attention launches per layer
  // q-norm + RoPE of the q heads inside the attention kernel's Q load where that kernel takes it (round 6: head_dim 128 on the 16-row
  // form, i.e. every prompt below ~3 k tokens): the rope kernel then handles K and V only and the attention reads the raw q heads of p_qkv
  bool q_fused = d == 128 && m->p_rope != nullptr;
  for (size_t si = 0; si < n_attn && q_fused; ++si) {
    AttnPrefillArgs pa{};
    pa.S = segs[si].len; pa.nh = nh; pa.kvh = kvh; pa.d = d; pa.causal = 1; pa.scale = m->attn_scale; pa.rows_hint = (int)S;
    if (one_launch) pa.S2 = segs[1].len;
    q_fused = attn_prefill_takes_qfuse(pa);
  }
  auto rope_attn = [&](int li, const LayerWeights& L) -> int {
    for (const RowSeg& sg : segs) {
      RopeArgs r{};
      r.qkv = rows(m->p_qkv, sg.l0, nq + 2 * nkv); r.ld = nq + 2 * nkv; r.q_norm_w = L.q_norm; r.k_norm_w = L.k_norm;
      r.pos = m->p_pos + sg.l0; r.pos_ld = Mloc; r.inv_freq = m->d_inv_freq; r.axis_map = m->d_axis_map;
      r.q_out = rows(m->p_q, sg.l0, nq); r.kv = model_kv_layer(m, li); r.kv_start = &m->d_state->kv_start;
      r.S = sg.len; r.nh = nh; r.kvh = kvh; r.d = d; r.eps = c.rms_norm_eps;
      r.kv_start_host = kv_off + sg.r0;   // == d_state->kv_start (push_state above) for the whole prompt
      r.rope_tab = rows(m->p_rope, sg.l0, 128);
      r.skip_q = q_fused ? 1 : 0;
      ProfScope ps(m, "elem", (double)sg.len * ((q_fused ? 0 : nq) + 2 * nkv) * 4, 0);
      launch_qknorm_rope(r, st);
    }
    if (cp && (rc = cp_gather_kv(m, li, cpp))) return rc;
    for (size_t si = 0; si < n_attn; ++si) {
      const RowSeg& sg = segs[si];
      AttnPrefillArgs a{};
      a.q = rows(m->p_q, sg.l0, nq); a.kv = model_kv_layer(m, li); a.o = rows(m->p_attn, sg.l0, nq); a.S = sg.len; a.nh = nh; a.kvh = kvh; a.d = d;
      a.kv_offset = kv_off + sg.r0; a.kv_total = kv_off + sg.r0 + sg.len; a.causal = 1; a.scale = m->attn_scale;
      a.rows_hint = (int)S;   // the kernel form by the whole prompt: a context-parallel rank's rows stay bit-identical to the un-sharded prefill
      if (q_fused) {
        a.q = rows(m->p_qkv, sg.l0, nq + 2 * nkv); a.q_ld = nq + 2 * nkv;
        a.q_norm_w = L.q_norm; a.q_rope_tab = rows(m->p_rope, sg.l0, 128); a.q_eps = c.rms_norm_eps;
      }
      double Lk = a.kv_total, flops = 4.0 * sg.len * (a.kv_offset + 0.5 * sg.len) * nq, rows_io = sg.len;
      if (one_launch) {
        const RowSeg& s2 = segs[1];
        a.S2 = s2.len; a.kv_offset2 = kv_off + s2.r0; a.kv_total2 = kv_off + s2.r0 + s2.len;
        Lk = a.kv_total2; flops += 4.0 * s2.len * (a.kv_offset2 + 0.5 * s2.len) * nq; rows_io += s2.len;
      }
      ProfScope ps(m, "attn_prefill", rows_io * nq * 4 + Lk * nkv * 4, flops);
      launch_attn_prefill(a, st);
    }
    return AHA_OK;
  };
  // sequence-parallel tensor parallelism: rank r owns rows [r * spr, (r+1) * spr) of the residual stream between the GEMMs
  const int spr = seq_parallel_on(m) ? (S + m->tp_size - 1) / m->tp_size : 0;
  if ((rc = prefill_layers(m, PrefillRows{Mloc, S, spr, m->tp_size <= 1, has_image}, rope_attn))) return rc;
  const void* x_last = (const char*)m->p_x + (size_t)(Mloc - 1) * H * 2;   // the prompt's last row (context-parallel: on rank 0, which owns the last chunk)
  if (cp) {
    // rank 0 owns the last chunk, hence the last row: every rank contributes its (stale, except rank 0's) copy of that row to one small
    // all-gather and takes slot 0 -- a broadcast; the final norm + lm_head then run replicated (full weights everywhere)
    AHA_HIP_CHECK(hipMemcpyAsync((char*)m->p_cp_stage + (size_t)m->cp_rank * H * 2, x_last, (size_t)H * 2, hipMemcpyDeviceToDevice, st));
    if ((rc = cp_all_gather(m, m->p_cp_stage, (size_t)H * 2))) return rc;
    AHA_HIP_CHECK(hipMemcpyAsync(m->d_x, m->p_cp_stage, (size_t)H * 2, hipMemcpyDeviceToDevice, st));
    x_last = m->d_x;
  }
  if (spr > 0) {
    // the last position lives on the rank that owns row S-1: every rank contributes that row as f32 (zeros elsewhere) to one
    // H-float all-reduce -- a broadcast, exact (bf16 -> f32 -> + 0 -> bf16)
    const bool mine = (S - 1) / spr == m->tp_rank;
    launch_row_to_f32(mine ? x_last : nullptr, m->d_partial, H, st);
    if ((rc = model_allreduce(m, m->d_partial, (size_t)H))) return rc;
    launch_f32_to_row(m->d_partial, m->d_x, H, st);
    x_last = m->d_x;
  }
  if (hidden_only) {  // forward_hidden: final norm of the last position only (qwen3/model.rs:186-188)
    launch_rmsnorm_rows(x_last, m->final_norm, m->d_hlast, 1, H, H, H, c.rms_norm_eps, st);
    m->cache_len += n;
    AHA_HIP_CHECK(hipGetLastError());
    return AHA_OK;
  }
  enqueue_lm_head(m, x_last);
  m->cache_len += n;
  AHA_HIP_CHECK(hipGetLastError());
  if (m->async_rc) { const int e = m->async_rc; m->async_rc = 0; return e; }   // e.g. a failed vocab-parallel all-reduce
  pstamp("decoder stack enqueued");
  rc = fetch_outputs(m, logits_out, argmax_out);
  pstamp("outputs fetched (GPU done)");
  return rc;
}

int model_forward_initial(aha_model* m, const uint32_t* ids, size_t n, size_t offset, const aha_mm_input* mm,
                          float* logits_out, uint32_t* argmax_out) {
  return forward_initial_impl(m, ids, n, offset, mm, logits_out, argmax_out, false);
}

// Qwen3Embedding::embed_one (qwen3_embedding/mod.rs:50-64): forward_hidden(ids, offset 0) -> last position after the final
// RMSNorm, bf16 -> f32, l2_normalize over the last dim (modules.rs:1287-1294: x / sqrt(sum(x^2) + 1e-6)), cache cleared.
// The stack runs on the GPU without the lm_head; the H-element normalisation is f32 host arithmetic like the reference's.
int model_embed(aha_model* m, const uint32_t* ids, size_t n, float* out) {
  if (!out) {
    set_error("embed: out is null");
    return AHA_ERR_INVALID;
  }
  if (m->desc.arch != AHA_ARCH_QWEN3) {
    set_error("embed: only the Qwen3 text stack has an embedding head in the reference (qwen3_embedding/mod.rs)");
    return AHA_ERR_UNSUPPORTED;
  }
  int rc = model_clear_cache(m);
  if (rc) return rc;
  if ((rc = forward_initial_impl(m, ids, n, 0, nullptr, nullptr, nullptr, true))) return rc;
  const int H = m->desc.hidden_size;
  std::vector<uint16_t> h((size_t)H);
  AHA_HIP_CHECK(hipMemcpyAsync(h.data(), m->d_hlast, (size_t)H * 2, hipMemcpyDeviceToHost, m->stream));
  AHA_HIP_CHECK(hipStreamSynchronize(m->stream));
  float ss = 0.f;
  for (int i = 0; i < H; ++i) {
    uint32_t u = (uint32_t)h[i] << 16;
    memcpy(&out[i], &u, 4);
    ss += out[i] * out[i];
  }
  const float nrm = sqrtf(ss + 1e-6f);
  for (int i = 0; i < H; ++i) out[i] /= nrm;
  return model_clear_cache(m);
}

// ---- packed-batch embedding -----------------------------------------------------------------------------------------------
// model_embed for many texts at once: the reference embeds one text at a time (qwen3_embedding/mod.rs:38-64), and so does this per
// sequence -- positions 0 .. len-1, a cache window of its own from a fresh 64-token page, causal attention inside it -- but the texts of
// a pass run as ONE packed prefill.  Every GEMM, norm and activation is row-wise and needs no change; the q/k-norm + RoPE kernel puts row r's
// K / V at cache slot row_slot[r], the 16-row attention kernel runs one block per (sequence, q block, head) over the sequence's own pages
// (AttnPrefillArgs::seg_tab), and embed_pool_kernel normalises every sequence's last row straight into the f32 output.  The generate_batch
// entries run their prompts' prefill as the same passes.
constexpr size_t PACKED_PASS_ROWS = 16384;

// The passes of a batch: sequences in order while the pass stays within max_tokens_per_pass rows (0: PACKED_PASS_ROWS) and twice that
// many cache slots (short texts waste up to a page each); a pass always holds at least one whole sequence.
struct PassRange {
  size_t j, k, off;   // sequences j .. k - 1, their ids from ids[off] on
};
static std::vector<PassRange> split_passes(const size_t* lens, size_t n, size_t max_tokens_per_pass) {
  const size_t budget = std::min(max_tokens_per_pass ? max_tokens_per_pass : PACKED_PASS_ROWS, (size_t)1 << 24);
  std::vector<PassRange> passes;
  for (size_t j = 0, off = 0; j < n;) {
    size_t rows = 0, slots = 0, k = j;
    while (k < n) {
      const size_t len = lens[k], sl = (len + KV_PAGE_TOKENS - 1) / KV_PAGE_TOKENS * KV_PAGE_TOKENS;
      if (k > j && (rows + len > budget || slots + sl > 2 * budget)) break;
      rows += len, slots += sl, ++k;
    }
    passes.push_back({j, k, off});
    off += rows;
    j = k;
  }
  return passes;
}

// The token ids of a batch: every sequence non-empty, within 2^24 tokens after growing by `grow` new ones, every id in the vocabulary
static int check_batch_ids(const aha_model_desc& c, const char* who, const uint32_t* ids, const size_t* lens, size_t n, size_t grow) {
  size_t total = 0;
  for (size_t j = 0; j < n; ++j) {
    if (lens[j] == 0) {
      set_error(std::string(who) + ": empty input_ids of sequence " + std::to_string(j));
      return AHA_ERR_INVALID;
    }
    if (lens[j] + grow > (size_t)1 << 24) {
      set_error(std::string(who) + ": sequence " + std::to_string(j) + (grow ? " would grow past" : " is longer than") + " 2^24 tokens");
      return AHA_ERR_INVALID;
    }
    for (size_t i = 0; i < lens[j]; ++i)
      if (ids[total + i] >= (uint32_t)c.vocab_size) {
        set_error("token id out of range in sequence " + std::to_string(j) + " at position " + std::to_string(i));
        return AHA_ERR_INVALID;
      }
    total += lens[j];
  }
  return AHA_OK;
}

struct ClearCacheGuard {   // the cache is empty afterwards, on success and on error alike (qwen3_embedding/mod.rs:58)
  aha_model* m;
  ~ClearCacheGuard() { model_clear_cache(m); }
};

// The layer stack of a packed prefill pass of independent sequences (run_packed_pass): prefill_layers on a single GPU, with the packed rows'
// cache slots in the rope kernel and segments in the attention.  The rows' embeddings in p_x, their positions' rope table in p_rope; K / V of
// row r go to cache slot d_slot[r] of the pages page_ptrs names, page p of 0 .. npages-1 holding the rows d_prow[2p] .. + d_prow[2p + 1]; the
// attention runs one block per (d_items entry, head) over d_seg's segments, reading attn_page_ptrs (chunked segments, d_kv0 their cache
// prefixes: the prefix pages, then the pages this pass writes) or else page_ptrs.  Leaves the last layer's output rows in p_x.  vis: the pass
// has visual rows (the tower's last pass scattered them).
static int packed_layers(aha_model* m, int S, const uint64_t* page_ptrs, const int32_t* d_seg, const int32_t* d_items, int n_items,
                         const int32_t* d_slot, const int32_t* d_prow, int npages, double attn_flops, bool vis = false,
                         const uint64_t* attn_page_ptrs = nullptr, const int32_t* d_kv0 = nullptr) {
  const aha_model_desc& c = m->desc;
  const int d = c.head_dim, nh = c.num_attention_heads, kvh = c.num_key_value_heads, nq = nh * d, nkv = kvh * d;
  hipStream_t st = m->stream;
  return prefill_layers(m, PrefillRows{S, S, 0, true, vis}, [&](int li, const LayerWeights& L) -> int {
    KvLayer kv = model_kv_layer(m, li);
    kv.page_ptrs = page_ptrs;
    {   // K and V of every row to its slot; the q heads are normed and rotated in the attention kernel's Q load
      RopeArgs r{};
      r.qkv = m->p_qkv; r.ld = nq + 2 * nkv; r.q_norm_w = L.q_norm; r.k_norm_w = L.k_norm;
      r.pos = m->p_pos; r.pos_ld = S; r.inv_freq = m->d_inv_freq; r.axis_map = m->d_axis_map;
      r.q_out = m->p_q; r.kv = kv; r.kv_start = &m->d_state->kv_start;
      r.S = S; r.nh = nh; r.kvh = kvh; r.d = d; r.eps = c.rms_norm_eps;
      r.kv_start_host = 0; r.rope_tab = m->p_rope; r.skip_q = 1;
      r.row_slot = d_slot; r.page_rows = d_prow; r.n_pages = npages;
      ProfScope ps(m, "elem", (double)S * 2 * nkv * 4, 0);
      launch_qknorm_rope(r, st);
    }
    AttnPrefillArgs a{};
    a.q = m->p_qkv; a.q_ld = nq + 2 * nkv; a.kv = kv; a.o = m->p_attn; a.S = S; a.nh = nh; a.kvh = kvh; a.d = d;
    a.kv_offset = 0; a.kv_total = S; a.causal = 1; a.scale = m->attn_scale;
    a.q_norm_w = L.q_norm; a.q_rope_tab = m->p_rope; a.q_eps = c.rms_norm_eps;
    a.seg_tab = d_seg; a.seg_items = d_items; a.n_items = n_items;
    if (attn_page_ptrs) a.kv.page_ptrs = attn_page_ptrs;
    a.seg_kv0 = d_kv0;
    ProfScope ps(m, "attn_prefill", (double)S * nq * 4 + (double)S * nkv * 4, attn_flops);
    launch_attn_prefill(a, st);
    return AHA_OK;
  });
}

// The host plan of one packed pass over n_seg sequences.  tab is the int32 table the pass's kernels read from p_pass_tab: segments
// {row0, len, page0} (AttnPrefillArgs::seg_tab) | items {segment, 64-row q block} (seg_items_of, causal) | per-row cache slots | per pass
// page {first row, rows} | every segment's last row.  Segment j's rows row0 .. row0 + len - 1 are its cache positions 0 .. len - 1, on
// pass pages page0, page0 + 1, ...; pass page p is logical page pages[p].
// With cache prefixes (kv0: the engine's chunked prefill) the table ends in every segment's kv0 (AttnPrefillArgs::seg_kv0), segment j's rows
// are its cache positions kv0 .. kv0 + len - 1, and the attention reads a page table of its own, attn_pages: per segment its prefix pages,
// then the ones this pass writes.  `pages` (the rope kernel's table: the slots and page rows index it) lists only the written ones, so no
// page of the rope kernel's list is without rows.
struct PackedPass {
  int n_seg = 0, S = 0, npages = 0, n_items = 0;
  size_t o_items = 0, o_slot = 0, o_prow = 0, o_last = 0, o_kv0 = 0;
  std::vector<int32_t> tab;
  std::vector<int32_t> pos;     // (3, S) positions
  std::vector<int64_t> pages;
  std::vector<int64_t> attn_pages;   // kv0 only
};

// lens: the sequences' lengths; page0: each one's first logical page (its pages follow it); pos3: null, or per sequence its (3, len)
// positions, an empty one meaning arange; kv0: null, or per sequence its cache prefix (a multiple of 64 tokens: the rows start a page),
// positions then kv0 + i
static PackedPass plan_packed_pass(const size_t* lens, int n_seg, const int64_t* page0, const std::vector<int32_t>* pos3,
                                   const int32_t* kv0 = nullptr) {
  PackedPass pp;
  pp.n_seg = n_seg;
  std::vector<int32_t> seg(3 * (size_t)n_seg), rope_p0(n_seg), k0s(n_seg, 0);
  for (int j = 0; j < n_seg; ++j) {
    const int len = (int)lens[j], k0 = kv0 ? kv0[j] : 0;
    k0s[j] = k0;
    seg[3 * j] = pp.S, seg[3 * j + 1] = len, seg[3 * j + 2] = (int32_t)(kv0 ? pp.attn_pages.size() : pp.pages.size());
    if (kv0)
      for (int p = 0; p * KV_PAGE_TOKENS < k0 + len; ++p) pp.attn_pages.push_back(page0[j] + p);
    rope_p0[j] = (int32_t)pp.pages.size();
    for (int p = 0; p * KV_PAGE_TOKENS < len; ++p) pp.pages.push_back(page0[j] + k0 / KV_PAGE_TOKENS + p);
    pp.S += len;
  }
  const int S = pp.S;
  pp.npages = (int)pp.pages.size();
  const std::vector<int32_t> items = seg_items_of(seg, true, kv0 ? &k0s : nullptr);
  pp.n_items = (int)items.size() / 2;
  pp.o_items = seg.size(), pp.o_slot = pp.o_items + items.size(), pp.o_prow = pp.o_slot + S, pp.o_last = pp.o_prow + 2 * (size_t)pp.npages;
  pp.o_kv0 = pp.o_last + n_seg;
  std::vector<int32_t>& tab = pp.tab;
  tab.resize(pp.o_last + n_seg + (kv0 ? n_seg : 0));
  std::copy(seg.begin(), seg.end(), tab.begin());
  std::copy(items.begin(), items.end(), tab.begin() + pp.o_items);
  if (kv0) std::copy(k0s.begin(), k0s.end(), tab.begin() + pp.o_kv0);
  pp.pos.resize(3 * (size_t)S);
  for (int j = 0; j < n_seg; ++j) {
    const int r0 = seg[3 * j], len = seg[3 * j + 1], p0 = rope_p0[j], k0 = k0s[j];
    const int32_t* pj = pos3 && !pos3[j].empty() ? pos3[j].data() : nullptr;
    for (int i = 0; i < len; ++i) {
      tab[pp.o_slot + r0 + i] = p0 * KV_PAGE_TOKENS + i;
      for (int a = 0; a < 3; ++a) pp.pos[(size_t)a * S + r0 + i] = pj ? pj[(size_t)a * len + i] : k0 + i;
    }
    for (int p = 0; p * KV_PAGE_TOKENS < len; ++p) {
      tab[pp.o_prow + 2 * (size_t)(p0 + p)] = r0 + p * KV_PAGE_TOKENS;
      tab[pp.o_prow + 2 * (size_t)(p0 + p) + 1] = std::min(KV_PAGE_TOKENS, len - p * KV_PAGE_TOKENS);
    }
    tab[pp.o_last + j] = r0 + len - 1;
  }
  return pp;
}

// Grows a buffer kept from pass to pass to at least n elements, its contents dropped: device memory (4096 elements at least) or pinned host
// memory.  The stream drains first, as work in flight may still read the old buffer.
template <class T>
static int grow_pass_buffer(aha_model* m, T** buf, size_t* cap, size_t n, bool pinned) {
  if (n <= *cap) return AHA_OK;
  AHA_HIP_CHECK(hipStreamSynchronize(m->stream));
  if (*buf) AHA_HIP_CHECK(pinned ? hipHostFree(*buf) : hipFree(*buf));
  *buf = nullptr;
  *cap = 0;
  const size_t want = pinned ? n : std::max(n, (size_t)4096);
  const hipError_t e = pinned ? hipHostMalloc((void**)buf, want * sizeof(T)) : hipMalloc((void**)buf, want * sizeof(T));
  if (e != hipSuccess) {
    set_error(std::string(pinned ? "hipHostMalloc" : "hipMalloc") + " of a packed pass's buffer failed: " + hipGetErrorString(e));
    return !pinned && e == hipErrorOutOfMemory ? AHA_ERR_OOM : AHA_ERR_HIP;
  }
  *cap = want;
  return AHA_OK;
}

// A planned pass up to its last layer: the rows' embeddings gathered from ids (the pass's, packed), the images / videos of vreqs and the
// audio clips of areqs encoded and scattered to their placeholder rows, the positions' rope table, then packed_layers over the pass pages
// page_ptrs names.  Leaves the last layer's rows in p_x and the plan's table in p_pass_tab.  The staging buffer is rewritten without a
// wait: every pass ends in a synchronise (its caller's tail, which needs one for its output anyway), so the previous pass's copies out
// of it have landed.
static int run_packed_pass(aha_model* m, const PackedPass& pp, const uint32_t* ids, const uint64_t* page_ptrs,
                           const std::vector<VisRequest>& vreqs = {}, const std::vector<AudRequest>& areqs = {},
                           const uint64_t* attn_page_ptrs = nullptr) {
  const aha_model_desc& c = m->desc;
  const int S = pp.S, H = c.hidden_size, nq = c.num_attention_heads * c.head_dim;
  hipStream_t st = m->stream;
  int rc;
  if ((rc = ensure_prefill_scratch(m, (size_t)S))) return rc;
  if ((size_t)S > m->pf_cap) {
    set_error("packed pass: prefill scratch of " + std::to_string(m->pf_cap) + " rows for a pass of " + std::to_string(S));
    return AHA_ERR_STATE;
  }
  const size_t n_tab = pp.tab.size(), n_stage = 4 * (size_t)S + n_tab;
  if ((rc = grow_pass_buffer(m, &m->p_pass_tab, &m->p_pass_tab_cap, n_tab, false)) ||
      (rc = grow_pass_buffer(m, &m->h_pass_stage, &m->h_pass_stage_cap, n_stage, true)))
    return rc;
  int32_t* hs = m->h_pass_stage;   // ids | positions | table
  memcpy(hs, ids, (size_t)S * 4);
  memcpy(hs + S, pp.pos.data(), pp.pos.size() * 4);
  memcpy(hs + 4 * (size_t)S, pp.tab.data(), n_tab * 4);
  GemmWorkspaceScope ws_scope(m->p_gemm_ws, m->gemm_ws_bytes, m->d_sk_ctrs);
  AHA_HIP_CHECK(hipMemcpyAsync(m->p_ids, hs, (size_t)S * 4, hipMemcpyHostToDevice, st));
  AHA_HIP_CHECK(hipMemcpyAsync(m->p_pos, hs + S, pp.pos.size() * 4, hipMemcpyHostToDevice, st));
  AHA_HIP_CHECK(hipMemcpyAsync(m->p_pass_tab, hs + 4 * (size_t)S, n_tab * 4, hipMemcpyHostToDevice, st));
  {
    ProfScope ps(m, "elem", (double)S * H * 4, 0);
    launch_embed_gather(m->embed, m->p_ids, m->p_x, S, H, st);
  }
  // ViT -> masked_scatter of every request's visual rows into its placeholder rows of the pass (qwen3vl/model.rs:1166-1190)
  if (!vreqs.empty() && (rc = vision_forward_requests(m, vreqs.data(), vreqs.size(), m->p_x))) return rc;
  // the audio tower over every clip of the pass -> masked_scatter into each request's <|audio_pad|> rows (qwen3_asr/model.rs:343-358)
  if (!areqs.empty() && (rc = audio_forward_requests(m, areqs.data(), areqs.size(), m->p_x))) return rc;
  launch_rope_table(m->p_pos, S, m->d_inv_freq, m->d_axis_map, S, m->p_rope, st);   // the packed rows' cos / sin, once for all layers
  double attn_flops = 0;
  const bool has_kv0 = !pp.attn_pages.empty();
  for (int j = 0; j < pp.n_seg; ++j)
    attn_flops += 4.0 * pp.tab[3 * j + 1] * ((has_kv0 ? pp.tab[pp.o_kv0 + j] : 0) + 0.5 * pp.tab[3 * j + 1]) * nq;
  const int32_t* t = m->p_pass_tab;
  return packed_layers(m, S, page_ptrs, t, t + pp.o_items, pp.n_items, t + pp.o_slot, t + pp.o_prow, pp.npages, attn_flops, !vreqs.empty(),
                       has_kv0 ? attn_page_ptrs : nullptr, has_kv0 ? t + pp.o_kv0 : nullptr);
}

static int embed_pass(aha_model* m, const uint32_t* ids, const size_t* lens, int n_seg, float* out) {
  const aha_model_desc& c = m->desc;
  const int H = c.hidden_size;
  hipStream_t st = m->stream;
  // the pass's pages are logical pages 0 .. npages - 1 (a pass reuses the previous one's): m->d_page_ptrs is its page table
  std::vector<int64_t> page0(n_seg);
  for (int j = 0, p = 0; j < n_seg; p += (int)((lens[j] + KV_PAGE_TOKENS - 1) / KV_PAGE_TOKENS), ++j) page0[j] = p;
  const PackedPass pp = plan_packed_pass(lens, n_seg, page0.data(), nullptr);
  int rc;
  if ((rc = model_ensure_pages(m, (size_t)pp.npages * KV_PAGE_TOKENS)) ||
      (rc = grow_pass_buffer(m, &m->p_pool, &m->p_pool_cap, (size_t)n_seg * H, false)) || (rc = run_packed_pass(m, pp, ids, m->d_page_ptrs)))
    return rc;
  {
    ProfScope ps(m, "elem", (double)n_seg * H * 2 + (double)n_seg * H * 4, 0);
    launch_embed_pool(m->p_x, m->p_pass_tab, n_seg, m->final_norm, m->p_pool, H, c.rms_norm_eps, st);
  }
  AHA_HIP_CHECK(hipGetLastError());
  AHA_HIP_CHECK(hipMemcpyAsync(out, m->p_pool, (size_t)n_seg * H * 4, hipMemcpyDeviceToHost, st));
  AHA_HIP_CHECK(hipStreamSynchronize(st));
  return AHA_OK;
}

int model_embed_batch(aha_model* m, const uint32_t* ids, const size_t* seq_lens, size_t n_seqs, size_t max_tokens_per_pass, float* out) {
  const aha_model_desc& c = m->desc;
  if (n_seqs == 0) {
    set_error("embed_batch: empty batch (n_seqs == 0)");
    return AHA_ERR_INVALID;
  }
  if (!ids || !seq_lens || !out) {
    set_error("embed_batch: null input_ids / seq_lens / out");
    return AHA_ERR_INVALID;
  }
  if (c.arch != AHA_ARCH_QWEN3) {
    set_error("embed_batch: only the Qwen3 text stack has an embedding head in the reference (qwen3_embedding/mod.rs)");
    return AHA_ERR_UNSUPPORTED;
  }
  if (m->tp_size > 1 || m->cp_size > 1 || c.head_dim != 128) {
    set_error("embed_batch: a single-GPU model with head_dim 128 only (no tensor / context parallelism)");
    return AHA_ERR_UNSUPPORTED;
  }
  int rc = check_batch_ids(c, "embed_batch", ids, seq_lens, n_seqs, 0);
  if (rc) return rc;
  AHA_HIP_CHECK(hipSetDevice(m->ctx->device));
  if ((rc = model_clear_cache(m))) return rc;
  ClearCacheGuard guard{m};
  for (const PassRange& p : split_passes(seq_lens, n_seqs, max_tokens_per_pass))
    if ((rc = embed_pass(m, ids + p.off, seq_lens + p.j, (int)(p.k - p.j), out + p.j * c.hidden_size))) return rc;
  return AHA_OK;
}

// ---- batched greedy generation ---------------------------------------------------------------------------------------------------
// generate_generic (common/generate.rs:115-159) at temperature 0 for many prompts at once.  Prefill (gen_packed_pass): the packed passes
// of embed_batch, each prompt on its own run of pages, then every prompt's last row through the final RMSNorm and the batched lm_head ->
// the first token.  Decode (gen_write_row per row, gen_decode_step, gen_finish_step): all unfinished sequences advance together, one step =
// the R rows through every layer with the weights streamed once per group of <= 32 rows (gemv_rows) and ONE attention launch per layer
// (attn_decode_batch); the next tokens stay on the device (the step's argmax writes the token vector the next step's embedding gather
// reads), the host reads them once per step to drop finished rows.  The blocking entries (model_generate_batch, its draft-and-verify loop)
// and the engine's step are these same pieces under different bookkeeping.
namespace {
struct DevBufs {   // per-call device / pinned scratch, freed after the stream has drained
  hipStream_t st;
  std::vector<void*> dev, host;
  ~DevBufs() {
    hipStreamSynchronize(st);
    for (void* p : dev) hipFree(p);
    for (void* p : host) hipHostFree(p);
  }
  template <class T>
  int alloc(T** out, size_t n, bool zero = false) {
    void* p = nullptr;
    hipError_t e = hipMalloc(&p, std::max<size_t>(n, 1) * sizeof(T));
    if (e != hipSuccess) {
      set_error(std::string("generate_batch: hipMalloc failed: ") + hipGetErrorString(e));
      return e == hipErrorOutOfMemory ? AHA_ERR_OOM : AHA_ERR_HIP;
    }
    dev.push_back(p);
    if (zero && hipMemsetAsync(p, 0, std::max<size_t>(n, 1) * sizeof(T), st) != hipSuccess) return AHA_ERR_HIP;
    *out = (T*)p;
    return AHA_OK;
  }
  template <class T>
  int alloc_host(T** out, size_t n) {
    void* p = nullptr;
    if (hipHostMalloc(&p, std::max<size_t>(n, 1) * sizeof(T)) != hipSuccess) {
      set_error("generate_batch: pinned host allocation failed");
      return AHA_ERR_OOM;
    }
    host.push_back(p);
    *out = (T*)p;
    return AHA_OK;
  }
};
}  // namespace

constexpr int GEN_ROW_GROUP = 32;   // rows of one gemv_rows launch: larger batches stream the weights once per group

// y[rows] = epi(x[rows] . W^T) in groups of GEN_ROW_GROUP rows.  For GEMV_LOGITS, y_f32 / blk partials are (rows, ldf) / (rows, tiles).
// wq: the MXFP8 or MXFP4 copy of g.W (model_quantize_weights, m->wq_format), streamed in its place when it exists -- the same bits at
// 1 + 1/32 or 1/2 + 1/32 bytes per weight (profile classes gemv_rows_fp8, gemv_rows_fp4).
static void gemv_rows_groups(aha_model* m, GemvRowsArgs g, GemvEpi epi, int rows, float* ws, const WQuant* wq = nullptr) {
  const int tiles = gemv_rows_num_tiles(g.N);
  const bool copy = wq && wq->q && m->fp8_rows;
  const bool fp8 = copy && m->wq_format == AHA_WQ_MXFP8_E4M3, fp4 = copy && m->wq_format == AHA_WQ_MXFP4_E2M1;
  const double wbytes = (double)g.N * g.K * (fp8 ? 1.03125 : fp4 ? 0.53125 : 2.0);
  for (int r0 = 0; r0 < rows; r0 += GEN_ROW_GROUP) {
    GemvRowsArgs a = g;
    a.R = std::min(GEN_ROW_GROUP, rows - r0);
    a.x = (const bf16_t*)g.x + (int64_t)r0 * g.ldx;
    if (g.y) a.y = (bf16_t*)g.y + (int64_t)r0 * g.ldy;
    if (g.residual) a.residual = (const bf16_t*)g.residual + (int64_t)r0 * g.ldy;
    if (g.y_f32) a.y_f32 = g.y_f32 + (int64_t)r0 * g.ldf;
    if (g.blk_max) a.blk_max = g.blk_max + (int64_t)r0 * tiles, a.blk_idx = g.blk_idx + (int64_t)r0 * tiles;
    a.ws = ws;
    ProfScope ps(m, fp8 ? "gemv_rows_fp8" : fp4 ? "gemv_rows_fp4" : "gemv_rows", wbytes + (double)a.R * (g.K + g.N) * 2, 2.0 * a.R * g.N * g.K);
    if (fp8) launch_gemv_rows_mxfp8(a, wq->q, wq->scales, epi, m->stream);
    else if (fp4) launch_gemv_rows_mxfp4(a, wq->q, wq->scales, epi, m->stream);
    else launch_gemv_rows(a, epi, m->stream);
  }
}

struct GenCall {
  int n = 0, V = 0, H = 0, max_nsplit = 1;
  int rows = 0;   // the largest row count of a step when it exceeds n (draft-and-verify: a sequence's drafts are rows of their own)
  int seq_words = SPEC_SEQ_WORDS;   // words of a sequence's entry behind the row table's rows (the engine: ENG_SEQ_WORDS)
  int ctr_rows = 0;                 // head_ctr blocks when they are not one per row (the engine: its slots, then its draft rows)
  float* ws = nullptr;
  void *x = nullptr, *h = nullptr, *qkv = nullptr, *attn = nullptr, *act = nullptr;
  float *rope = nullptr, *logits = nullptr, *blk_max = nullptr, *part_o = nullptr, *part_ml = nullptr;
  uint32_t *blk_idx = nullptr, *tok[2] = {nullptr, nullptr};
  int32_t* rowtab = nullptr;
  unsigned* ctr = nullptr;
  uint64_t* pass_pages = nullptr;
  int32_t* h_rowtab = nullptr;   // pinned
  uint32_t* h_tok = nullptr;     // pinned: a step's tokens
  uint32_t *spec_out = nullptr, *h_spec_out = nullptr;   // draft-and-verify: (n, SPEC_OUT_WORDS) emitted tokens per sequence, device / pinned
  // the caller's outputs: per sequence max_new entries of tokens_out (n_out of them written) and of step_logits_out (V floats each)
  size_t max_new = 0;
  uint32_t* tokens_out = nullptr;
  size_t* n_out = nullptr;
  float* step_logits_out = nullptr;
  // the engine (aha_engine): sequence j's generated tokens at seq_tokens[j] instead of tokens_out + j * max_new; row r's logits to
  // row_logits[r] (null: not copied) instead of step_logits_out; the decode steps' page table (null: the model's)
  uint32_t* const* seq_tokens = nullptr;
  float* const* row_logits = nullptr;
  const uint64_t* dec_pages = nullptr;
  // per-token logprobs (aha_hip_generate_batch_logprobs, aha_hip_engine_step_logprobs): lp_top[j] = sequence j's top_logprobs (-1: none);
  // row r's entry goes to row_logprobs[r] (the engine; null: not reported) or to logprobs_out[j * max_new + n_out[j]].  The pass's
  // buffers (gen_logprob_alloc; lp_tab null: none) and finish_step's per-row scratch.
  const int32_t* lp_top = nullptr;
  aha_token_logprobs* logprobs_out = nullptr;
  aha_token_logprobs* const* row_logprobs = nullptr;
  int32_t *lp_tab = nullptr, *h_lp_tab = nullptr;
  float *lp_cval = nullptr, *lp_part = nullptr, *lp_out = nullptr, *h_lp_out = nullptr;
  unsigned* lp_cidx = nullptr;
  std::vector<int> lp_slot, lp_fb;
};
static_assert(sizeof(aha_token_logprobs) == 168 && sizeof(aha_token_logprobs) == (size_t)LOGPROB_OUT_M * 4 && AHA_MAX_TOP_LOGPROBS == LOGPROB_MAX_TOP,
              "aha_token_logprobs is the head of a logprob pass output row");

static inline uint32_t* gen_seq_tokens(const GenCall& gc, int j) {
  return gc.seq_tokens ? gc.seq_tokens[j] : gc.tokens_out + (size_t)j * gc.max_new;
}

// final RMSNorm + lm_head + argmax of `rows` rows of gc.x (bf16, pitch H) -> logits rows / token vector entries from `row0` on
static void gen_head(aha_model* m, GenCall& gc, int row0, int rows, uint32_t* tok_out) {
  const aha_model_desc& c = m->desc;
  const int H = c.hidden_size, tiles = gemv_rows_num_tiles(gc.V);
  {
    ProfScope ps(m, "elem", (double)rows * H * 4, 0);
    launch_rmsnorm_rows((const bf16_t*)gc.x + (int64_t)row0 * H, m->final_norm, (bf16_t*)gc.h + (int64_t)row0 * H, rows, H, H, H, c.rms_norm_eps,
                        m->stream);
  }
  GemvRowsArgs g{};
  g.W = m->lm_head; g.x = (const bf16_t*)gc.h + (int64_t)row0 * H; g.ldx = H; g.N = gc.V; g.K = H;
  g.y_f32 = gc.logits + (int64_t)row0 * gc.V; g.ldf = gc.V;
  g.blk_max = gc.blk_max + (int64_t)row0 * tiles; g.blk_idx = gc.blk_idx + (int64_t)row0 * tiles;
  gemv_rows_groups(m, g, GEMV_LOGITS, rows, gc.ws, &m->q_lm_head);
  ProfScope ps(m, "argmax", 0, 0);
  launch_argmax_rows(gc.blk_max + (int64_t)row0 * tiles, gc.blk_idx + (int64_t)row0 * tiles, tiles, rows, tok_out + row0, m->stream);
}

// A batched decode step's running totals over its rows
struct GenStepRows {
  int max_split = 1;      // the rows' largest KV split
  double kv_tokens = 0;   // their cache lengths summed (the profile's bytes)
};

// Row r of a batched decode step's table (kernels.h GEN_ROW_*): a sequence whose cache holds kv_len tokens after the row's append, on the
// pages from page0 of the step's page table.  ctr_acc: where the counters of the row's head_ctr block ctr_row stand, advanced by the step's
// arrivals; src / tok: the entry of the step's token vector that holds the row's input token, or the token itself (GEN_ROW_TOK).
static void gen_write_row(const aha_model* m, GenCall& gc, GenStepRows& sr, int r, int64_t page0, int kv_len, int64_t rope_delta,
                          unsigned& ctr_acc, int src, int ctr_row, int32_t tok = 0) {
  const aha_model_desc& c = m->desc;
  const int ns = attn_decode_nsplit(kv_len, c.num_attention_heads / c.num_key_value_heads, m->max_nsplit);
  int32_t* t = gc.h_rowtab + (size_t)r * GEN_ROW_WORDS;
  t[GEN_ROW_PAGE0] = (int32_t)page0;
  t[GEN_ROW_KVLEN] = kv_len;
  t[GEN_ROW_NSPLIT] = ns;
  t[GEN_ROW_CTR] = (int32_t)ctr_acc;
  t[GEN_ROW_POS] = (int32_t)(kv_len - 1 + rope_delta);   // seqlen_offset + rope_delta (qwen3vl/model.rs:1235-1264)
  t[GEN_ROW_SRC] = src;
  t[GEN_ROW_CTRROW] = ctr_row;
  t[GEN_ROW_TOK] = tok;
  if (ns > 1) ctr_acc += (unsigned)c.num_hidden_layers * (unsigned)ns;   // a single split never touches its counter
  sr.max_split = std::max(sr.max_split, ns);
  sr.kv_tokens += kv_len;
}

// The packed prefill pass of a generate_batch* call or of an engine step, planned by the caller: pp over ids (the pass's, packed), its pages
// indices into phys, the physical page addresses.  mm (may be null, as may any entry): segment j's images / videos or its audio clip
// (check_mm_requests checked both kinds), reported as sequence seq0 + j, encoded for the whole pass in one tower pass and scattered to its
// placeholder rows.  The pass's pages go up as a table of their own, gc.pass_pages -- the rope kernel's, then the attention's when the plan
// has cache prefixes -- so pages a segment does not write in this pass never appear in the rope kernel's page list; the table is free: the
// previous pass ended in a synchronise.  Then the last rows of the first k segments -> gc.x rows row0 .., and the head -> their first tokens
// in token vector 0.  Nothing here waits for the stream: the caller does, before the table and the staging buffer are reused.
static int gen_packed_pass(aha_model* m, GenCall& gc, const PackedPass& pp, const uint32_t* ids, const aha_mm_input* const* mm, int seq0,
                           const uint64_t* phys, int k, int row0) {
  std::vector<VisRequest> vreqs;   // the pass's requests with images / videos, at their first packed row
  std::vector<AudRequest> areqs;   // the pass's requests with an audio clip
  for (int j = 0; j < pp.n_seg && mm; ++j) {
    const aha_mm_input* q = mm[j];
    const int r0 = pp.tab[3 * j];
    const size_t len = (size_t)pp.tab[3 * j + 1];
    if (q && (q->n_images > 0 || q->n_videos > 0)) vreqs.push_back(VisRequest{q, ids + r0, len, r0, seq0 + j});
    else if (q && m->audio) areqs.push_back(AudRequest{q, ids + r0, len, r0, seq0 + j});
  }
  const size_t n_rope = pp.pages.size();
  std::vector<uint64_t> tab(n_rope + pp.attn_pages.size());
  for (size_t p = 0; p < n_rope; ++p) tab[p] = phys[(size_t)pp.pages[p]];
  for (size_t p = 0; p < pp.attn_pages.size(); ++p) tab[n_rope + p] = phys[(size_t)pp.attn_pages[p]];
  AHA_HIP_CHECK(hipMemcpy(gc.pass_pages, tab.data(), tab.size() * 8, hipMemcpyHostToDevice));
  if (int rc = run_packed_pass(m, pp, ids, gc.pass_pages, vreqs, areqs, gc.pass_pages + n_rope)) return rc;
  if (k > 0) {
    launch_embed_gather(m->p_x, reinterpret_cast<const uint32_t*>(m->p_pass_tab + pp.o_last), (bf16_t*)gc.x + (int64_t)row0 * gc.H, k, gc.H,
                        m->stream);
    gen_head(m, gc, row0, k, gc.tok[0]);
    AHA_HIP_CHECK(hipGetLastError());
  }
  return AHA_OK;
}

// generate_batch_mm's requests, every check of the towers and of get_rope_index before any device work; positions (3, len) and
// rope_delta of each request with images / videos (a text request: arange, delta 0)
static int check_mm_requests(aha_model* m, const uint32_t* ids, const size_t* seq_lens, size_t n_seqs, const aha_mm_input* const* mm,
                             std::vector<std::vector<int32_t>>& pos3, std::vector<int64_t>& rope_delta) {
  const aha_model_desc& c = m->desc;
  int rc;
  size_t off = 0;
  for (size_t j = 0; j < n_seqs; off += seq_lens[j], ++j) {
    const aha_mm_input* q = mm[j];
    if (!q) continue;
    const std::string who = "generate_batch_mm: sequence " + std::to_string(j) + ": ";
    if (q->image_embeds) {
      set_error(who + "precomputed image_embeds are not supported in batches (pixel values only)");
      return AHA_ERR_UNSUPPORTED;
    }
    const bool has_img = q->n_images > 0, has_vid = q->n_videos > 0;
    if (((q->audio_features && q->n_frames > 0) || (q->audio_samples && q->n_samples > 0)) && (c.arch != AHA_ARCH_QWEN3ASR || !m->audio)) {
      set_error(who + "audio input given but this model has no audio tower");
      return AHA_ERR_UNSUPPORTED;
    }
    // on a Qwen3-ASR model every entry without images / videos is an audio request: the tower's own checks (samples or features, the
    // placeholder count)
    if (!has_img && !has_vid && c.arch == AHA_ARCH_QWEN3ASR && m->audio) {
      const AudRequest r{q, ids + off, seq_lens[j], 0, (int)j};
      if ((rc = audio_check_requests(m, &r, 1))) return rc;
      continue;
    }
    if (!has_img && !has_vid) continue;
    if (c.arch != AHA_ARCH_QWEN3VL || !m->vision) {
      set_error(who + "image input given but this model has no vision tower (arch / model.visual.* weights)");
      return AHA_ERR_UNSUPPORTED;
    }
    int64_t n_img, n_vid;
    if ((rc = vision_check_request(c, VisRequest{q, ids + off, seq_lens[j], 0, (int)j}, &n_img, &n_vid))) return rc;
    pos3[j].resize(3 * seq_lens[j]);
    if ((rc = rope_index_core(c, ids + off, seq_lens[j], q->image_grid_thw, has_img ? q->n_images : 0, q->video_grid_thw,
                              has_vid ? q->n_videos : 0, pos3[j].data(), &rope_delta[j]))) {
      set_error(who + last_error_cstr());
      return rc;
    }
  }
  return AHA_OK;
}

// The call's device buffers (decode rows, logits, token vectors, attention partials, the pass page table) and pinned row table / tokens;
// gc.max_nsplit set by the caller
static int gen_call_alloc(aha_model* m, DevBufs& bufs, GenCall& gc, size_t max_pass_pages) {
  const aha_model_desc& c = m->desc;
  // n: the rows a step can have (the row table also holds one SPEC_SEQ_WORDS entry per sequence behind the rows)
  const int n = std::max(gc.n, gc.rows), H = gc.H, V = gc.V, I = c.intermediate_size, nh = c.num_attention_heads, kvh = c.num_key_value_heads;
  const int nq = nh * 128, nkv = kvh * 128;
  const size_t tab_words = (size_t)n * GEN_ROW_WORDS + (size_t)gc.n * gc.seq_words;
  size_t ws = 0;
  const int shapes[5][2] = {{nq + 2 * nkv, H}, {H, nq}, {2 * I, H}, {H, I}, {V, H}};
  for (auto& sh : shapes) ws = std::max(ws, gemv_rows_ws_floats(std::min(n, GEN_ROW_GROUP), sh[0], sh[1]));
  const int tiles = gemv_rows_num_tiles(V);
  int rc;
  if ((rc = bufs.alloc(&gc.ws, ws)) || (rc = bufs.alloc((bf16_t**)&gc.x, (size_t)n * H)) || (rc = bufs.alloc((bf16_t**)&gc.h, (size_t)n * H)) ||
      (rc = bufs.alloc((bf16_t**)&gc.qkv, (size_t)n * (nq + 2 * nkv))) || (rc = bufs.alloc((bf16_t**)&gc.attn, (size_t)n * nq)) ||
      (rc = bufs.alloc((bf16_t**)&gc.act, (size_t)n * I)) || (rc = bufs.alloc(&gc.rope, (size_t)n * 128)) ||
      (rc = bufs.alloc(&gc.logits, (size_t)n * V)) || (rc = bufs.alloc(&gc.blk_max, (size_t)n * tiles)) ||
      (rc = bufs.alloc(&gc.blk_idx, (size_t)n * tiles)) || (rc = bufs.alloc(&gc.tok[0], (size_t)n)) || (rc = bufs.alloc(&gc.tok[1], (size_t)n)) ||
      (rc = bufs.alloc(&gc.rowtab, tab_words)) || (rc = bufs.alloc(&gc.ctr, (size_t)(gc.ctr_rows ? gc.ctr_rows : n) * kvh * 32, true)) ||
      (rc = bufs.alloc(&gc.part_o, (size_t)n * gc.max_nsplit * nq)) || (rc = bufs.alloc(&gc.part_ml, (size_t)n * gc.max_nsplit * nh * 2)) ||
      (rc = bufs.alloc(&gc.pass_pages, max_pass_pages)) || (rc = bufs.alloc_host(&gc.h_rowtab, tab_words)) ||
      (rc = bufs.alloc_host(&gc.h_tok, (size_t)n)))
    return rc;
  return AHA_OK;
}

// The logprob pass's buffers for gc.n rows
static int gen_logprob_alloc(DevBufs& bufs, GenCall& gc) {
  if (!logprob_shape_ok(gc.V)) {
    set_error("generate_batch_logprobs: vocabulary too large for the logprob pass");
    return AHA_ERR_UNSUPPORTED;
  }
  const size_t n = (size_t)gc.n, nw = (size_t)logprob_stage1_waves(gc.V);
  int rc;
  if ((rc = bufs.alloc(&gc.lp_tab, n * LOGPROB_ROW_WORDS)) || (rc = bufs.alloc_host(&gc.h_lp_tab, n * LOGPROB_ROW_WORDS)) ||
      (rc = bufs.alloc(&gc.lp_cval, n * nw * LOGPROB_MAX_TOP)) || (rc = bufs.alloc(&gc.lp_cidx, n * nw * LOGPROB_MAX_TOP)) ||
      (rc = bufs.alloc(&gc.lp_part, 2 * n * nw)) || (rc = bufs.alloc(&gc.lp_out, n * LOGPROB_OUT_WORDS)) ||
      (rc = bufs.alloc_host(&gc.h_lp_out, n * LOGPROB_OUT_WORDS)))
    return rc;
  return AHA_OK;
}

// Sampled generation: one sampler per sequence and the candidate step's buffers (no samplers: greedy)
struct GenChoice {
  std::vector<HostSampler> samplers;
  int nw = 0;   // sample_stage1_waves(V)
  int32_t *d_stab = nullptr, *h_stab = nullptr;
  uint32_t *d_sctx = nullptr, *h_sctx = nullptr, *d_cidx = nullptr;
  float *d_cval = nullptr, *d_part = nullptr, *d_sout = nullptr, *h_sout = nullptr, *h_fb = nullptr;
  // the rows' addend lists (logit_bias, presence / frequency penalties), pinned staging and device: null until a sequence has an adjust
  uint32_t *d_adj_id = nullptr, *h_adj_id = nullptr;
  float *d_adj_val = nullptr, *h_adj_val = nullptr;
  // allowed-token masks: row j of h_masks (pinned) / d_masks is sequence / slot j's ceil(V / 32) words; null until the call or engine can
  // have masks.  mask_state[j]: 0 = its next token is unmasked, 1 = masked by the words already on the device, 2 = masked, words to upload.
  uint32_t *d_masks = nullptr, *h_masks = nullptr;
  size_t mask_w = 0;
  std::vector<uint8_t> mask_state;
  aha_token_mask_fn mask_fn = nullptr;   // aha_hip_generate_batch_masked's callback: asked once per live sequence per step
  void* mask_user = nullptr;
  std::vector<int> mode, slot, fb_rows;   // finish_step's per-row scratch
};

// the mask buffers for n sequences / slots, every word all ones, every sequence unmasked
static int gen_choice_mask_alloc(DevBufs& bufs, int n, int V, GenChoice& ch) {
  ch.mask_w = token_mask_words((size_t)V);
  int rc;
  if ((rc = bufs.alloc(&ch.d_masks, (size_t)n * ch.mask_w)) || (rc = bufs.alloc_host(&ch.h_masks, (size_t)n * ch.mask_w))) return rc;
  memset(ch.h_masks, 0xff, (size_t)n * ch.mask_w * 4);
  ch.mask_state.assign(n, 0);
  return AHA_OK;
}

// room for `cap` addend entries (cap > 0)
static int gen_choice_adj_alloc(DevBufs& bufs, size_t cap, GenChoice& ch) {
  int rc;
  if ((rc = bufs.alloc(&ch.d_adj_id, cap)) || (rc = bufs.alloc(&ch.d_adj_val, cap)) || (rc = bufs.alloc_host(&ch.h_adj_id, cap)) ||
      (rc = bufs.alloc_host(&ch.h_adj_val, cap)))
    return rc;
  return AHA_OK;
}
// the most entries a sequence's list can reach: its non-zero biases and one per generated token, never more than the vocabulary
static size_t adjust_list_cap(const HostSampler& S, size_t max_new, size_t V) {
  return S.adj.active ? std::min(V, S.adj.bias_ids.size() + max_new) : 0;
}

// The candidate step's buffers for gc.n rows: ctx_cap penalty-context ids, n_fb full logits rows on the host
static int gen_choice_alloc(DevBufs& bufs, const GenCall& gc, size_t ctx_cap, size_t n_fb, GenChoice& ch) {
  const int n = gc.n;
  const size_t V = (size_t)gc.V;
  ch.nw = sample_stage1_waves(gc.V);
  int rc;
  const size_t cand = (size_t)n * (ch.nw + 16) * 64;
  if ((rc = bufs.alloc(&ch.d_stab, (size_t)n * SAMPLE_ROW_WORDS)) || (rc = bufs.alloc(&ch.d_sctx, ctx_cap)) || (rc = bufs.alloc(&ch.d_cval, cand)) ||
      (rc = bufs.alloc(&ch.d_cidx, cand)) || (rc = bufs.alloc(&ch.d_part, 2 * (size_t)n * ch.nw)) ||
      (rc = bufs.alloc(&ch.d_sout, (size_t)n * SAMPLE_OUT_WORDS)) || (rc = bufs.alloc_host(&ch.h_stab, (size_t)n * SAMPLE_ROW_WORDS)) ||
      (rc = bufs.alloc_host(&ch.h_sctx, ctx_cap)) || (rc = bufs.alloc_host(&ch.h_sout, (size_t)n * SAMPLE_OUT_WORDS)) ||
      (rc = bufs.alloc_host(&ch.h_fb, n_fb * V)))
    return rc;
  return AHA_OK;
}

static int gen_choice_init(DevBufs& bufs, const GenCall& gc, const aha_sampling_params* params, GenChoice& ch,
                           const aha_logit_adjust* adjust = nullptr) {
  const int n = gc.n, V = gc.V;
  if (!sample_shape_ok(V, 64)) {
    set_error("generate_batch_sampled: vocabulary too large for the candidate step");
    return AHA_ERR_UNSUPPORTED;
  }
  ch.samplers.resize(n);
  size_t ctx_cap = 0, n_fb = 0, adj_cap = 0;
  int rc;
  for (int j = 0; j < n; ++j) {
    if ((rc = host_sampler_init(ch.samplers[j], params[j]))) return rc;
    if (adjust) sampler_set_adjust(ch.samplers[j], &adjust[j]);
    const HostSampler& S = ch.samplers[j];
    adj_cap += adjust_list_cap(S, gc.max_new, (size_t)V);
    if (S.repeat_penalty != 1.0f) ctx_cap += std::min<size_t>(gc.max_new, (size_t)S.repeat_last_n);
    // a sequence that may need its full logits row: Sampling::All, oversized k, any TopP (nucleus wider than the candidates)
    if (S.kind != SAMPLE_ARGMAX && (S.kind == SAMPLE_TOPP || sampler_candidates_needed(S, (size_t)V) == 0)) ++n_fb;
  }
  if (adj_cap && (rc = gen_choice_adj_alloc(bufs, adj_cap, ch))) return rc;
  return gen_choice_alloc(bufs, gc, ctx_cap, n_fb, ch);
}

// The end of every step (the prefill's first tokens, then each decode step): the tokens of rows r = 0 .. R-1 (row r = sequence seqs[r])
// into gc.h_tok, from the device argmax vector `tok_dev` the head wrote.  Greedy: one copy and one sync.  Sampled: before that sync, one
// candidate step over every row that samples (its penalty context uploaded with it) and the candidates' copy; after it the host picks,
// a second sync only for rows whose candidates cannot decide (their logits rows come down), and the picked tokens go back up into
// tok_dev for the next step's embedding gather.  gc.step_logits_out (greedy or sampled): every step's logits.
// Addends (a sampler with an active aha_logit_adjust): the sampler's counts are brought up to the sequence's tokens, and a row with a live
// addend is a candidate row (k = 1 for ArgMax) whose sorted (id, addend) list goes up with the table; a row that needs its full vector gets
// the addends in sampler_pick.  A step without a live addend launches and copies what it did before they existed.
// Masks: the callback (batch generation) is asked here, after the step's device work has been queued and before the candidate step is, with
// the sequence's previous words in place; a masked row is a candidate row (k = 1 for ArgMax) that names its words in d_masks, uploaded when
// they changed; a row that needs its full vector gets the mask in sampler_pick.  A step without a masked row launches and copies what it
// did before masks existed.
// Logprobs (gc.lp_top): one two-launch pass over the rows that ask for them, behind the candidate step and in front of the same sync; a
// greedy row's entry is complete on the device (its token is in tok_dev), a sampled row's lp is finished here from the raw logit of the
// token the host picked -- among its candidates' raw logits, which came down with the entry, or in its full row when it fell back.
static int gen_finish_step(aha_model* m, GenCall& gc, GenChoice& ch, const std::vector<int>& seqs, uint32_t* tok_dev) {
  hipStream_t st = m->stream;
  const int R = (int)seqs.size(), V = gc.V;
  const bool sampled = !ch.samplers.empty();
  const size_t max_new = gc.max_new;
  uint32_t* h_tok = gc.h_tok;
  enum { GREEDY, CAND, FULL };
  int ns = 0;
  if (sampled) {
    ch.mode.assign(R, GREEDY);
    ch.slot.assign(R, -1);
    size_t nc = 0, na = 0, nm = 0;
    for (int r = 0; r < R; ++r) {
      const int j = seqs[r];
      HostSampler& S = ch.samplers[j];
      float pen;
      size_t n_ctx;
      sampler_penalty_context(S, gc.n_out[j], &pen, &n_ctx);
      sampler_adjust_sync(S, gen_seq_tokens(gc, j), gc.n_out[j], (size_t)V);
      const bool live = sampler_adjust_bound(S) > 0;
      if (ch.mask_fn) {
        uint32_t* words = ch.h_masks + (size_t)j * ch.mask_w;
        const int mrc = ch.mask_fn(ch.mask_user, (size_t)j, gen_seq_tokens(gc, j), gc.n_out[j], words, ch.mask_w);
        if (mrc < 0) {
          set_error("generate_batch_masked: the mask callback returned " + std::to_string(mrc) + " for sequence " + std::to_string(j) +
                    " at step " + std::to_string(gc.n_out[j]));
          return AHA_ERR_STATE;
        }
        if (mrc > 0 && !token_mask_any(words, (size_t)V)) {
          set_error("generate_batch_masked: the mask of sequence " + std::to_string(j) + " at step " + std::to_string(gc.n_out[j]) +
                    " allows no id below vocab_size");
          return AHA_ERR_INVALID;
        }
        ch.mask_state[j] = mrc > 0 ? 2 : 0;
      }
      const bool masked = !ch.mask_state.empty() && ch.mask_state[j] != 0;
      S.mask = masked ? ch.h_masks + (size_t)j * ch.mask_w : nullptr;   // for a pick from the full vector
      S.mask_words = masked ? ch.mask_w : 0;
      if (S.kind == SAMPLE_ARGMAX && pen == 1.0f && !live && !masked) continue;   // the device argmax is the token
      const int k = S.kind == SAMPLE_ARGMAX ? 1 : sampler_candidates_needed(S, (size_t)V);
      if (!k) {
        ch.mode[r] = FULL;
        continue;
      }
      ch.mode[r] = CAND;
      ch.slot[r] = ns;
      int32_t* t = ch.h_stab + (size_t)ns * SAMPLE_ROW_WORDS;
      // `&logits / temperature`: 1/T computed in f64, applied in f32 (as model_sample_candidates; ArgMax: T treated as 1)
      const float inv_t = S.kind == SAMPLE_ARGMAX ? 1.0f : (float)(1.0 / (double)(float)S.temperature);
      const size_t c0 = nc;
      if (pen != 1.0f) {   // the distinct in-vocabulary ids of the last n_ctx generated (apply_repeat_penalty's HashSet)
        const uint32_t* g = gen_seq_tokens(gc, j) + gc.n_out[j] - n_ctx;
        for (size_t i = 0; i < n_ctx; ++i)
          if (g[i] < (uint32_t)V) ch.h_sctx[nc++] = g[i];
        std::sort(ch.h_sctx + c0, ch.h_sctx + nc);
        nc = (size_t)(std::unique(ch.h_sctx + c0, ch.h_sctx + nc) - ch.h_sctx);
      }
      t[SAMPLE_ROW_LROW] = r;
      t[SAMPLE_ROW_K] = k;
      memcpy(&t[SAMPLE_ROW_INVT], &inv_t, 4);
      memcpy(&t[SAMPLE_ROW_PEN], &pen, 4);
      t[SAMPLE_ROW_CTX0] = (int32_t)c0;
      t[SAMPLE_ROW_NCTX] = (int32_t)(nc - c0);
      t[SAMPLE_ROW_ADJ0] = (int32_t)na;
      t[SAMPLE_ROW_NADJ] = live ? (int32_t)sampler_adjust_list(S, ch.h_adj_id + na, ch.h_adj_val + na) : 0;
      na += (size_t)t[SAMPLE_ROW_NADJ];
      t[SAMPLE_ROW_MASK] = masked ? j : -1;
      nm += masked;
      ++ns;
    }
    // changed masks go up whether their row is a candidate row or not: state 1 means "on the device"
    for (int r = 0; r < R && !ch.mask_state.empty(); ++r) {
      const int j = seqs[r];
      if (ch.mask_state[j] != 2) continue;
      AHA_HIP_CHECK(hipMemcpyAsync(ch.d_masks + (size_t)j * ch.mask_w, ch.h_masks + (size_t)j * ch.mask_w, ch.mask_w * 4, hipMemcpyHostToDevice, st));
      ch.mask_state[j] = 1;
    }
    if (ns) {
      AHA_HIP_CHECK(hipMemcpyAsync(ch.d_stab, ch.h_stab, (size_t)ns * SAMPLE_ROW_WORDS * 4, hipMemcpyHostToDevice, st));
      if (nc) AHA_HIP_CHECK(hipMemcpyAsync(ch.d_sctx, ch.h_sctx, nc * 4, hipMemcpyHostToDevice, st));
      if (na) {
        AHA_HIP_CHECK(hipMemcpyAsync(ch.d_adj_id, ch.h_adj_id, na * 4, hipMemcpyHostToDevice, st));
        AHA_HIP_CHECK(hipMemcpyAsync(ch.d_adj_val, ch.h_adj_val, na * 4, hipMemcpyHostToDevice, st));
      }
      const char* names[3] = {"sample_rows_stage1", "sample_rows_stage2a", "sample_rows_stage2b"};
      for (int stage = 0; stage < 3; ++stage) {
        // (the logits, the uploaded lists, the masks)
        ProfScope ps(m, names[stage], stage == 0 ? (double)ns * V * 4 + (double)na * 8 + (double)nm * ch.mask_w * 4 : 0, 0);
        launch_topk_rows(gc.logits, V, V, ns, ch.d_stab, ch.d_sctx, ch.d_cval, ch.d_cidx, ch.d_part, ch.d_part + (size_t)gc.n * ch.nw, ch.d_sout,
                         stage, st, ch.d_adj_id, ch.d_adj_val, ch.d_masks);
      }
      AHA_HIP_CHECK(hipGetLastError());
      AHA_HIP_CHECK(hipMemcpyAsync(ch.h_sout, ch.d_sout, (size_t)ns * SAMPLE_OUT_WORDS * 4, hipMemcpyDeviceToHost, st));
    }
  }
  auto lp_dst = [&](int r) -> aha_token_logprobs* {
    if (gc.row_logprobs) return gc.row_logprobs[r];
    return gc.logprobs_out ? gc.logprobs_out + (size_t)seqs[r] * max_new + gc.n_out[seqs[r]] : nullptr;
  };
  int nl = 0;
  if (gc.lp_top && gc.lp_tab) {
    gc.lp_slot.assign(R, -1);
    gc.lp_fb.assign(R, -1);
    for (int r = 0; r < R; ++r) {
      if (!lp_dst(r) || gc.lp_top[seqs[r]] < 0) continue;
      int32_t* t = gc.h_lp_tab + (size_t)nl * LOGPROB_ROW_WORDS;
      t[LOGPROB_ROW_LROW] = r;
      t[LOGPROB_ROW_NTOP] = gc.lp_top[seqs[r]];
      t[LOGPROB_ROW_TOK] = r;
      t[LOGPROB_ROW_CSLOT] = sampled ? ch.slot[r] : -1;
      gc.lp_slot[r] = nl++;
    }
    if (nl) {
      const int nw = logprob_stage1_waves(V);
      AHA_HIP_CHECK(hipMemcpyAsync(gc.lp_tab, gc.h_lp_tab, (size_t)nl * LOGPROB_ROW_WORDS * 4, hipMemcpyHostToDevice, st));
      const char* names[2] = {"logprob_rows_stage1", "logprob_rows_stage2"};
      for (int stage = 0; stage < 2; ++stage) {
        ProfScope ps(m, names[stage], stage == 0 ? (double)nl * V * 4 : 0, 0);
        launch_logprob_rows(gc.logits, V, V, nl, gc.lp_tab, tok_dev, gc.lp_cval, gc.lp_cidx, gc.lp_part, gc.lp_part + (size_t)gc.n * nw,
                            sampled ? ch.d_sout : nullptr, gc.lp_out, stage, st);
      }
      AHA_HIP_CHECK(hipGetLastError());
      AHA_HIP_CHECK(hipMemcpyAsync(gc.h_lp_out, gc.lp_out, (size_t)nl * LOGPROB_OUT_WORDS * 4, hipMemcpyDeviceToHost, st));
    }
  }
  // after the step's sync(s) and picks: every row's entry to the caller
  auto lp_finish = [&]() -> int {
    if (!gc.lp_top) return AHA_OK;
    for (int r = 0; r < R; ++r) {
      aha_token_logprobs* d = lp_dst(r);
      if (!d) continue;
      if (!nl || gc.lp_slot[r] < 0) {
        d->n_top = -1;
        continue;
      }
      const float* o = gc.h_lp_out + (size_t)gc.lp_slot[r] * LOGPROB_OUT_WORDS;
      memcpy(d, o, sizeof(aha_token_logprobs));
      if (!sampled || ch.mode[r] == GREEDY) continue;
      const uint32_t tok = h_tok[r];
      float x = 0.f;
      bool found = false;
      if (gc.lp_fb[r] >= 0) {
        x = ch.h_fb[(size_t)gc.lp_fb[r] * V + tok];
        found = true;
      } else {
        const float* so = ch.h_sout + (size_t)ch.slot[r] * SAMPLE_OUT_WORDS;
        const uint32_t* ids = reinterpret_cast<const uint32_t*>(so + 66);
        const int k = ch.h_stab[(size_t)ch.slot[r] * SAMPLE_ROW_WORDS + SAMPLE_ROW_K];
        for (int i = 0; i < k && !found; ++i)
          if (ids[i] == tok) x = o[LOGPROB_OUT_RAW + i], found = true;
      }
      if (!found) {
        set_error("generate_batch_logprobs: the sampled token is not among the row's candidates");
        return AHA_ERR_STATE;
      }
      d->logprob = (x - o[LOGPROB_OUT_M]) - o[LOGPROB_OUT_LOGS];
    }
    return AHA_OK;
  };
  if (gc.row_logits) {
    for (int r = 0; r < R; ++r)
      if (gc.row_logits[r]) AHA_HIP_CHECK(hipMemcpyAsync(gc.row_logits[r], gc.logits + (size_t)r * V, (size_t)V * 4, hipMemcpyDeviceToHost, st));
  } else if (gc.step_logits_out) {
    for (int r = 0; r < R; ++r)
      AHA_HIP_CHECK(hipMemcpyAsync(gc.step_logits_out + ((size_t)seqs[r] * max_new + gc.n_out[seqs[r]]) * V, gc.logits + (size_t)r * V,
                                   (size_t)V * 4, hipMemcpyDeviceToHost, st));
  }
  AHA_HIP_CHECK(hipMemcpyAsync(h_tok, tok_dev, (size_t)R * 4, hipMemcpyDeviceToHost, st));
  AHA_HIP_CHECK(hipStreamSynchronize(st));
  if (!sampled) return lp_finish();
  ch.fb_rows.clear();
  for (int r = 0; r < R; ++r) {
    if (ch.mode[r] == GREEDY) continue;
    const int j = seqs[r];
    if (ch.mode[r] == CAND) {
      const float* o = ch.h_sout + (size_t)ch.slot[r] * SAMPLE_OUT_WORDS;
      const int k = ch.h_stab[(size_t)ch.slot[r] * SAMPLE_ROW_WORDS + SAMPLE_ROW_K];
      const int prc = sampler_pick(ch.samplers[j], o, reinterpret_cast<const uint32_t*>(o + 66), k, o[64], o[65], nullptr, (size_t)V,
                                   gen_seq_tokens(gc, j), gc.n_out[j], &h_tok[r]);
      if (prc < 0) return prc;
      if (prc == AHA_OK) continue;
    }
    ch.fb_rows.push_back(r);
  }
  if (!ch.fb_rows.empty()) {   // rows whose candidates cannot decide: their full logits rows, one more sync
    for (size_t f = 0; f < ch.fb_rows.size(); ++f)
      AHA_HIP_CHECK(hipMemcpyAsync(ch.h_fb + f * V, gc.logits + (size_t)ch.fb_rows[f] * V, (size_t)V * 4, hipMemcpyDeviceToHost, st));
    AHA_HIP_CHECK(hipStreamSynchronize(st));
    for (size_t f = 0; f < ch.fb_rows.size(); ++f) {
      const int r = ch.fb_rows[f], j = seqs[r];
      if (nl) gc.lp_fb[r] = (int)f;
      const int prc = sampler_pick(ch.samplers[j], nullptr, nullptr, 0, 0.f, 0.f, ch.h_fb + f * V, (size_t)V, gen_seq_tokens(gc, j),
                                   gc.n_out[j], &h_tok[r]);
      if (prc != AHA_OK) return prc < 0 ? prc : AHA_ERR_STATE;
    }
  }
  AHA_HIP_CHECK(hipMemcpyAsync(tok_dev, h_tok, (size_t)R * 4, hipMemcpyHostToDevice, st));
  return lp_finish();
}

// One decode step's device work over the R rows of the uploaded row table gc.rowtab: the tokens tok_in embedded (with their rope rows),
// every layer, then the head -> tok_out.  kv_tokens: the rows' cache lengths summed (the profile's bytes); max_split: their largest split.
// split_append (draft-and-verify steps): rows of one sequence at consecutive positions -- every row's K/V is appended by a launch of its
// own in front of the attention, whose own append is compiled out, so row i + 1 reads row i's token from the pages.
static void gen_decode_step(aha_model* m, GenCall& gc, int R, int max_split, double kv_tokens, const uint32_t* tok_in, uint32_t* tok_out,
                            bool split_append = false) {
  const aha_model_desc& c = m->desc;
  hipStream_t st = m->stream;
  const int H = c.hidden_size, I = c.intermediate_size, nh = c.num_attention_heads, kvh = c.num_key_value_heads;
  const int nq = nh * 128, nkv = kvh * 128;
  {
    ProfScope ps(m, "elem", (double)R * H * 4, 0);
    launch_gen_embed(m->embed, tok_in, gc.rowtab, R, gc.x, H, m->d_inv_freq, m->d_axis_map, gc.rope, st);
  }
  for (int li = 0; li < c.num_hidden_layers; ++li) {
    const LayerWeights& Lw = m->layers[li];
    {   // h = RMSNorm(x); qkv = h Wqkv^T                      (qwen3/model.rs:79, modules.rs:538-552)
      {
        ProfScope ps(m, "elem", (double)R * H * 4, 0);
        launch_rmsnorm_rows(gc.x, Lw.in_norm, gc.h, R, H, H, H, c.rms_norm_eps, st);
      }
      GemvRowsArgs a{};
      a.W = Lw.wqkv; a.x = gc.h; a.ldx = H; a.y = gc.qkv; a.ldy = nq + 2 * nkv; a.N = nq + 2 * nkv; a.K = H;
      gemv_rows_groups(m, a, GEMV_STORE, R, gc.ws, &Lw.q_wqkv);
    }
    {   // q/k norm + rope + KV append + attention of every row over its own pages (modules.rs:544-574, 757-813)
      AttnDecodeBatchArgs b{};
      b.qkv = gc.qkv; b.q_norm_w = Lw.q_norm; b.k_norm_w = Lw.k_norm; b.rope = gc.rope; b.page_ptrs = gc.dec_pages ? gc.dec_pages : m->d_page_ptrs;
      b.layer_off = (uint64_t)li * m->layer_stride; b.row_tab = gc.rowtab; b.part_o = gc.part_o; b.part_ml = gc.part_ml; b.o = gc.attn;
      b.head_ctr = gc.ctr; b.ctr_step = li + 1; b.nh = nh; b.kvh = kvh; b.max_nsplit = gc.max_nsplit; b.eps = c.rms_norm_eps;
      b.scale = m->attn_scale;
      if (split_append) {
        ProfScope ps(m, "kv_append_rows", (double)R * nkv * 2 * 4, 0);
        launch_kv_append_rows(b, R, st);
      }
      ProfScope ps(m, "attn_decode_batch", kv_tokens * 2 * nkv * 2 + (double)R * (nq + 2 * nkv) * 2, 4.0 * kv_tokens * nq);
      launch_attn_decode_batch(b, R, max_split, st, !split_append);
    }
    {   // x = x + attn Wo^T                                    (modules.rs:577, qwen3/model.rs:81)
      GemvRowsArgs a{};
      a.W = Lw.wo; a.x = gc.attn; a.ldx = nq; a.residual = gc.x; a.y = gc.x; a.ldy = H; a.N = H; a.K = nq;
      gemv_rows_groups(m, a, GEMV_RESIDUAL, R, gc.ws, &Lw.q_wo);
    }
    {   // act = silu(h Wg^T) * (h Wu^T), h = RMSNorm(x)        (qwen3/model.rs:83, modules.rs:81-84)
      {
        ProfScope ps(m, "elem", (double)R * H * 4, 0);
        launch_rmsnorm_rows(gc.x, Lw.post_norm, gc.h, R, H, H, H, c.rms_norm_eps, st);
      }
      GemvRowsArgs a{};
      a.W = Lw.wgu; a.x = gc.h; a.ldx = H; a.y = gc.act; a.ldy = I; a.N = 2 * I; a.K = H;
      gemv_rows_groups(m, a, GEMV_SILU_MUL, R, gc.ws, &Lw.q_wgu);
    }
    {   // x = x + act Wd^T                                     (modules.rs:85, qwen3/model.rs:86)
      GemvRowsArgs a{};
      a.W = Lw.wdown; a.x = gc.act; a.ldx = I; a.residual = gc.x; a.y = gc.x; a.ldy = H; a.N = H; a.K = I;
      gemv_rows_groups(m, a, GEMV_RESIDUAL, R, gc.ws, &Lw.q_wdown);
    }
  }
  gen_head(m, gc, 0, R, tok_out);
}

static bool is_stop(const aha_model_desc& c, uint32_t t) {
  for (int e = 0; e < c.n_stop_tokens; ++e)
    if (t == c.stop_tokens[e]) return true;
  return false;
}

// ---- draft-and-verify greedy decoding (aha_hip_generate_batch_spec) ------------------------------------------------------------------
// The decode loop of model_generate_batch with up to max_draft draft tokens per sequence riding along as rows of the same step: a sequence
// whose cache holds p tokens and whose last token is g contributes rows (g, d1 .. dk) at cache lengths p + 1 .. p + 1 + k on the same pages.
// Row i's logits are those of plain greedy decoding at its position as long as d1 .. di are the tokens greedy decoding chose there (row
// isolation of gemv_rows, the unchanged attention body), which is exactly what spec_accept_rows_kernel checks: it keeps the longest
// confirmed prefix and the token that follows it.  K/V of rejected rows stay in slots >= the new cache length: every reader masks by its
// kv_len, and the slots are overwritten by the appends of the next steps before any kv_len reaches them.
// Rows of a step: every active sequence's mandatory row, then drafts in submission order until the total reaches the next multiple of
// GEN_ROW_GROUP at or above the number of active sequences -- no gemv_rows group is added by speculation.
// The input tokens of the rows are known on the host (the last emitted token, the drafts): they travel in word GEN_ROW_TOK of the row
// table, which doubles as the step's token vector; the sequences' (first row, drafts) pairs sit behind the rows, one upload per step.
// sp: the call's options, of which the spec fields are read.
static int spec_decode_loop(aha_model* m, GenCall& gc, const GenOptions& sp, const uint32_t* ids, const size_t* seq_lens,
                            const std::vector<size_t>& pred_off, const std::vector<int64_t>& page0, const std::vector<int64_t>& rope_delta,
                            std::vector<int>& active, float* logits_out) {
  const aha_model_desc& c = m->desc;
  hipStream_t st = m->stream;
  const int n = gc.n, V = gc.V;
  const size_t max_new = gc.max_new;
  // context of the proposer: prompt || generated
  std::vector<std::vector<uint32_t>> ctx(n);
  {
    size_t off = 0;
    for (int j = 0; j < n; off += seq_lens[j], ++j) {
      ctx[j].reserve(seq_lens[j] + max_new);
      ctx[j].assign(ids + off, ids + off + seq_lens[j]);
      ctx[j].push_back(gc.tokens_out[(size_t)j * max_new]);
    }
  }
  std::vector<unsigned> ctr_acc((size_t)gc.rows, 0u);   // per row slot: the rows of a step change from step to step
  std::vector<int> row0(n), ndraft(n);
  uint32_t draft[SPEC_MAX_DRAFT];
  while (!active.empty()) {
    const int nact = (int)active.size();
    int extra = (nact + GEN_ROW_GROUP - 1) / GEN_ROW_GROUP * GEN_ROW_GROUP - nact;
    int R = 0, n_drafts = 0;
    GenStepRows sr;
    for (int a = 0; a < nact; ++a) {
      const int j = active[a];
      const size_t t_gen = gc.n_out[j];
      size_t k = 0;
      const size_t room = std::min<size_t>((size_t)extra, max_new - t_gen - 1);   // t + 1 + |draft| <= max_new: the cache stays in its pages
      if (room > 0) {
        const uint32_t* pred = sp.predictions ? sp.predictions + pred_off[j] : nullptr;
        spec_propose(*sp.spec, ctx[j].data(), ctx[j].size(), seq_lens[j], pred, pred ? sp.prediction_lens[j] : 0, draft, &k);
        k = std::min(k, room);
      }
      extra -= (int)k;
      n_drafts += (int)k;
      row0[a] = R;
      ndraft[a] = (int)k;
      for (int i = 0; i <= (int)k; ++i, ++R)   // the cache after row i's append: the prompt, the tokens so far and the drafts before it
        gen_write_row(m, gc, sr, R, page0[j], (int)(seq_lens[j] + t_gen) + i, rope_delta[j], ctr_acc[R], R * GEN_ROW_WORDS + GEN_ROW_TOK, R,
                      (int32_t)(i == 0 ? ctx[j].back() : draft[i - 1]));
    }
    int32_t* h_seq = gc.h_rowtab + (size_t)R * GEN_ROW_WORDS;
    for (int a = 0; a < nact; ++a) h_seq[a * SPEC_SEQ_WORDS + SPEC_SEQ_ROW0] = row0[a], h_seq[a * SPEC_SEQ_WORDS + SPEC_SEQ_NDRAFT] = ndraft[a];
    const size_t words = (size_t)R * GEN_ROW_WORDS + (size_t)nact * SPEC_SEQ_WORDS;
    AHA_HIP_CHECK(hipMemcpyAsync(gc.rowtab, gc.h_rowtab, words * 4, hipMemcpyHostToDevice, st));
    // a step without drafts is generate_batch's step: one attention launch per layer, the fused append
    gen_decode_step(m, gc, R, sr.max_split, sr.kv_tokens, reinterpret_cast<const uint32_t*>(gc.rowtab), gc.tok[0], n_drafts > 0);
    {
      ProfScope ps(m, "spec_accept_rows", (double)R * 8, 0);
      launch_spec_accept_rows(gc.tok[0], gc.rowtab, gc.rowtab + (size_t)R * GEN_ROW_WORDS, nact, gc.spec_out, st);
    }
    AHA_HIP_CHECK(hipGetLastError());
    AHA_HIP_CHECK(hipMemcpyAsync(gc.h_spec_out, gc.spec_out, (size_t)nact * SPEC_OUT_WORDS * 4, hipMemcpyDeviceToHost, st));
    AHA_HIP_CHECK(hipStreamSynchronize(st));
    if (sp.stats) sp.stats->decode_steps += 1, sp.stats->rows += (size_t)R, sp.stats->proposed += (size_t)n_drafts;
    std::vector<int> next;
    for (int a = 0; a < nact; ++a) {
      const int j = active[a];
      const uint32_t* o = gc.h_spec_out + (size_t)a * SPEC_OUT_WORDS;
      const int emitted = (int)o[SPEC_OUT_COUNT];
      if (emitted < 1 || emitted > ndraft[a] + 1 || (int)o[SPEC_OUT_LAST_ROW] != row0[a] + emitted - 1) {
        set_error("generate_batch_spec: the accept step returned an impossible run");
        return AHA_ERR_STATE;
      }
      // stop tokens and max_new in order: the run is cut at, and keeps, the first stop token
      int kept = 0;
      bool done = false;
      while (kept < emitted && !done) {
        const uint32_t t = o[SPEC_OUT_TOKENS + kept++];
        gc.tokens_out[(size_t)j * max_new + gc.n_out[j]++] = t;
        ctx[j].push_back(t);
        done = is_stop(c, t) || gc.n_out[j] == max_new;
      }
      const size_t acc = (size_t)std::min(kept, emitted - 1);   // drafts among the kept tokens (the run's last token is the row's own choice)
      if (sp.n_proposed) sp.n_proposed[j] += (size_t)ndraft[a];
      if (sp.n_accepted) sp.n_accepted[j] += acc;
      if (sp.stats) sp.stats->accepted += acc;
      if (done) {   // the logits that chose the last kept token
        if (logits_out)
          AHA_HIP_CHECK(hipMemcpy(logits_out + (size_t)j * V, gc.logits + (size_t)(row0[a] + kept - 1) * V, (size_t)V * 4, hipMemcpyDeviceToHost));
      } else {
        next.push_back(j);
      }
    }
    active.swap(next);
  }
  return AHA_OK;
}

constexpr aha_sampling_params GREEDY_PARAMS{0.f, 1.f, 0, 1.f, 64, 0u, 299792458ull};   // ArgMax, no penalty: the device argmax

// The one implementation behind every aha_hip_generate_batch* entry; GenOptions (model.h) names what a call carries.  A new per-request
// option is added in three places: a GenOptions field, its device-free check in capi.hip's gen_options_check, and its use here.
// o.params == nullptr: greedy, the device argmax.  Otherwise one sampler per sequence; the step's tokens are then picked on the host after
// the batched candidate step, and written back into the token vector the next step's embedding gather reads.  o.logits_out: each sequence's
// last logits; o.step_logits_out (greedy or sampled): every step's logits.  o.mm (may be null): per sequence null or its images / videos
// -- Qwen3-VL positions (get_rope_index of the sequence alone), the tower per prefill pass, DeepStack in the packed layers, and decode
// positions kv_len - 1 + the sequence's rope_delta (qwen3vl/model.rs:1235-1264); m->rope_delta is neither read nor written.
int model_generate_batch(aha_model* m, const uint32_t* ids, const size_t* seq_lens, size_t n_seqs, size_t max_new, size_t max_tokens_per_pass,
                         const GenOptions& o, uint32_t* tokens_out, size_t* n_out) {
  const aha_sampling_params* params = o.params;
  const aha_logit_adjust* adjust = o.adjust;
  float* const logits_out = o.logits_out;
  const aha_model_desc& c = m->desc;
  if (!ids || !seq_lens || !tokens_out || !n_out) {
    set_error("generate_batch: null input_ids / seq_lens / tokens_out / n_out");
    return AHA_ERR_INVALID;
  }
  if (n_seqs == 0) {
    set_error("generate_batch: empty batch (n_seqs == 0)");
    return AHA_ERR_INVALID;
  }
  if (max_new == 0) {
    set_error("generate_batch: max_new must be at least 1");
    return AHA_ERR_INVALID;
  }
  if (c.arch != AHA_ARCH_QWEN3 && c.arch != AHA_ARCH_QWEN3VL && c.arch != AHA_ARCH_QWEN3ASR) {
    set_error("generate_batch: Qwen3, Qwen3-VL and Qwen3-ASR only");
    return AHA_ERR_UNSUPPORTED;
  }
  if (m->tp_size > 1 || m->cp_size > 1 || c.head_dim != 128) {
    set_error("generate_batch: a single-GPU model with head_dim 128 only (no tensor / context parallelism)");
    return AHA_ERR_UNSUPPORTED;
  }
  if (n_seqs > ((size_t)1 << 20) || max_new > ((size_t)1 << 20)) {
    set_error("generate_batch: at most 2^20 sequences and 2^20 new tokens");
    return AHA_ERR_INVALID;
  }
  int rc = check_batch_ids(c, "generate_batch", ids, seq_lens, n_seqs, max_new);
  if (rc) return rc;
  // aha_logit_adjust: checked against the vocabulary; all inactive = no adjust at all; a greedy call (params == nullptr) with an active
  // one gets ArgMax samplers, whose rows without a live addend stay the device argmax
  std::vector<aha_sampling_params> greedy_params;
  if (adjust) {
    bool any = false;
    for (size_t j = 0; j < n_seqs; ++j) {
      std::string why;
      if (logit_adjust_check(&adjust[j], (size_t)c.vocab_size, &why)) {
        set_error("generate_batch_adjusted: adjust of sequence " + std::to_string(j) + ": " + why);
        return AHA_ERR_INVALID;
      }
      any |= logit_adjust_active(&adjust[j]);
    }
    if (!any) adjust = nullptr;
  }
  if ((adjust || o.mask_fn) && !params) {   // (a mask callback likewise: a row it leaves unmasked stays the device argmax)
    greedy_params.assign(n_seqs, GREEDY_PARAMS);
    params = greedy_params.data();
  }
  std::vector<size_t> pred_off(n_seqs, 0);
  if (o.spec && o.predictions) {
    size_t off = 0;
    for (size_t j = 0; j < n_seqs; off += o.prediction_lens[j], ++j) {
      pred_off[j] = off;
      for (size_t i = 0; i < o.prediction_lens[j]; ++i)
        if (o.predictions[off + i] >= (uint32_t)c.vocab_size) {
          set_error("generate_batch_spec: prediction id out of range in sequence " + std::to_string(j) + " at position " + std::to_string(i));
          return AHA_ERR_INVALID;
        }
    }
  }
  const bool spec_on = o.spec && o.spec->max_draft > 0;
  if (o.spec) {
    if (o.stats) *o.stats = aha_spec_stats{0, 0, 0, 0};
    for (size_t j = 0; j < n_seqs; ++j) {
      if (o.n_proposed) o.n_proposed[j] = 0;
      if (o.n_accepted) o.n_accepted[j] = 0;
    }
  }
  std::vector<std::vector<int32_t>> pos3(n_seqs);
  std::vector<int64_t> rope_delta(n_seqs, 0);
  if (o.mm && (rc = check_mm_requests(m, ids, seq_lens, n_seqs, o.mm, pos3, rope_delta))) return rc;
  AHA_HIP_CHECK(hipSetDevice(m->ctx->device));
  if ((rc = model_clear_cache(m))) return rc;
  ClearCacheGuard guard{m};
  hipStream_t st = m->stream;
  const int n = (int)n_seqs, g = c.num_attention_heads / c.num_key_value_heads, V = c.vocab_size;
  // every sequence's pages, reserved up front: ceil((len + max_new) / 64) consecutive logical pages
  std::vector<int64_t> page0(n);
  size_t npages = 0;
  for (int j = 0; j < n; ++j) {
    page0[j] = (int64_t)npages;
    npages += (seq_lens[j] + max_new + KV_PAGE_TOKENS - 1) / KV_PAGE_TOKENS;
  }
  if ((rc = model_ensure_pages(m, npages * KV_PAGE_TOKENS))) return rc;
  DevBufs bufs{st, {}, {}};
  GenCall gc;
  gc.n = n, gc.V = V, gc.H = c.hidden_size, gc.max_new = max_new;
  // draft-and-verify: a step's rows never pass the next multiple of GEN_ROW_GROUP at or above its sequences (the row budget)
  if (spec_on) gc.rows = (int)std::min<size_t>((size_t)(n + GEN_ROW_GROUP - 1) / GEN_ROW_GROUP * GEN_ROW_GROUP, (size_t)n * (1 + o.spec->max_draft));
  gc.tokens_out = tokens_out, gc.n_out = n_out, gc.step_logits_out = o.step_logits_out;
  GenChoice ch;
  size_t max_pass_pages = 0;
  for (int j = 0; j < n; ++j) {
    gc.max_nsplit = std::max(gc.max_nsplit, attn_decode_nsplit((int)(seq_lens[j] + max_new), g, m->max_nsplit));
    max_pass_pages += (seq_lens[j] + KV_PAGE_TOKENS - 1) / KV_PAGE_TOKENS;
  }
  if ((rc = gen_call_alloc(m, bufs, gc, max_pass_pages)) || (params && (rc = gen_choice_init(bufs, gc, params, ch, adjust)))) return rc;
  if (o.mask_fn) {
    if ((rc = gen_choice_mask_alloc(bufs, n, V, ch))) return rc;
    ch.mask_fn = o.mask_fn, ch.mask_user = o.mask_user;
  }
  if (o.top_logprobs) {
    gc.lp_top = o.top_logprobs, gc.logprobs_out = o.logprobs_out;
    if (std::any_of(o.top_logprobs, o.top_logprobs + n, [](int32_t t) { return t >= 0; }) && (rc = gen_logprob_alloc(bufs, gc))) return rc;
  }
  if (spec_on && ((rc = bufs.alloc(&gc.spec_out, (size_t)n * SPEC_OUT_WORDS)) || (rc = bufs.alloc_host(&gc.h_spec_out, (size_t)n * SPEC_OUT_WORDS))))
    return rc;

  // ---- prefill: packed passes ----
  // sequence j's cache starts on logical page page0[j]; its positions are its three M-RoPE rows pos3[j] (get_rope_index at offset 0) when
  // it has them, else arange; every sequence's last row -> gc.x row j -> its first token
  for (const PassRange& p : split_passes(seq_lens, n_seqs, max_tokens_per_pass)) {
    const int j0 = (int)p.j, n_seg = (int)(p.k - p.j);
    const PackedPass pp = plan_packed_pass(seq_lens + j0, n_seg, page0.data() + j0, pos3.data() + j0);
    if ((rc = gen_packed_pass(m, gc, pp, ids + p.off, o.mm ? o.mm + j0 : nullptr, j0, m->h_page_ptrs.data(), n_seg, j0))) return rc;
    AHA_HIP_CHECK(hipStreamSynchronize(st));   // the pass page table and the staging buffer are reused by the next pass
  }
  {
    std::vector<int> all(n);
    for (int j = 0; j < n; ++j) all[j] = j, n_out[j] = 0;
    if ((rc = gen_finish_step(m, gc, ch, all, gc.tok[0]))) return rc;
  }
  auto copy_logits = [&](int row, int j) -> int {
    if (logits_out) AHA_HIP_CHECK(hipMemcpy(logits_out + (size_t)j * V, gc.logits + (size_t)row * V, (size_t)V * 4, hipMemcpyDeviceToHost));
    return AHA_OK;
  };
  std::vector<int> active, src_row(n);
  for (int j = 0; j < n; ++j) {
    tokens_out[(size_t)j * max_new] = gc.h_tok[j];   // the first token never ends a sequence (generate.rs:131-134)
    n_out[j] = 1;
    src_row[j] = j;
    if (max_new == 1) {
      if ((rc = copy_logits(j, j))) return rc;
    } else {
      active.push_back(j);
    }
  }

  // ---- decode ----
  if (spec_on) return spec_decode_loop(m, gc, o, ids, seq_lens, pred_off, page0, rope_delta, active, logits_out);
  std::vector<unsigned> ctr_acc(n, 0u);
  int cur = 0;
  while (!active.empty()) {
    const int R = (int)active.size();
    if (o.spec && o.stats) o.stats->decode_steps += 1, o.stats->rows += (size_t)R;
    GenStepRows sr;
    for (int r = 0; r < R; ++r) {
      const int j = active[r];   // its cache after this step's append: the prompt and the tokens so far
      gen_write_row(m, gc, sr, r, page0[j], (int)(seq_lens[j] + n_out[j]), rope_delta[j], ctr_acc[r], src_row[j], r);
    }
    AHA_HIP_CHECK(hipMemcpyAsync(gc.rowtab, gc.h_rowtab, (size_t)R * GEN_ROW_WORDS * 4, hipMemcpyHostToDevice, st));
    gen_decode_step(m, gc, R, sr.max_split, sr.kv_tokens, gc.tok[cur], gc.tok[cur ^ 1]);
    AHA_HIP_CHECK(hipGetLastError());
    if ((rc = gen_finish_step(m, gc, ch, active, gc.tok[cur ^ 1]))) return rc;
    std::vector<int> next;
    for (int r = 0; r < R; ++r) {
      const int j = active[r];
      const uint32_t t = gc.h_tok[r];
      tokens_out[(size_t)j * max_new + n_out[j]++] = t;
      src_row[j] = r;
      if (is_stop(c, t) || n_out[j] == max_new) {
        if ((rc = copy_logits(r, j))) return rc;
      } else {
        next.push_back(j);
      }
    }
    active.swap(next);
    cur ^= 1;
  }
  return AHA_OK;
}

// ---- continuous batching engine (aha_hip_engine_*) ------------------------------------------------------------------------------
// generate_generic's stream (common/generate.rs:231-368) for requests that come and go: the engine owns the model's cache (kv_pages pages
// reserved up front, a free list) and max_running slots.  A slot owns the window [slot * kv_pages, + kv_pages) of the engine's device page
// table; a request takes ceil((len + max_new) / 64) pages from the free list when it is admitted, writes them into its slot's window, and
// gives them back when it ends or is cancelled.  A step = the prefill work (one gen_packed_pass: whole prompts of requests admitted this
// step in submission order under max_tokens_per_step, then at most one 64-aligned chunk of a long TEXT prompt, with its cache prefix in the
// attention: AttnPrefillArgs::seg_kv0) -> the first tokens of the prompts it completes, then one gen_decode_step over every request that
// had a first token before the step, then its gen_finish_step.  A request's bits are those of its prompt's packed pass (the same
// composition through generate_batch* gives the same bits: the decode rows are row-isolated) -- requests with images, video or audio are
// prefilled whole, never chunked.
// Split counters: slot s owns head_ctr block s (GEN_ROW_CTRROW) and ctr_acc[s], both reset to ctr_base when a slot is taken.  The kernel's
// "last split" test is prev + 1 == ctr0 + layer * nsplit in 32-bit unsigned arithmetic, so a counter that wraps past 2^32 still meets its
// target exactly once: a false match would need 2^32 arrivals inside one launch (aha_hip_engine_debug_ctr_base moves the base near the wrap
// point for the test).
// Requests that may draft (aha_hip_engine_submit_spec): a decode step's mandatory rows keep rows 0 .. R-1, the draft rows follow request by
// request (include/aha_hip.h has the scheduler).  Draft row d of a step owns head_ctr block max_running + d and ctr_acc[max_running + d],
// kept per row slot as in spec_decode_loop.  The accept step (spec_accept_split_kernel), its download and the draft rows' logits are queued
// in front of gen_finish_step's synchronisation; a step in which no row drafts is the step it was before such requests existed.
namespace {
struct EngReq {
  uint64_t id = 0;
  std::vector<uint32_t> ids;
  const aha_mm_input* mm = nullptr;   // the caller's, valid until the request's first token
  bool whole = false;                 // images / video / audio: prefilled whole
  std::vector<int32_t> pos3;          // (3, len) of an image / video request, else empty
  int64_t rope_delta = 0;
  aha_sampling_params params{};
  size_t max_new = 0, npages = 0, done = 0;   // done: prompt tokens prefilled
  int32_t top_logprobs = -1;          // aha_hip_engine_submit_logprobs (-1: no logprobs)
  aha_logit_adjust adjust{};          // aha_hip_engine_submit_adjusted: its arrays point into the two vectors below
  std::vector<uint32_t> bias_ids;
  std::vector<float> bias_vals;
  std::vector<uint32_t> mask;         // aha_hip_engine_submit_masked / set_mask while the request waits (empty: none); a running
                                      // request's words live in its slot's row of GenChoice::h_masks
  int slot = -1;
  bool started = false, cancel = false;
  std::vector<uint32_t> toks;         // capacity max_new: gen_finish_step reads the penalty context through a pointer to it
  // aha_hip_engine_submit_spec with max_draft > 0 (drafts: true): the proposer's config, the prediction (copied) and context
  // (prompt || generated, kept beside ids / toks because spec_propose wants it in one piece), the draft counts so far
  bool drafts = false;
  aha_spec_config spec{};
  std::vector<uint32_t> prediction, ctx;
  size_t n_proposed = 0, n_accepted = 0;
};
struct EngSpecCount {   // a request a step retired: what aha_hip_engine_request_spec answers until the next step begins
  uint64_t id;
  size_t n_proposed, n_accepted;
};
struct EngSeg {
  EngReq* q;
  int kv0, len;
};
}  // namespace
}  // namespace aha

struct aha_engine {
  aha_model* m = nullptr;
  size_t max_running = 0, kv_pages = 0, budget = 0, chunk = 0;
  uint64_t next_id = 1;
  std::deque<aha::EngReq*> waiting;
  std::vector<aha::EngReq*> slots;
  std::vector<std::vector<uint64_t>> slot_pages;
  std::vector<uint64_t> free_pages;   // page addresses; taken from the back
  std::vector<aha_engine_event> pending;   // cancellations of requests that never ran
  std::vector<unsigned> ctr_acc;
  unsigned ctr_base = 0;
  std::vector<size_t> n_out;          // per slot: tokens so far
  std::vector<uint32_t*> seq_tok;     // per slot: EngReq::toks
  std::vector<float*> row_logits;
  std::vector<int32_t> lp_top;        // per slot: its request's top_logprobs (-1: none)
  std::vector<aha_token_logprobs*> row_lp;
  aha::DevBufs bufs{nullptr, {}, {}};
  aha::GenCall gc;
  aha::GenChoice ch;
  uint64_t* d_win = nullptr;          // (max_running, kv_pages) page table of the slots
  uint32_t* d_tok_in = nullptr;       // a decode step's input tokens
  uint32_t* h_tok_in = nullptr;       // pinned
  size_t ctx_cap = 0, adj_cap = 0;
  // draft-and-verify requests (aha_hip_engine_submit_spec): a step's rows may reach row_cap = the row budget of max_running.  Draft row d
  // of a step (the d-th row behind the mandatory ones) owns head_ctr block max_running + d and ctr_acc[max_running + d]; the blocks are
  // set to ctr_base at creation and again by the first drafting step after aha_hip_engine_debug_ctr_base (draft_ctr_stale).
  size_t row_cap = 0;
  bool draft_ctr_stale = false;
  float* h_stage = nullptr;           // pinned (row_cap, vocab), from the first drafting step that reports logits: a drafting step's
                                      // rows come down here, as the events they belong to are known only after the accept step
  std::vector<aha_token_logprobs> lp_stage;   // the same for the rows' logprob entries
  aha_spec_stats spec_stats{};
  std::vector<aha::EngSpecCount> retired;
  ~aha_engine() {
    for (aha::EngReq* q : waiting) delete q;
    for (aha::EngReq* q : slots) delete q;
  }
};

namespace aha {

// a caller's mask: n_words == ceil(V / 32) and an allowed id below V, or the error `who` reports (non-zero)
static int rc_mask_check(const uint32_t* words, size_t n_words, size_t V, const char* who) {
  if (n_words != token_mask_words(V)) {
    set_error(std::string(who) + ": the mask has " + std::to_string(n_words) + " words, the vocabulary needs " + std::to_string(token_mask_words(V)));
    return AHA_ERR_INVALID;
  }
  if (!token_mask_any(words, V)) {
    set_error(std::string(who) + ": the mask allows no id below vocab_size");
    return AHA_ERR_INVALID;
  }
  return AHA_OK;
}

// The config's own rules (no model needed): the effective step budget and chunk
int engine_config_check(const aha_engine_config* cfg, size_t* budget_out, size_t* chunk_out) {
  if (!cfg) {
    set_error("engine_create: null config");
    return AHA_ERR_INVALID;
  }
  const size_t budget = cfg->max_tokens_per_step ? cfg->max_tokens_per_step : PACKED_PASS_ROWS;
  const size_t chunk = cfg->prefill_chunk ? cfg->prefill_chunk : budget / KV_PAGE_TOKENS * KV_PAGE_TOKENS;
  if (cfg->max_running < 1 || cfg->max_running > AHA_ENGINE_MAX_RUNNING || cfg->kv_pages < 1 || cfg->kv_pages > ((size_t)1 << 18) ||
      budget < (size_t)KV_PAGE_TOKENS || budget > ((size_t)1 << 24) || chunk < (size_t)KV_PAGE_TOKENS || chunk % KV_PAGE_TOKENS || chunk > budget) {
    set_error("engine_create: bad config (max_running 1 .. " + std::to_string(AHA_ENGINE_MAX_RUNNING) +
              ", kv_pages 1 .. 2^18, max_tokens_per_step 0 or >= 64, prefill_chunk 0 or a multiple of 64 within max_tokens_per_step)");
    return AHA_ERR_INVALID;
  }
  if (budget_out) *budget_out = budget;
  if (chunk_out) *chunk_out = chunk;
  return AHA_OK;
}

int engine_create(aha_model* m, const aha_engine_config* cfg, aha_engine** out) {
  const aha_model_desc& c = m->desc;
  size_t budget = 0, chunk = 0;
  if (int rc = engine_config_check(cfg, &budget, &chunk)) return rc;
  if (!out) {
    set_error("engine_create: null out");
    return AHA_ERR_INVALID;
  }
  if (m->engine) {
    set_error("engine_create: the model already has an engine");
    return AHA_ERR_STATE;
  }
  if (c.arch != AHA_ARCH_QWEN3 && c.arch != AHA_ARCH_QWEN3VL && c.arch != AHA_ARCH_QWEN3ASR) {
    set_error("engine_create: Qwen3, Qwen3-VL and Qwen3-ASR only");
    return AHA_ERR_UNSUPPORTED;
  }
  if (m->tp_size > 1 || m->cp_size > 1 || c.head_dim != 128) {
    set_error("engine_create: a single-GPU model with head_dim 128 only (no tensor / context parallelism)");
    return AHA_ERR_UNSUPPORTED;
  }
  if (!sample_shape_ok(c.vocab_size, 64)) {
    set_error("engine_create: vocabulary too large for the candidate step");
    return AHA_ERR_UNSUPPORTED;
  }
  AHA_HIP_CHECK(hipSetDevice(m->ctx->device));
  int rc;
  if ((rc = model_clear_cache(m)) || (rc = model_ensure_pages(m, cfg->kv_pages * KV_PAGE_TOKENS))) return rc;
  aha_engine* e = new aha_engine();
  e->m = m;
  e->max_running = cfg->max_running, e->kv_pages = cfg->kv_pages, e->budget = budget, e->chunk = chunk;
  e->bufs.st = m->stream;
  const int n = (int)e->max_running, kvh = c.num_key_value_heads;
  e->slots.assign(n, nullptr);
  e->slot_pages.resize(n);
  e->row_cap = (size_t)((n + GEN_ROW_GROUP - 1) / GEN_ROW_GROUP * GEN_ROW_GROUP);
  e->ctr_acc.assign((size_t)n + GEN_ROW_GROUP, 0u);   // the slots, then the draft rows of a step (fewer than GEN_ROW_GROUP)
  e->n_out.assign(n, 0);
  e->seq_tok.assign(n, nullptr);
  e->row_logits.assign(n, nullptr);
  e->lp_top.assign(n, -1);
  e->row_lp.assign(n, nullptr);
  for (size_t p = e->kv_pages; p > 0; --p) e->free_pages.push_back(m->h_page_ptrs[p - 1]);   // page 0 is taken first
  GenCall& gc = e->gc;
  gc.n = n, gc.V = c.vocab_size, gc.H = c.hidden_size, gc.max_new = 0;
  gc.rows = (int)e->row_cap, gc.seq_words = ENG_SEQ_WORDS, gc.ctr_rows = n + GEN_ROW_GROUP;
  gc.max_nsplit = attn_decode_nsplit((int)std::min<size_t>(e->kv_pages * KV_PAGE_TOKENS, (size_t)1 << 24), c.num_attention_heads / kvh, m->max_nsplit);
  gc.n_out = e->n_out.data(), gc.seq_tokens = e->seq_tok.data(), gc.row_logits = e->row_logits.data();
  gc.lp_top = e->lp_top.data(), gc.row_logprobs = e->row_lp.data();
  e->ctx_cap = (size_t)n * 64;
  if ((rc = gen_call_alloc(m, e->bufs, gc, 2 * e->kv_pages)) || (rc = gen_choice_alloc(e->bufs, gc, e->ctx_cap, (size_t)n, e->ch)) ||
      (rc = e->bufs.alloc(&e->d_win, (size_t)n * e->kv_pages, true)) || (rc = e->bufs.alloc(&e->d_tok_in, e->row_cap)) ||
      (rc = e->bufs.alloc_host(&e->h_tok_in, e->row_cap)) || (rc = e->bufs.alloc(&gc.spec_out, (size_t)n * SPEC_OUT_WORDS)) ||
      (rc = e->bufs.alloc_host(&gc.h_spec_out, (size_t)n * SPEC_OUT_WORDS)) || (logprob_shape_ok(gc.V) && (rc = gen_logprob_alloc(e->bufs, gc))) ||
      (rc = gen_choice_mask_alloc(e->bufs, n, gc.V, e->ch))) {
    delete e;
    model_clear_cache(m);
    return rc;
  }
  gc.dec_pages = e->d_win;
  e->ch.samplers.resize(n);
  m->engine = e;
  *out = e;
  return AHA_OK;
}

void engine_destroy(aha_engine* e) {
  if (!e) return;
  aha_model* m = e->m;
  hipSetDevice(m->ctx->device);
  delete e;   // DevBufs drains the stream before it frees
  m->engine = nullptr;
  model_clear_cache(m);
}

int engine_submit(aha_engine* e, const uint32_t* ids, size_t n_ids, const SubmitOptions& o, size_t max_new, uint64_t* req_id) {
  aha_model* m = e->m;
  const aha_model_desc& c = m->desc;
  const aha_mm_input* mm = o.mm;
  const aha_logit_adjust* adjust = o.adjust;
  if (o.mask && (rc_mask_check(o.mask, o.n_mask_words, (size_t)c.vocab_size, "engine_submit_masked"))) return AHA_ERR_INVALID;
  {
    std::string why;
    if (logit_adjust_check(adjust, (size_t)c.vocab_size, &why)) {
      set_error("engine_submit_adjusted: adjust: " + why);
      return AHA_ERR_INVALID;
    }
  }
  if (o.top_logprobs >= 0 && !e->gc.lp_tab) {
    set_error("engine_submit_logprobs: vocabulary too large for the logprob pass");
    return AHA_ERR_UNSUPPORTED;
  }
  if (!ids || !req_id) {
    set_error("engine_submit: null input_ids / req_id");
    return AHA_ERR_INVALID;
  }
  if (max_new == 0) {
    set_error("engine_submit: max_new must be at least 1");
    return AHA_ERR_INVALID;
  }
  if (max_new > ((size_t)1 << 20)) {
    set_error("engine_submit: at most 2^20 new tokens");
    return AHA_ERR_INVALID;
  }
  int rc = check_batch_ids(c, "engine_submit", ids, &n_ids, 1, max_new);
  if (rc) return rc;
  std::vector<std::vector<int32_t>> pos3(1);
  std::vector<int64_t> rope_delta(1, 0);
  if (mm && (rc = check_mm_requests(m, ids, &n_ids, 1, &mm, pos3, rope_delta))) return rc;
  for (size_t i = 0; o.spec && o.prediction && i < o.n_prediction; ++i)
    if (o.prediction[i] >= (uint32_t)c.vocab_size) {
      set_error("engine_submit_spec: prediction id out of range at position " + std::to_string(i));
      return AHA_ERR_INVALID;
    }
  const size_t npages = (n_ids + max_new + KV_PAGE_TOKENS - 1) / KV_PAGE_TOKENS;
  if (npages > e->kv_pages) {
    set_error("engine_submit: the request needs " + std::to_string(npages) + " pages, the engine has " + std::to_string(e->kv_pages));
    return AHA_ERR_OOM;
  }
  EngReq* q = new EngReq();
  q->id = e->next_id++;
  q->ids.assign(ids, ids + n_ids);
  const bool vis = mm && (mm->n_images > 0 || mm->n_videos > 0);
  q->mm = mm && (vis || m->audio) ? mm : nullptr;
  q->whole = q->mm != nullptr;
  q->pos3 = std::move(pos3[0]);
  q->rope_delta = rope_delta[0];
  q->params = o.params ? *o.params : GREEDY_PARAMS;
  q->max_new = max_new;
  q->top_logprobs = o.top_logprobs;
  if (logit_adjust_active(adjust)) {   // copied: the caller's arrays need not outlive the call
    q->bias_ids.assign(adjust->bias_ids, adjust->bias_ids + adjust->n_bias);
    q->bias_vals.assign(adjust->bias_vals, adjust->bias_vals + adjust->n_bias);
    q->adjust = aha_logit_adjust{adjust->presence_penalty, adjust->frequency_penalty, q->bias_ids.data(), q->bias_vals.data(), adjust->n_bias};
  }
  if (o.mask) q->mask.assign(o.mask, o.mask + o.n_mask_words);
  if (o.spec && o.spec->max_draft > 0) {   // max_draft 0: an ordinary greedy request
    q->drafts = true;
    q->spec = *o.spec;
    if (o.prediction) q->prediction.assign(o.prediction, o.prediction + o.n_prediction);
    q->ctx.reserve(n_ids + max_new);
    q->ctx = q->ids;
  }
  q->npages = npages;
  q->toks.reserve(max_new);
  e->waiting.push_back(q);
  *req_id = q->id;
  return AHA_OK;
}

int engine_set_mask(aha_engine* e, uint64_t req_id, const uint32_t* words, size_t n_words) {
  const size_t V = (size_t)e->m->desc.vocab_size;
  if (words && rc_mask_check(words, n_words, V, "engine_set_mask")) return AHA_ERR_INVALID;
  auto drafts = [&](const EngReq* q) {   // a drafting step takes its tokens from the unmasked argmax: such a request has no mask
    if (q->drafts) set_error("engine_set_mask: request " + std::to_string(req_id) + " was submitted through engine_submit_spec, which takes no mask");
    return q->drafts;
  };
  for (EngReq* q : e->waiting)
    if (q->id == req_id) {
      if (drafts(q)) return AHA_ERR_INVALID;
      if (words) q->mask.assign(words, words + n_words);
      else q->mask.clear();
      return AHA_OK;
    }
  for (EngReq* q : e->slots)
    if (q && q->id == req_id && !q->cancel) {
      if (drafts(q)) return AHA_ERR_INVALID;
      // between steps the stream has drained: the slot's pinned words are free to change, and go up with the next candidate step
      if (words) memcpy(e->ch.h_masks + (size_t)q->slot * e->ch.mask_w, words, n_words * 4);
      e->ch.mask_state[q->slot] = words ? 2 : 0;
      return AHA_OK;
    }
  set_error("engine_set_mask: no waiting or running request " + std::to_string(req_id));
  return AHA_ERR_INVALID;
}

int engine_cancel(aha_engine* e, uint64_t req_id) {
  for (auto it = e->waiting.begin(); it != e->waiting.end(); ++it)
    if ((*it)->id == req_id) {
      e->pending.push_back(aha_engine_event{req_id, AHA_ENGINE_NO_TOKEN, AHA_ENGINE_EV_CANCELLED});
      delete *it;
      e->waiting.erase(it);
      return AHA_OK;
    }
  for (EngReq* q : e->slots)
    if (q && q->id == req_id) {
      q->cancel = true;
      return AHA_OK;
    }
  set_error("engine_cancel: no waiting or running request " + std::to_string(req_id));
  return AHA_ERR_INVALID;
}

int engine_stats(const aha_engine* e, aha_engine_stats* out) {
  out->waiting = e->waiting.size();
  out->running = 0;
  for (const EngReq* q : e->slots) out->running += q != nullptr;
  out->free_pages = e->free_pages.size();
  out->total_pages = e->kv_pages;
  return AHA_OK;
}

int engine_debug_ctr_base(aha_engine* e, uint32_t base) {
  e->ctr_base = base;
  e->draft_ctr_stale = true;   // the draft rows' blocks follow at the next step that drafts
  return AHA_OK;
}

// Whether a request that may draft is waiting or running: its steps may emit more than one event per request
static bool engine_may_draft(const aha_engine* e) {
  for (const EngReq* q : e->waiting)
    if (q->drafts) return true;
  for (const EngReq* q : e->slots)
    if (q && q->drafts) return true;
  return false;
}

// The events the next step may emit, cancellations included: the cap it asks for
size_t engine_max_events(const aha_engine* e) {
  size_t n = e->pending.size();
  for (const EngReq* q : e->slots) n += q && q->cancel;
  return n + (engine_may_draft(e) ? e->row_cap : e->max_running);
}

int engine_spec_stats(const aha_engine* e, aha_spec_stats* out) {
  *out = e->spec_stats;
  return AHA_OK;
}

int engine_request_spec(const aha_engine* e, uint64_t req_id, size_t* n_proposed, size_t* n_accepted) {
  for (const EngReq* q : e->slots)
    if (q && q->id == req_id) {
      *n_proposed = q->n_proposed, *n_accepted = q->n_accepted;
      return AHA_OK;
    }
  for (const EngSpecCount& r : e->retired)
    if (r.id == req_id) {
      *n_proposed = r.n_proposed, *n_accepted = r.n_accepted;
      return AHA_OK;
    }
  set_error("engine_request_spec: no running request " + std::to_string(req_id) + ", and none the last step ended");
  return AHA_ERR_INVALID;
}

static void engine_release(aha_engine* e, int s) {
  EngReq* q = e->slots[s];
  e->retired.push_back(EngSpecCount{q->id, q->n_proposed, q->n_accepted});
  std::vector<uint64_t>& pg = e->slot_pages[s];
  for (size_t i = pg.size(); i > 0; --i) e->free_pages.push_back(pg[i - 1]);
  pg.clear();
  e->slots[s] = nullptr;
  e->ch.samplers[s].adj = LogitAdjust{};   // the slot's bias copy and count table go with the request
  e->ch.samplers[s].mask = nullptr, e->ch.samplers[s].mask_words = 0;
  e->ch.mask_state[s] = 0;                 // and its mask: the slot's next request starts unmasked
  delete q;
}

// a waiting request into a free slot: its pages from the free list into the slot's window, its sampler, its counters reset
static int engine_admit(aha_engine* e, EngReq* q, int s) {
  aha_model* m = e->m;
  hipStream_t st = m->stream;
  std::vector<uint64_t>& pg = e->slot_pages[s];
  for (size_t i = 0; i < q->npages; ++i) {
    pg.push_back(e->free_pages.back());
    e->free_pages.pop_back();
  }
  q->slot = s;
  e->slots[s] = q;   // from here on a failure releases the slot and its pages with the request
  const int kvh = m->desc.num_key_value_heads;
  const std::vector<unsigned> base((size_t)kvh * 32, e->ctr_base);
  int rc = AHA_OK;
  if (hipMemcpyAsync(e->d_win + (size_t)s * e->kv_pages, pg.data(), pg.size() * 8, hipMemcpyHostToDevice, st) != hipSuccess ||
      hipMemcpyAsync(e->gc.ctr + (size_t)s * kvh * 32, base.data(), base.size() * 4, hipMemcpyHostToDevice, st) != hipSuccess ||
      hipStreamSynchronize(st) != hipSuccess) {   // (pageable sources)
    set_error("engine_step: uploading a slot's page window / counters failed");
    rc = AHA_ERR_HIP;
  }
  e->ctr_acc[s] = e->ctr_base;
  if (rc || (rc = host_sampler_init(e->ch.samplers[s], q->params))) {
    engine_release(e, s);
    return rc;
  }
  sampler_set_adjust(e->ch.samplers[s], &q->adjust);
  if (!q->mask.empty()) {   // the mask it was submitted with, or was given while it waited
    memcpy(e->ch.h_masks + (size_t)s * e->ch.mask_w, q->mask.data(), e->ch.mask_w * 4);
    e->ch.mask_state[s] = 2;
  }
  size_t need = 0, need_adj = 0;   // the penalty contexts and the addend lists of every slot's sampler
  for (int k = 0; k < (int)e->max_running; ++k) {
    const EngReq* o = k == s ? q : e->slots[k];
    if (o && e->ch.samplers[k].repeat_penalty != 1.0f) need += std::min<size_t>(o->max_new, (size_t)e->ch.samplers[k].repeat_last_n);
    if (o) need_adj += adjust_list_cap(e->ch.samplers[k], o->max_new, (size_t)m->desc.vocab_size);
  }
  if (need_adj > e->adj_cap) {   // grow the addend buffers the same way (the stream has drained)
    const size_t cap = std::max(need_adj, 2 * e->adj_cap);
    GenChoice grown;
    if ((rc = gen_choice_adj_alloc(e->bufs, cap, grown))) {
      engine_release(e, s);
      return rc;
    }
    e->ch.d_adj_id = grown.d_adj_id, e->ch.d_adj_val = grown.d_adj_val, e->ch.h_adj_id = grown.h_adj_id, e->ch.h_adj_val = grown.h_adj_val;
    e->adj_cap = cap;
  }
  if (need > e->ctx_cap) {   // grow the penalty-context buffers (the stream has drained)
    const size_t cap = std::max(need, 2 * e->ctx_cap);
    uint32_t *d = nullptr, *h = nullptr;
    if ((rc = e->bufs.alloc(&d, cap)) || (rc = e->bufs.alloc_host(&h, cap))) {
      engine_release(e, s);
      return rc;
    }
    e->ch.d_sctx = d, e->ch.h_sctx = h;
    e->ctx_cap = cap;
  }
  e->n_out[s] = 0;
  e->seq_tok[s] = q->toks.data();
  e->lp_top[s] = q->top_logprobs;
  return AHA_OK;
}

int engine_step(aha_engine* e, aha_engine_event* ev, size_t cap, size_t* n_ev, float* logits_out, aha_token_logprobs* logprobs_out) {
  aha_model* m = e->m;
  const aha_model_desc& c = m->desc;
  hipStream_t st = m->stream;
  GenCall& gc = e->gc;
  const int V = c.vocab_size;
  if (!ev || !n_ev) {
    set_error("engine_step: null events / n_ev");
    return AHA_ERR_INVALID;
  }
  *n_ev = 0;
  const size_t max_ev = engine_max_events(e);
  if (cap < max_ev) {
    set_error("engine_step: room for " + std::to_string(cap) + " events, a step may emit " + std::to_string(max_ev));
    return AHA_ERR_INVALID;
  }
  AHA_HIP_CHECK(hipSetDevice(m->ctx->device));
  e->retired.clear();   // the counts of what the previous step retired were kept until here
  size_t ne = 0;
  int n_first = 0;      // first-token events of this step
  auto emit = [&](uint64_t id, uint32_t tok, uint32_t flags) {
    if (logprobs_out && (flags & AHA_ENGINE_EV_CANCELLED)) logprobs_out[ne].n_top = -1;   // (a token's entry: gen_finish_step wrote it)
    ev[ne++] = aha_engine_event{id, tok, flags};
  };
  // 1. cancellations
  for (const aha_engine_event& p : e->pending) {
    emit(p.req_id, p.token, p.flags);
    e->retired.push_back(EngSpecCount{p.req_id, 0, 0});   // it ended in this step, without ever running
  }
  e->pending.clear();
  for (int s = 0; s < (int)e->max_running; ++s)
    if (e->slots[s] && e->slots[s]->cancel) {
      emit(e->slots[s]->id, AHA_ENGINE_NO_TOKEN, AHA_ENGINE_EV_CANCELLED);
      engine_release(e, s);
    }
  // 2. the decode rows: every request with a first token, in submission order
  std::vector<int> dec;
  for (int s = 0; s < (int)e->max_running; ++s)
    if (e->slots[s] && e->slots[s]->started) dec.push_back(s);
  std::sort(dec.begin(), dec.end(), [&](int a, int b) { return e->slots[a]->id < e->slots[b]->id; });
  // 3. the prefill pass: at most one chunk of the running long prompt, then admissions in FIFO order
  std::vector<EngSeg> whole;
  EngSeg chunk{nullptr, 0, 0};
  long long left = (long long)e->budget;
  for (EngReq* q : e->slots)
    if (q && !q->started) {   // a long prompt part-way through its prefill (at most one)
      const int len = (int)std::min(e->chunk, q->ids.size() - q->done);
      chunk = EngSeg{q, (int)q->done, len};
      left -= len;
    }
  int rc;
  while (!e->waiting.empty()) {
    EngReq* q = e->waiting.front();
    int s = 0;
    while (s < (int)e->max_running && e->slots[s]) ++s;
    if (s == (int)e->max_running || e->free_pages.size() < q->npages) break;
    const long long len = (long long)q->ids.size();
    EngSeg sg{q, 0, (int)len};
    if (len <= left || (q->whole && whole.empty() && !chunk.q)) {
      whole.push_back(sg);   // (a request with images / video / audio over the budget runs alone)
    } else if (!q->whole && len > (long long)e->budget && !chunk.q && left >= KV_PAGE_TOKENS) {   // only prompts over the whole budget
      sg.len = (int)std::min<long long>((long long)e->chunk, left / KV_PAGE_TOKENS * KV_PAGE_TOKENS);
      chunk = sg;
    } else {
      break;
    }
    left -= sg.len;
    e->waiting.pop_front();
    if ((rc = engine_admit(e, q, s))) return rc;   // (the request is gone, its pages back in the pool)
  }
  std::vector<EngSeg> segs = whole;
  if (chunk.q) segs.push_back(chunk);
  if (!segs.empty()) {
    const int n_seg = (int)segs.size();
    std::vector<size_t> lens(n_seg);
    std::vector<int64_t> page0(n_seg);
    std::vector<int32_t> kv0(n_seg);
    std::vector<std::vector<int32_t>> pos3(n_seg);
    std::vector<uint64_t> phys;   // the pass's "logical" pages: every segment's slot pages, back to back
    std::vector<uint32_t> ids;
    std::vector<const aha_mm_input*> mm(n_seg);
    bool any_kv0 = false;
    for (int j = 0; j < n_seg; ++j) {
      const EngSeg& sg = segs[j];
      lens[j] = (size_t)sg.len;
      kv0[j] = sg.kv0;
      any_kv0 |= sg.kv0 > 0;
      page0[j] = (int64_t)phys.size();
      const std::vector<uint64_t>& pg = e->slot_pages[sg.q->slot];
      phys.insert(phys.end(), pg.begin(), pg.end());
      pos3[j] = sg.q->pos3;
      mm[j] = sg.q->mm;
      ids.insert(ids.end(), sg.q->ids.begin() + sg.kv0, sg.q->ids.begin() + sg.kv0 + sg.len);
    }
    const PackedPass pp = plan_packed_pass(lens.data(), n_seg, page0.data(), pos3.data(), any_kv0 ? kv0.data() : nullptr);
    // the prompts this pass completes: their last rows -> gc rows 0 .. k-1 (the chunk, if it does not end its prompt, is the last segment)
    int k = n_seg;
    if (chunk.q && (size_t)(chunk.kv0 + chunk.len) < chunk.q->ids.size()) --k;
    if ((rc = gen_packed_pass(m, gc, pp, ids.data(), mm.data(), 0, phys.data(), k, 0))) return rc;
    for (int j = 0; j < n_seg; ++j) segs[j].q->done += (size_t)segs[j].len;
    n_first = k;
    if (k > 0) {
      std::vector<int> seqs(k);
      for (int j = 0; j < k; ++j) {
        seqs[j] = segs[j].q->slot;
        e->n_out[seqs[j]] = 0;
        e->row_logits[j] = logits_out ? logits_out + (ne + j) * (size_t)V : nullptr;
        e->row_lp[j] = logprobs_out ? logprobs_out + (ne + j) : nullptr;
      }
      if ((rc = gen_finish_step(m, gc, e->ch, seqs, gc.tok[0]))) return rc;
      for (int j = 0; j < k; ++j) {
        EngReq* q = segs[j].q;
        const uint32_t t = gc.h_tok[j];   // the first token never ends a sequence (generate.rs:131-134)
        q->toks.push_back(t);
        if (q->drafts) q->ctx.push_back(t);
        q->started = true;
        q->mm = nullptr;
        e->n_out[q->slot] = 1;
        emit(q->id, t, AHA_ENGINE_EV_FIRST | (q->max_new == 1 ? AHA_ENGINE_EV_LENGTH : 0u));
      }
    } else {
      AHA_HIP_CHECK(hipStreamSynchronize(st));
    }
  }
  // 4. one decode step over the rows that had a first token before this step
  std::vector<int> rows;
  for (int s : dec)
    if (e->slots[s]->toks.size() < e->slots[s]->max_new) rows.push_back(s);
  if (!rows.empty()) {
    const int R = (int)rows.size(), nslots = (int)e->max_running;
    // the draft rows (aha_hip_engine_step's scheduler): behind the R mandatory rows, granted in submission order while the step stays
    // inside its last gemv_rows group and inside the event cap its first tokens have already drawn on
    int extra = std::max(0, std::min((R + GEN_ROW_GROUP - 1) / GEN_ROW_GROUP * GEN_ROW_GROUP - R, (int)e->row_cap - n_first - R));
    std::vector<int> nd(R, 0), d0(R, 0);
    int D = 0, n_seq = 0;
    for (int r = 0; r < R && extra > 0; ++r) {
      const EngReq* q = e->slots[rows[r]];
      if (!q->drafts) continue;
      const size_t room = std::min<size_t>((size_t)extra, q->max_new - q->toks.size() - 1);   // t + 1 + |draft| <= max_new: the cache stays in its pages
      if (room == 0) continue;
      uint32_t draft[SPEC_MAX_DRAFT];
      size_t k = 0;
      spec_propose(q->spec, q->ctx.data(), q->ctx.size(), q->ids.size(), q->prediction.empty() ? nullptr : q->prediction.data(),
                   q->prediction.size(), draft, &k);
      k = std::min(k, room);
      if (k == 0) continue;
      nd[r] = (int)k, d0[r] = R + D;
      for (size_t i = 0; i < k; ++i) e->h_tok_in[R + D + (int)i] = draft[i];
      D += (int)k, extra -= (int)k, ++n_seq;
    }
    const bool staged = D > 0;   // the rows' events are known only after the accept step: logits and logprob entries come down to staging
    if (staged && e->draft_ctr_stale) {   // (after aha_hip_engine_debug_ctr_base only; the stream has drained)
      const std::vector<unsigned> base((size_t)GEN_ROW_GROUP * c.num_key_value_heads * 32, e->ctr_base);
      AHA_HIP_CHECK(hipMemcpy(gc.ctr + (size_t)nslots * c.num_key_value_heads * 32, base.data(), base.size() * 4, hipMemcpyHostToDevice));
      std::fill(e->ctr_acc.begin() + nslots, e->ctr_acc.end(), e->ctr_base);
      e->draft_ctr_stale = false;
    }
    if (staged && logits_out && !e->h_stage && (rc = e->bufs.alloc_host(&e->h_stage, e->row_cap * (size_t)V))) return rc;
    if (staged && logprobs_out) e->lp_stage.resize((size_t)R);
    GenStepRows sr;
    for (int r = 0; r < R; ++r) {
      const int s = rows[r];
      const EngReq* q = e->slots[s];   // its cache after this step's append: the prompt and the tokens so far, in the slot's page window
      gen_write_row(m, gc, sr, r, (int64_t)((size_t)s * e->kv_pages), (int)(q->ids.size() + e->n_out[s]), q->rope_delta, e->ctr_acc[s], r, s);
      e->h_tok_in[r] = q->toks.back();
      if (staged) {
        e->row_logits[r] = logits_out ? e->h_stage + (size_t)r * V : nullptr;
        e->row_lp[r] = logprobs_out ? &e->lp_stage[r] : nullptr;
      } else {
        e->row_logits[r] = logits_out ? logits_out + (ne + r) * (size_t)V : nullptr;
        e->row_lp[r] = logprobs_out ? logprobs_out + (ne + r) : nullptr;
      }
    }
    if (staged) {   // draft row i of a request: its cache one token longer per row, counters of its own, the draft in GEN_ROW_TOK
      int32_t* h_seq = gc.h_rowtab + (size_t)(R + D) * GEN_ROW_WORDS;
      for (int r = 0, a = 0; r < R; ++r) {
        if (!nd[r]) continue;
        const int s = rows[r];
        const EngReq* q = e->slots[s];
        for (int i = 0; i < nd[r]; ++i) {
          const int row = d0[r] + i, blk = nslots + row - R;
          gen_write_row(m, gc, sr, row, (int64_t)((size_t)s * e->kv_pages), (int)(q->ids.size() + e->n_out[s]) + 1 + i, q->rope_delta,
                        e->ctr_acc[blk], row, blk, (int32_t)e->h_tok_in[row]);
        }
        h_seq[a * ENG_SEQ_WORDS + ENG_SEQ_ROW] = r, h_seq[a * ENG_SEQ_WORDS + ENG_SEQ_DRAFT0] = d0[r], h_seq[a * ENG_SEQ_WORDS + ENG_SEQ_NDRAFT] = nd[r];
        ++a;
      }
    }
    const int RT = R + D;
    AHA_HIP_CHECK(hipMemcpyAsync(gc.rowtab, gc.h_rowtab, ((size_t)RT * GEN_ROW_WORDS + (size_t)n_seq * ENG_SEQ_WORDS) * 4, hipMemcpyHostToDevice, st));
    AHA_HIP_CHECK(hipMemcpyAsync(e->d_tok_in, e->h_tok_in, (size_t)RT * 4, hipMemcpyHostToDevice, st));
    // a step without drafts is the step it was before: one attention launch per layer, the fused append
    gen_decode_step(m, gc, RT, sr.max_split, sr.kv_tokens, e->d_tok_in, gc.tok[1], staged);
    if (staged) {   // the accept step, its download and the draft rows' logits in front of gen_finish_step's synchronisation
      {
        ProfScope ps(m, "spec_accept_split", (double)RT * 8, 0);
        launch_spec_accept_split(gc.tok[1], gc.rowtab, gc.rowtab + (size_t)RT * GEN_ROW_WORDS, n_seq, gc.spec_out, st);
      }
      AHA_HIP_CHECK(hipMemcpyAsync(gc.h_spec_out, gc.spec_out, (size_t)n_seq * SPEC_OUT_WORDS * 4, hipMemcpyDeviceToHost, st));
      if (logits_out)
        AHA_HIP_CHECK(hipMemcpyAsync(e->h_stage + (size_t)R * V, gc.logits + (size_t)R * V, (size_t)D * V * 4, hipMemcpyDeviceToHost, st));
    }
    AHA_HIP_CHECK(hipGetLastError());
    if ((rc = gen_finish_step(m, gc, e->ch, rows, gc.tok[1]))) return rc;
    e->spec_stats.decode_steps += 1, e->spec_stats.rows += (size_t)RT, e->spec_stats.proposed += (size_t)D;
    for (int r = 0, a = 0; r < R; ++r) {
      EngReq* q = e->slots[rows[r]];
      if (!nd[r]) {
        const uint32_t t = gc.h_tok[r];
        q->toks.push_back(t);
        if (q->drafts) q->ctx.push_back(t);
        e->n_out[rows[r]] = q->toks.size();
        const uint32_t f = (is_stop(c, t) ? AHA_ENGINE_EV_STOP : 0u) | (q->toks.size() == q->max_new ? AHA_ENGINE_EV_LENGTH : 0u);
        if (staged && logits_out) memcpy(logits_out + ne * (size_t)V, e->h_stage + (size_t)r * V, (size_t)V * 4);
        if (staged && logprobs_out) logprobs_out[ne] = e->lp_stage[r];
        emit(q->id, t, f);
        continue;
      }
      const uint32_t* o = gc.h_spec_out + (size_t)a++ * SPEC_OUT_WORDS;
      const int emitted = (int)o[SPEC_OUT_COUNT];
      if (emitted < 1 || emitted > nd[r] + 1 || (int)o[SPEC_OUT_LAST_ROW] != (emitted == 1 ? r : d0[r] + emitted - 2)) {
        set_error("engine_step: the accept step returned an impossible run");
        return AHA_ERR_STATE;
      }
      // stop tokens and max_new in order: the run is cut at, and keeps, the first stop token; event i's logits are those of the row that
      // chose its token -- the request's own row, then the verify row of draft i
      int kept = 0;
      bool done = false;
      while (kept < emitted && !done) {
        const uint32_t t = o[SPEC_OUT_TOKENS + kept];
        const int row = kept == 0 ? r : d0[r] + kept - 1;
        ++kept;
        q->toks.push_back(t);
        q->ctx.push_back(t);
        const bool stop = is_stop(c, t), length = q->toks.size() == q->max_new;
        done = stop || length;
        if (logits_out) memcpy(logits_out + ne * (size_t)V, e->h_stage + (size_t)row * V, (size_t)V * 4);
        if (logprobs_out) logprobs_out[ne].n_top = -1;   // a request that drafts has no logprobs
        emit(q->id, t, (stop ? AHA_ENGINE_EV_STOP : 0u) | (length ? AHA_ENGINE_EV_LENGTH : 0u));
      }
      e->n_out[rows[r]] = q->toks.size();
      const size_t acc = (size_t)std::min(kept, emitted - 1);   // drafts among the kept tokens (the run's last token is its row's own choice)
      q->n_proposed += (size_t)nd[r], q->n_accepted += acc;
      e->spec_stats.accepted += acc;
    }
  }
  // 5. retire what ended
  for (int s = 0; s < (int)e->max_running; ++s) {
    EngReq* q = e->slots[s];
    if (!q || !q->started) continue;
    const uint32_t last = q->toks.back();
    if (q->toks.size() >= q->max_new || (q->toks.size() > 1 && is_stop(c, last))) engine_release(e, s);
  }
  *n_ev = ne;
  return AHA_OK;
}

}  // namespace aha
