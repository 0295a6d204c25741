// Qwen3-ASR audio tower on the GPU and the audio-token scatter (A3).
//   create   <- Qwen3ASRAudioEncoder::new             /root/reference/src/models/qwen3_asr/model.rs:102-169
//   forward  <- Qwen3ASRAudioEncoder::forward         /root/reference/src/models/qwen3_asr/model.rs:171-226
//   frontend <- WhisperFeatureExtractor               /root/reference/src/models/feature_extractor/feature_extraction_whisper.rs:93-115
//   scatter  <- Qwen3ASRThinker::forward              /root/reference/src/models/qwen3_asr/model.rs:336-361
// Window / mel filter bank / twiddle tables are host-built exactly as the reference builds them (f32 arithmetic, f64 for
// the Hann window) and uploaded once; every tensor op runs in a HIP kernel.
#include <math.h>
#include <string.h>

#include <algorithm>

#include "audio.h"
#include "common.h"

namespace aha {

struct AudLayerW {
  void *ln1w, *ln1b, *qkv_w, *qkv_b, *out_w, *out_b, *ln2w, *ln2b, *fc1_w, *fc1_b, *fc2_w, *fc2_b;
};

struct AudioModel {
  int D = 0, nh = 0, hd = 0, ffn = 0, layers = 0, mels = 0, H = 0, out = 0, nwin = 0, fq = 0;
  void *c1w = nullptr, *c1b = nullptr, *c2w = nullptr, *c2b = nullptr, *c3w = nullptr, *c3b = nullptr, *conv_out = nullptr;
  std::vector<AudLayerW> L;
  void *lnp_w = nullptr, *lnp_b = nullptr, *p1w = nullptr, *p1b = nullptr, *p2w = nullptr, *p2b = nullptr;
  float *d_window = nullptr, *d_twid = nullptr, *d_melfb = nullptr;
  float scale = 0.f;
  // scratch (audio_ensure_scratch): frames, samples, 100-frame chunks, KV pages and clips of the largest tower pass so far
  size_t cap_frames = 0, cap_samples = 0, cap_chunks = 0, cap_pages = 0, cap_clips = 0;
  std::vector<void*> owned;
  float *d_samples = nullptr, *d_feat = nullptr, *d_fmax = nullptr;
  void *col = nullptr, *act_a = nullptr, *act_b = nullptr, *tok = nullptr, *x = nullptr, *h = nullptr, *qkv = nullptr, *attn = nullptr,
       *mlp = nullptr, *embeds = nullptr;
  int32_t* d_rows = nullptr;
  int64_t* d_clips = nullptr;                                            // log-mel clip table
  int32_t *d_chunks = nullptr, *d_seg = nullptr, *d_slot = nullptr;      // conv1 chunk table, attention {row0, len, page0} + items, KV slots
  uint32_t* d_src = nullptr;                                             // compaction: packed token row -> conv_out row
  void* page_store = nullptr;
  uint64_t* d_page_ptrs = nullptr;
  uint64_t page_bytes = 0;
  int64_t n_tok = 0;
};

static int aneed(const aha_tensor_view* w, size_t nw, const std::string& name, const aha_tensor_view** out) {
  *out = find_tensor(w, nw, name);
  if (!*out) {
    set_error("missing weight tensor: " + name);
    return AHA_ERR_MISSING_WEIGHT;
  }
  return AHA_OK;
}

static inline uint16_t f2bf_h(float f) {
  uint32_t u;
  memcpy(&u, &f, 4);
  if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x40u);
  u += 0x7fffu + ((u >> 16) & 1u);
  return (uint16_t)(u >> 16);
}
static inline float bf2f_h(uint16_t b) {
  const uint32_t u = (uint32_t)b << 16;
  float f;
  memcpy(&f, &u, 4);
  return f;
}
static int host_bf16(const aha_tensor_view* t, std::vector<uint16_t>& out) {
  int64_t n = 1;
  for (int i = 0; i < t->ndim; ++i) n *= t->shape[i];
  out.resize(n);
  if (t->on_device) {
    if (t->dtype != AHA_BF16) {
      set_error("device-resident weights must be bf16");
      return AHA_ERR_UNSUPPORTED;
    }
    AHA_HIP_CHECK(hipMemcpy(out.data(), t->data, n * 2, hipMemcpyDeviceToHost));
  } else if (t->dtype == AHA_BF16) memcpy(out.data(), t->data, n * 2);
  else if (t->dtype == AHA_F32)
    for (int64_t i = 0; i < n; ++i) out[i] = f2bf_h(((const float*)t->data)[i]);
  else {
    set_error(std::string("tensor ") + t->name + ": unsupported dtype for the audio tower");
    return AHA_ERR_UNSUPPORTED;
  }
  return AHA_OK;
}

// conv weight (Cout, Cin, 3, 3) -> GEMM weight (Cout, Kpad) with K ordered (kh, kw, cin) to match im2col_nhwc
static int upload_conv(aha_model* m, const aha_tensor_view* t, int cout, int cin, int kpad, void** out) {
  std::vector<uint16_t> src;
  int rc = host_bf16(t, src);
  if (rc) return rc;
  if ((int64_t)src.size() != (int64_t)cout * cin * 9) {
    set_error(std::string("tensor ") + t->name + " has the wrong number of elements");
    return AHA_ERR_SHAPE;
  }
  std::vector<uint16_t> dst((size_t)cout * kpad, 0);
  for (int o = 0; o < cout; ++o)
    for (int c = 0; c < cin; ++c)
      for (int k = 0; k < 9; ++k) dst[(size_t)o * kpad + (size_t)k * cin + c] = src[((size_t)o * cin + c) * 9 + k];
  if ((rc = dev_alloc(m, dst.size() * 2, out))) return rc;
  AHA_HIP_CHECK(hipMemcpy(*out, dst.data(), dst.size() * 2, hipMemcpyHostToDevice));
  return AHA_OK;
}

// ---- host tables of the Whisper frontend ---------------------------------------------------------------------------------
static float hz2mel(float f) {  // audio_utils.rs:1157-1175, Slaney
  float mels = 3.0f * f / 200.0f;
  if (f >= 1000.0f) mels = 15.0f + logf(f / 1000.0f) * (27.0f / logf(6.4f));
  return mels;
}
static float mel2hz(float m) {  // audio_utils.rs:1177-1195
  float fr = 200.0f * m / 3.0f;
  if (m >= 15.0f) fr = 1000.0f * expf((logf(6.4f) / 27.0f) * (m - 15.0f));
  return fr;
}
static std::vector<float> linspace_f(float a, float b, int n) {  // tensor_utils.rs:354-365
  std::vector<float> v(n);
  if (n == 1) {
    v[0] = a;
    return v;
  }
  const float step = (b - a) / (float)(n - 1);
  for (int i = 0; i < n; ++i) v[i] = a + (float)i * step;
  return v;
}

int audio_create(aha_model* m, const aha_tensor_view* w, size_t nw) {
  const aha_model_desc& c = m->desc;
  const std::string pre = "thinker.audio_tower.";
  if (c.aud_d_model % c.aud_attention_heads || c.aud_d_model / c.aud_attention_heads != 64) {
    set_error("audio tower: only head_dim 64 is supported (Qwen3-ASR encoder)");
    return AHA_ERR_UNSUPPORTED;
  }
  if (c.aud_downsample_hidden_size % 8 || c.aud_num_mel_bins != 128) {
    set_error("audio tower: downsample_hidden_size must be a multiple of 8 and num_mel_bins 128");
    return AHA_ERR_UNSUPPORTED;
  }
  AudioModel* a = new AudioModel();
  m->audio = a;
  a->D = c.aud_d_model; a->nh = c.aud_attention_heads; a->hd = 64; a->ffn = c.aud_ffn_dim; a->layers = c.aud_encoder_layers;
  a->mels = c.aud_num_mel_bins; a->H = c.aud_downsample_hidden_size; a->out = c.aud_output_dim; a->nwin = c.aud_n_window;
  a->fq = (((a->mels + 1) / 2 + 1) / 2 + 1) / 2;
  if (a->out != c.hidden_size) {
    set_error("audio output_dim must equal the text hidden_size");
    return AHA_ERR_SHAPE;
  }
  int rc;
  const aha_tensor_view* t;
  using S = std::vector<int64_t>;
#define LOADA(name, shape, dst)                  \
  if ((rc = aneed(w, nw, name, &t))) return rc;  \
  if ((rc = upload_tensor(m, t, shape, &(dst)))) return rc;
  if ((rc = aneed(w, nw, pre + "conv2d1.weight", &t))) return rc;
  if ((rc = upload_conv(m, t, a->H, 1, 16, &a->c1w))) return rc;
  LOADA(pre + "conv2d1.bias", (S{a->H}), a->c1b);
  if ((rc = aneed(w, nw, pre + "conv2d2.weight", &t))) return rc;
  if ((rc = upload_conv(m, t, a->H, a->H, 9 * a->H, &a->c2w))) return rc;
  LOADA(pre + "conv2d2.bias", (S{a->H}), a->c2b);
  if ((rc = aneed(w, nw, pre + "conv2d3.weight", &t))) return rc;
  if ((rc = upload_conv(m, t, a->H, a->H, 9 * a->H, &a->c3w))) return rc;
  LOADA(pre + "conv2d3.bias", (S{a->H}), a->c3b);
  LOADA(pre + "conv_out.weight", (S{a->D, (int64_t)a->H * a->fq}), a->conv_out);
  a->L.resize(a->layers);
  for (int i = 0; i < a->layers; ++i) {
    const std::string p = pre + "layers." + std::to_string(i) + ".";
    AudLayerW& L = a->L[i];
    LOADA(p + "self_attn_layer_norm.weight", (S{a->D}), L.ln1w);
    LOADA(p + "self_attn_layer_norm.bias", (S{a->D}), L.ln1b);
    // fused q|k|v projection: rows and bias concatenated (three Linear with bias, modules.rs:208-210)
    if ((rc = dev_alloc(m, (size_t)3 * a->D * a->D * 2, &L.qkv_w))) return rc;
    if ((rc = dev_alloc(m, (size_t)3 * a->D * 2, &L.qkv_b))) return rc;
    const char* names[3] = {"q_proj", "k_proj", "v_proj"};
    for (int j = 0; j < 3; ++j) {
      std::vector<uint16_t> tmp;
      if ((rc = aneed(w, nw, p + "self_attn." + names[j] + ".weight", &t))) return rc;
      if ((rc = host_bf16(t, tmp))) return rc;
      if ((int64_t)tmp.size() != (int64_t)a->D * a->D) { set_error("audio q/k/v weight shape"); return AHA_ERR_SHAPE; }
      AHA_HIP_CHECK(hipMemcpy((char*)L.qkv_w + (size_t)j * a->D * a->D * 2, tmp.data(), tmp.size() * 2, hipMemcpyHostToDevice));
      if ((rc = aneed(w, nw, p + "self_attn." + names[j] + ".bias", &t))) return rc;
      if ((rc = host_bf16(t, tmp))) return rc;
      if ((int64_t)tmp.size() != a->D) { set_error("audio q/k/v bias shape"); return AHA_ERR_SHAPE; }
      AHA_HIP_CHECK(hipMemcpy((char*)L.qkv_b + (size_t)j * a->D * 2, tmp.data(), tmp.size() * 2, hipMemcpyHostToDevice));
    }
    LOADA(p + "self_attn.out_proj.weight", (S{a->D, a->D}), L.out_w);
    LOADA(p + "self_attn.out_proj.bias", (S{a->D}), L.out_b);
    LOADA(p + "final_layer_norm.weight", (S{a->D}), L.ln2w);
    LOADA(p + "final_layer_norm.bias", (S{a->D}), L.ln2b);
    LOADA(p + "fc1.weight", (S{a->ffn, a->D}), L.fc1_w);
    LOADA(p + "fc1.bias", (S{a->ffn}), L.fc1_b);
    LOADA(p + "fc2.weight", (S{a->D, a->ffn}), L.fc2_w);
    LOADA(p + "fc2.bias", (S{a->D}), L.fc2_b);
  }
  LOADA(pre + "ln_post.weight", (S{a->D}), a->lnp_w);
  LOADA(pre + "ln_post.bias", (S{a->D}), a->lnp_b);
  LOADA(pre + "proj1.weight", (S{a->D, a->D}), a->p1w);
  LOADA(pre + "proj1.bias", (S{a->D}), a->p1b);
  LOADA(pre + "proj2.weight", (S{a->out, a->D}), a->p2w);
  LOADA(pre + "proj2.bias", (S{a->out}), a->p2b);
#undef LOADA
  // frontend tables
  {
    std::vector<float> win(400), tw(800), fb((size_t)201 * 128);
    for (int j = 0; j < 400; ++j) {
      const double i = (double)(1 - 400 + 2 * j);                       // audio_utils.rs:1071-1080 (symmetric Hann, f64)
      win[j] = (float)(0.5 + 0.5 * cos(M_PI * i / 399.0));
      tw[2 * j] = (float)cos(2.0 * M_PI * j / 400.0);
      tw[2 * j + 1] = (float)(-sin(2.0 * M_PI * j / 400.0));           // sign is irrelevant for the power spectrum
    }
    const std::vector<float> melpts = linspace_f(hz2mel(0.0f), hz2mel(8000.0f), 130);
    std::vector<float> filt(130);
    for (int i = 0; i < 130; ++i) filt[i] = mel2hz(melpts[i]);
    const std::vector<float> fft = linspace_f(0.0f, 8000.0f, 201);
    for (int k = 0; k < 201; ++k)
      for (int j = 0; j < 128; ++j) {                                   // audio_utils.rs:1197-1216, 1281-1290
        const float down = -1.0f * (filt[j] - fft[k]) / (filt[j + 1] - filt[j]);
        const float up = (filt[j + 2] - fft[k]) / (filt[j + 2] - filt[j + 1]);
        const float tri = std::max(std::min(down, up), 0.0f);
        fb[(size_t)k * 128 + j] = tri * (2.0f / (filt[j + 2] - filt[j]));
      }
    void* p;
    if ((rc = dev_alloc(m, win.size() * 4, &p))) return rc;
    a->d_window = (float*)p;
    if ((rc = dev_alloc(m, tw.size() * 4, &p))) return rc;
    a->d_twid = (float*)p;
    if ((rc = dev_alloc(m, fb.size() * 4, &p))) return rc;
    a->d_melfb = (float*)p;
    AHA_HIP_CHECK(hipMemcpy(a->d_window, win.data(), win.size() * 4, hipMemcpyHostToDevice));
    AHA_HIP_CHECK(hipMemcpy(a->d_twid, tw.data(), tw.size() * 4, hipMemcpyHostToDevice));
    AHA_HIP_CHECK(hipMemcpy(a->d_melfb, fb.data(), fb.size() * 4, hipMemcpyHostToDevice));
  }
  a->scale = 0.125f;  // 1/sqrt(64), exactly representable in bf16
  a->page_bytes = (uint64_t)2 * a->nh * KV_PAGE_TOKENS * a->hd * 2;
  return AHA_OK;
}

static void audio_free_scratch(AudioModel* a) {
  for (void* p : a->owned) hipFree(p);
  a->owned.clear();
  a->cap_frames = a->cap_samples = a->cap_chunks = a->cap_pages = a->cap_clips = 0;
}
void audio_destroy(aha_model* m) {
  if (!m->audio) return;
  audio_free_scratch(m->audio);
  delete m->audio;
  m->audio = nullptr;
}

// Scratch of one tower pass: `frames` feature columns, `samples` raw samples, `chunks` 100-frame windows (13 token rows each), `pages` KV
// pages (every clip starts on a page of its own: sum of ceil(n_tok_j / 64)), `clips` clips.  Grows only; frames round up to 1000.
static int audio_ensure_scratch(aha_model* m, size_t frames, size_t samples, size_t chunks, size_t pages, size_t clips) {
  AudioModel* a = m->audio;
  if (frames <= a->cap_frames && samples <= a->cap_samples && chunks <= a->cap_chunks && pages <= a->cap_pages && clips <= a->cap_clips)
    return AHA_OK;
  AHA_HIP_CHECK(hipStreamSynchronize(m->stream));
  const size_t cap = std::max((std::max(frames, a->cap_frames) + 999) / 1000 * 1000, (size_t)1000);
  const size_t C = std::max(std::max(chunks, a->cap_chunks), (cap + 99) / 100), win = 2 * (size_t)a->nwin;
  const size_t scap = std::max(std::max(samples, a->cap_samples), cap * 160);
  const size_t ntok = C * 13;
  const size_t pcap = std::max(std::max(pages, a->cap_pages), ntok / KV_PAGE_TOKENS + 2);
  const size_t ccap = std::max(std::max(clips, a->cap_clips), (size_t)16);
  audio_free_scratch(a);
  auto al = [&](size_t bytes, void** out, bool zero = false) -> int {
    void* p = nullptr;
    hipError_t e = hipMalloc(&p, bytes ? bytes : 16);
    if (e != hipSuccess) {
      set_error(std::string("audio scratch hipMalloc failed: ") + hipGetErrorString(e));
      return e == hipErrorOutOfMemory ? AHA_ERR_OOM : AHA_ERR_HIP;
    }
    if (zero) hipMemsetAsync(p, 0, bytes, m->stream);
    a->owned.push_back(p);
    *out = p;
    return AHA_OK;
  };
  int rc;
  const size_t H = a->H, r1 = C * 64 * ((win + 1) / 2), r2 = C * 32 * 25, r3 = C * 16 * 13;
  if ((rc = al((scap + 1024) * 4, (void**)&a->d_samples))) return rc;
  if ((rc = al((size_t)a->mels * cap * 4, (void**)&a->d_feat))) return rc;
  if ((rc = al(cap * 4, (void**)&a->d_fmax))) return rc;
  if ((rc = al(std::max(r1 * 16, std::max(r2, r3) * 9 * H) * 2, &a->col))) return rc;
  if ((rc = al(r1 * H * 2, &a->act_a))) return rc;
  if ((rc = al(r2 * H * 2, &a->act_b))) return rc;
  if ((rc = al(ntok * H * a->fq * 2, &a->tok))) return rc;
  if ((rc = al(ntok * a->D * 2, &a->x))) return rc;
  if ((rc = al(ntok * a->D * 2, &a->h))) return rc;
  if ((rc = al(ntok * 3 * a->D * 2, &a->qkv))) return rc;
  if ((rc = al(ntok * a->D * 2, &a->attn))) return rc;
  if ((rc = al(ntok * a->ffn * 2, &a->mlp))) return rc;
  if ((rc = al(ntok * a->out * 2, &a->embeds))) return rc;
  if ((rc = al(ntok * 4, (void**)&a->d_rows))) return rc;
  if ((rc = al(ccap * LOGMEL_CLIP_WORDS * 8, (void**)&a->d_clips))) return rc;
  if ((rc = al(C * 3 * 4, (void**)&a->d_chunks))) return rc;
  if ((rc = al((3 * ccap + 2 * pcap) * 4, (void**)&a->d_seg))) return rc;
  if ((rc = al(ntok * 4, (void**)&a->d_slot))) return rc;
  if ((rc = al(ntok * 4, (void**)&a->d_src))) return rc;
  if ((rc = al(pcap * a->page_bytes, &a->page_store, true))) return rc;
  if ((rc = al(pcap * 8, (void**)&a->d_page_ptrs))) return rc;
  std::vector<uint64_t> ptrs(pcap);
  for (size_t i = 0; i < pcap; ++i) ptrs[i] = (uint64_t)(uintptr_t)a->page_store + i * a->page_bytes;
  AHA_HIP_CHECK(hipMemcpy(a->d_page_ptrs, ptrs.data(), pcap * 8, hipMemcpyHostToDevice));
  a->cap_frames = cap, a->cap_samples = scap, a->cap_chunks = C, a->cap_pages = pcap, a->cap_clips = ccap;
  return AHA_OK;
}

// ln_w / ln_b / ln_out: a LayerNorm of the finished rows riding on the call (eps 1e-5) -- inside the reduce pass where the plan has one
// (gemm_splitk_reduce_layernorm_kernel, bit-identical to the two launches), a launch_layernorm_rows behind the GEMM otherwise
static void agemm(aha_model* m, const void* A, const void* W, void* C, int M, int N, int K, const void* bias, const void* residual,
                  int act, const void* ln_w = nullptr, const void* ln_b = nullptr, void* ln_out = nullptr) {
  GemmArgs g{};
  g.A = A; g.W = W; g.C = C; g.M = M; g.N = N; g.K = K; g.lda = K; g.ldw = K; g.ldc = N; g.bias = bias; g.residual = residual; g.act = act;
  if (ln_w) { g.norm_w = ln_w; g.norm_b = ln_b; g.norm_out = ln_out; g.norm_eps = 1e-5f; }
  ProfScope ps(m, "gemm", ((double)M * K + (double)N * K + (double)M * N * (residual ? 2 : 1)) * 2, 2.0 * M * N * K);
  launch_gemm(g, m->stream);
}

static int get_out_len(int n) {  // get_feat_extract_output_lengths, processor.rs:187-195
  const int r = n % 100;
  if (r > 0) {
    const int f = (r - 1) / 2 + 1;
    return ((f - 1) / 2 + 1 - 1) / 2 + 1 + (n / 100) * 13;
  }
  return (n / 100) * 13;
}
int64_t audio_tokens_of_frames(int64_t F) {
  const int win = 100;
  int64_t n_tok = 0;
  for (int64_t i = 0; i * win < F; ++i) n_tok += get_out_len((int)std::min<int64_t>(win, F - i * win));
  return n_tok;
}

// One clip of a tower pass (host view)
struct AudClip {
  const AudRequest* req;
  bool samples;       // raw samples (log-mel on the device) rather than features
  int64_t L, F;       // samples (0 for features), frames
  int C, n_tok;       // 100-frame windows, audio tokens
};

// every check of a request, before any device work: the clip's frames / tokens and its placeholder count
static int audio_check_request(aha_model* m, const AudRequest& r, AudClip* out) {
  const aha_model_desc& c = m->desc;
  const std::string who = r.seq >= 0 ? "sequence " + std::to_string(r.seq) + ": " : "";
  const aha_mm_input* mm = r.mm;
  AudClip k{&r, false, 0, 0, 0, 0};
  if (mm->audio_samples && mm->n_samples > 0) {   // samples win over features (as forward_initial has always read them)
    if (mm->n_samples < 401) {
      set_error(who + "audio too short for the reflect padding (need > 400 samples)");
      return AHA_ERR_INVALID;
    }
    k.samples = true;
    k.L = mm->n_samples;
    k.F = mm->n_samples / 160;  // (L + 400 - 400) / 160 + 1 frames, last one dropped
  } else if (mm->audio_features && mm->n_frames > 0) {
    k.F = mm->n_frames;
  } else {
    set_error(who + "forward_initial: audio input without features or samples");
    return AHA_ERR_INVALID;
  }
  if (k.F > ((int64_t)1 << 26)) {
    set_error(who + "audio input too long");
    return AHA_ERR_INVALID;
  }
  k.C = (int)((k.F + 2 * m->audio->nwin - 1) / (2 * m->audio->nwin));
  k.n_tok = (int)audio_tokens_of_frames(k.F);
  if (r.ids) {
    int64_t n_pad = 0;
    for (size_t i = 0; i < r.n; ++i) n_pad += r.ids[i] == (uint32_t)c.audio_token_id;
    if (n_pad != k.n_tok) {  // qwen3_asr/model.rs:349-355
      set_error(who + "n_audio_tokens num: " + std::to_string(n_pad) + " not equal to audio_feature len: " + std::to_string(k.n_tok));
      return AHA_ERR_SHAPE;
    }
  }
  *out = k;
  return AHA_OK;
}

int audio_check_requests(aha_model* m, const AudRequest* reqs, size_t n_reqs) {
  if (!m->audio) {
    set_error(std::string(n_reqs && reqs[0].seq >= 0 ? "sequence " + std::to_string(reqs[0].seq) + ": " : "") +
              "audio input given but this model has no audio tower");
    return AHA_ERR_UNSUPPORTED;
  }
  AudClip k;
  for (size_t i = 0; i < n_reqs; ++i) {
    const int rc = audio_check_request(m, reqs[i], &k);
    if (rc) return rc;
  }
  return AHA_OK;
}

// One tower sub-pass over clips k[0 .. n).  Layout (round 7):
//   features  (128, Ftot) f32, clip j in columns fo_j .. fo_j + F_j - 1: the sample clips' log-mel in ONE launch pair, the feature clips
//             copied into their columns;
//   conv      every clip's C_j windows in clip order (sum C_j chunks): conv1 .. conv3, the token gather, conv_out and the 13-periodic
//             position add run once, row order unchanged;
//   encoder   clip j keeps the first n_tok_j of its C_j * 13 rows (narrow(0, 0, feature_len_after_cnn) per clip), packed by a row gather;
//             row-wise ops once over the packed rows, K / V to pages with every clip starting on a page of its own, and the attention
//             block-diagonal: ONE non-causal seg_tab launch per layer ({row0, len, page0} per clip, 64-row items longest clip first);
//   projector over the packed rows, then clip j's rows scattered to its request's <|audio_pad|> rows.
// With one clip every step computes the bits of the one-clip code before it: the same features, the same chunks, the same GEMM shapes (so
// the same plans), no gather (the rows are already packed), identity KV slots, and a one-segment seg_tab launch = the plain launch.
static int audio_tower_pass(aha_model* m, const AudClip* k, int n, void* x_text) {
  AudioModel* a = m->audio;
  const aha_model_desc& c = m->desc;
  hipStream_t st = m->stream;
  const int win = 2 * a->nwin;  // 100 frames per chunk
  // ---- host tables --------------------------------------------------------------------------------------------------
  std::vector<int64_t> fo(n), clip_tab;
  std::vector<int32_t> chunk_tab, rows, slot, seg, src;
  int64_t Ftot = 0, Ltot = 0, groups = 0;
  int Ctot = 0, Ntok = 0, pages = 0, n_mel = 0;
  for (int j = 0; j < n; ++j) {
    fo[j] = Ftot;
    if (k[j].samples) {
      clip_tab.insert(clip_tab.end(), {Ltot, k[j].L, Ftot, k[j].F, groups});
      Ltot += k[j].L;
      groups += (k[j].F + 3) / 4;
      ++n_mel;
    }
    for (int i = 0; i < k[j].C; ++i) chunk_tab.insert(chunk_tab.end(), {(int32_t)Ftot, (int32_t)k[j].F, i});
    seg.insert(seg.end(), {Ntok, k[j].n_tok, pages});
    for (int i = 0; i < k[j].n_tok; ++i) {
      src.push_back(Ctot * 13 + i);
      slot.push_back(pages * KV_PAGE_TOKENS + i);
    }
    const AudRequest& r = *k[j].req;
    if (r.ids)
      for (size_t i = 0; i < r.n; ++i)
        if (r.ids[i] == (uint32_t)c.audio_token_id) rows.push_back((int32_t)(r.row0 + (int64_t)i));
    Ftot += k[j].F;
    Ctot += k[j].C;
    Ntok += k[j].n_tok;
    pages += (k[j].n_tok + KV_PAGE_TOKENS - 1) / KV_PAGE_TOKENS;
  }
  // attention items: (clip, 64-row q block), non-causal: longest clip first
  const std::vector<int32_t> items = seg_items_of(seg, false);
  seg.insert(seg.end(), items.begin(), items.end());
  const bool packed = n > 1;   // one clip: its rows are already packed, its KV slots the identity
  int rc;
  if ((rc = audio_ensure_scratch(m, (size_t)Ftot, (size_t)Ltot, (size_t)Ctot, (size_t)pages, (size_t)n))) return rc;
  // ---- uploads ------------------------------------------------------------------------------------------------------
  {
    int64_t so = 0;
    for (int j = 0; j < n; ++j) {
      const aha_mm_input* mm = k[j].req->mm;
      if (k[j].samples) {
        AHA_HIP_CHECK(hipMemcpyAsync(a->d_samples + so, mm->audio_samples, (size_t)k[j].L * 4, hipMemcpyDefault, st));
        so += k[j].L;
      } else {   // (128, F_j) -> columns fo_j .. of the (128, Ftot) buffer
        AHA_HIP_CHECK(hipMemcpy2DAsync(a->d_feat + fo[j], (size_t)Ftot * 4, mm->audio_features, (size_t)k[j].F * 4, (size_t)k[j].F * 4,
                                       (size_t)a->mels, hipMemcpyDefault, st));
      }
    }
  }
  if (n_mel) AHA_HIP_CHECK(hipMemcpyAsync(a->d_clips, clip_tab.data(), clip_tab.size() * 8, hipMemcpyHostToDevice, st));
  AHA_HIP_CHECK(hipMemcpyAsync(a->d_chunks, chunk_tab.data(), chunk_tab.size() * 4, hipMemcpyHostToDevice, st));
  AHA_HIP_CHECK(hipMemcpyAsync(a->d_seg, seg.data(), seg.size() * 4, hipMemcpyHostToDevice, st));
  if (packed) {
    AHA_HIP_CHECK(hipMemcpyAsync(a->d_slot, slot.data(), slot.size() * 4, hipMemcpyHostToDevice, st));
    AHA_HIP_CHECK(hipMemcpyAsync(a->d_src, src.data(), src.size() * 4, hipMemcpyHostToDevice, st));
  }
  if (!rows.empty()) AHA_HIP_CHECK(hipMemcpyAsync(a->d_rows, rows.data(), rows.size() * 4, hipMemcpyHostToDevice, st));
  AHA_HIP_CHECK(hipStreamSynchronize(st));   // host vectors are pageable
  if (n_mel) {
    ProfScope ps(m, "logmel", (double)Ltot * 4 + (double)128 * Ftot * 4, 2.0 * Ftot * 201 * 400 * 2);
    launch_logmel(a->d_samples, a->d_clips, n_mel, groups, Ftot, a->d_window, a->d_twid, a->d_melfb, a->d_feat, a->d_fmax, st);
  }

  // conv stack: (C,1,128,100) -> (C,H,64,50) -> (C,H,32,25) -> (C,H,16,13), each conv + bias + tanh-GELU (model.rs:196-204)
  const int H = a->H, C = Ctot;
  {
    ProfScope ps(m, "elem", (double)C * 64 * 50 * 32, 0);
    launch_audio_im2col1(a->d_feat, a->d_chunks, a->col, Ftot, C, a->mels, win, st);
  }
  agemm(m, a->col, a->c1w, a->act_a, C * 64 * 50, H, 16, a->c1b, nullptr, ACT_GELU_TANH);
  {
    ProfScope ps(m, "elem", (double)C * 32 * 25 * 9 * H * 4, 0);
    launch_im2col_nhwc(a->act_a, a->col, C, 64, 50, H, st);
  }
  agemm(m, a->col, a->c2w, a->act_b, C * 32 * 25, H, 9 * H, a->c2b, nullptr, ACT_GELU_TANH);
  {
    ProfScope ps(m, "elem", (double)C * 16 * 13 * 9 * H * 4, 0);
    launch_im2col_nhwc(a->act_b, a->col, C, 32, 25, H, st);
  }
  agemm(m, a->col, a->c3w, a->act_a, C * 16 * 13, H, 9 * H, a->c3b, nullptr, ACT_GELU_TANH);
  {
    ProfScope ps(m, "elem", (double)C * 13 * H * a->fq * 4, 0);
    launch_audio_tokens_gather(a->act_a, a->tok, C, a->fq, 13, H, st);
  }
  const int D = a->D;
  void* xc = packed ? a->h : a->x;   // the conv_out rows: packed into a->x below when there is more than one clip
  agemm(m, a->tok, a->conv_out, xc, C * 13, D, H * a->fq, nullptr, nullptr, ACT_NONE);
  {
    ProfScope ps(m, "elem", (double)C * 13 * D * 4, 0);
    launch_sinus_pe_add(xc, (int64_t)C * 13, D, 13, st);
  }
  // clip j's first n_tok_j rows are its audio tokens (narrow(0, 0, feature_len_after_cnn), model.rs:213-215)
  const int n_tok = Ntok;
  if (packed) {
    ProfScope ps(m, "elem", (double)n_tok * D * 4, 0);
    launch_embed_gather(a->h, a->d_src, a->x, n_tok, D, st);
  }
  KvLayer kv{};
  kv.page_ptrs = a->d_page_ptrs;
  kv.layer_off = 0;
  kv.kvh = a->nh;
  kv.d = a->hd;
  // round 6: the LayerNorm behind fc2 + residual -- norm1 of the next layer, ln_post after the last -- rides on the fc2 call (its plan at the
  // real widths is K slices + a reduce pass: one launch less per layer); AHA_AUD_FUSE_LN=0: every LayerNorm its own launch (same bits)
  static const bool fuse_ln = [] { const char* e = getenv("AHA_AUD_FUSE_LN"); return e ? atoi(e) != 0 : true; }();
  double attn_flops = 0;
  for (int j = 0; j < n; ++j) attn_flops += 4.0 * k[j].n_tok * k[j].n_tok * D;
  bool h_ready = false;   // a->h already holds the LayerNorm of a->x
  for (int li = 0; li < a->layers; ++li) {
    const AudLayerW& L = a->L[li];
    if (!h_ready) {
      ProfScope ps(m, "elem", (double)n_tok * D * 4, 0);
      launch_layernorm_rows(a->x, L.ln1w, L.ln1b, a->h, n_tok, D, 1e-5f, st);
    }
    agemm(m, a->h, L.qkv_w, a->qkv, n_tok, 3 * D, D, L.qkv_b, nullptr, ACT_NONE);
    {
      ProfScope ps(m, "elem", (double)n_tok * D * 8, 0);
      launch_kv_pack_generic(a->qkv, 3 * D, D, 2 * D, kv, n_tok, a->nh, a->hd, st, packed ? a->d_slot : nullptr);
    }
    {  // global (unmasked, unwindowed) attention over each clip's own tokens (model.rs:218-220): block-diagonal, one launch
      AttnPrefillArgs q{};
      q.q = a->qkv; q.q_ld = 3 * D; q.kv = kv; q.o = a->attn; q.S = n_tok; q.nh = a->nh; q.kvh = a->nh; q.d = a->hd;
      q.kv_offset = 0; q.kv_total = n_tok; q.causal = 0; q.scale = a->scale;
      q.seg_tab = a->d_seg; q.seg_items = a->d_seg + 3 * (size_t)n; q.n_items = (int)items.size() / 2;
      ProfScope ps(m, "attn_audio", (double)n_tok * D * 8, attn_flops);
      launch_attn_prefill(q, st);
    }
    agemm(m, a->attn, L.out_w, a->x, n_tok, D, D, L.out_b, a->x, ACT_NONE);
    {
      ProfScope ps(m, "elem", (double)n_tok * D * 4, 0);
      launch_layernorm_rows(a->x, L.ln2w, L.ln2b, a->h, n_tok, D, 1e-5f, st);
    }
    agemm(m, a->h, L.fc1_w, a->mlp, n_tok, a->ffn, D, L.fc1_b, nullptr, ACT_GELU_ERF);
    if (fuse_ln) {
      const bool last = li + 1 == a->layers;
      agemm(m, a->mlp, L.fc2_w, a->x, n_tok, D, a->ffn, L.fc2_b, a->x, ACT_NONE, last ? a->lnp_w : a->L[li + 1].ln1w,
            last ? a->lnp_b : a->L[li + 1].ln1b, a->h);
      h_ready = true;
    } else {
      agemm(m, a->mlp, L.fc2_w, a->x, n_tok, D, a->ffn, L.fc2_b, a->x, ACT_NONE);
    }
  }
  if (!h_ready) {
    ProfScope ps(m, "elem", (double)n_tok * D * 4, 0);
    launch_layernorm_rows(a->x, a->lnp_w, a->lnp_b, a->h, n_tok, D, 1e-5f, st);
  }
  agemm(m, a->h, a->p1w, a->mlp, n_tok, D, D, a->p1b, nullptr, ACT_GELU_ERF);
  agemm(m, a->mlp, a->p2w, a->embeds, n_tok, a->out, D, a->p2b, nullptr, ACT_NONE);
  a->n_tok = n_tok;
  if (!rows.empty()) {
    ProfScope ps(m, "elem", (double)n_tok * a->out * 4, 0);
    launch_scatter_rows(x_text, a->embeds, a->d_rows, n_tok, a->out, 0, st);
  }
  AHA_HIP_CHECK(hipGetLastError());
  return AHA_OK;
}

int audio_forward_requests(aha_model* m, const AudRequest* reqs, size_t n_reqs, void* x_text) {
  int rc;
  if ((rc = audio_check_requests(m, reqs, n_reqs))) return rc;
  std::vector<AudClip> clips(n_reqs);
  for (size_t i = 0; i < n_reqs; ++i) audio_check_request(m, reqs[i], &clips[i]);
  // sub-passes of at most AUD_PASS_FRAMES frames (a clip is never split; one longer clip is a sub-pass of its own)
  size_t i = 0;
  while (i < n_reqs) {
    size_t e = i + 1;
    int64_t frames = clips[i].F;
    while (e < n_reqs && frames + clips[e].F <= AUD_PASS_FRAMES) frames += clips[e++].F;
    if ((rc = audio_tower_pass(m, clips.data() + i, (int)(e - i), x_text))) return rc;
    i = e;
  }
  return AHA_OK;
}

int audio_debug_embeds(aha_model* m, float* out, size_t n) {
  AudioModel* a = m->audio;
  if (!a || n != (size_t)a->n_tok * a->out) {
    set_error("debug_audio_embeds: no audio embeddings of that shape");
    return AHA_ERR_INVALID;
  }
  std::vector<uint16_t> tmp(n);
  AHA_HIP_CHECK(hipStreamSynchronize(m->stream));
  AHA_HIP_CHECK(hipMemcpy(tmp.data(), a->embeds, n * 2, hipMemcpyDeviceToHost));
  for (size_t i = 0; i < n; ++i) out[i] = bf2f_h(tmp[i]);
  return AHA_OK;
}

// op-level frontend (aha_hip_logmel, aha_hip_logmel_batch): tables built on the fly; clip j's n_samples[j] samples follow clip j - 1's in
// d_samples, its n_samples[j] / 160 frames follow clip j - 1's in the (128, sum F_j) output
int logmel_standalone(const float* d_samples, const int64_t* n_samples, size_t n_clips, float* d_out, hipStream_t st) {
  std::vector<int64_t> tab;
  int64_t so = 0, Ftot = 0, groups = 0;
  for (size_t j = 0; j < n_clips; ++j) {
    const int64_t F = n_samples[j] / 160;
    tab.insert(tab.end(), {so, n_samples[j], Ftot, F, groups});
    so += n_samples[j], Ftot += F, groups += (F + 3) / 4;
  }
  aha_model fake;
  aha_ctx ctx;
  fake.ctx = &ctx;
  fake.stream = st;
  int rc = AHA_OK;
  std::vector<float> win(400), tw(800), fb((size_t)201 * 128);
  for (int j = 0; j < 400; ++j) {
    const double i = (double)(1 - 400 + 2 * j);
    win[j] = (float)(0.5 + 0.5 * cos(M_PI * i / 399.0));
    tw[2 * j] = (float)cos(2.0 * M_PI * j / 400.0);
    tw[2 * j + 1] = (float)(-sin(2.0 * M_PI * j / 400.0));
  }
  const std::vector<float> melpts = linspace_f(hz2mel(0.0f), hz2mel(8000.0f), 130);
  std::vector<float> filt(130);
  for (int i = 0; i < 130; ++i) filt[i] = mel2hz(melpts[i]);
  const std::vector<float> fft = linspace_f(0.0f, 8000.0f, 201);
  for (int k = 0; k < 201; ++k)
    for (int j = 0; j < 128; ++j) {
      const float down = -1.0f * (filt[j] - fft[k]) / (filt[j + 1] - filt[j]);
      const float up = (filt[j + 2] - fft[k]) / (filt[j + 2] - filt[j + 1]);
      fb[(size_t)k * 128 + j] = std::max(std::min(down, up), 0.0f) * (2.0f / (filt[j + 2] - filt[j]));
    }
  void *pw = nullptr, *pt = nullptr, *pf = nullptr, *pm = nullptr, *pc = nullptr;
  if ((rc = dev_alloc(&fake, win.size() * 4, &pw)) || (rc = dev_alloc(&fake, tw.size() * 4, &pt)) ||
      (rc = dev_alloc(&fake, fb.size() * 4, &pf)) || (rc = dev_alloc(&fake, (size_t)Ftot * 4 + 16, &pm)) ||
      (rc = dev_alloc(&fake, tab.size() * 8, &pc))) {
    for (void* p : fake.owned) hipFree(p);
    return rc;
  }
  hipMemcpy(pw, win.data(), win.size() * 4, hipMemcpyHostToDevice);
  hipMemcpy(pt, tw.data(), tw.size() * 4, hipMemcpyHostToDevice);
  hipMemcpy(pf, fb.data(), fb.size() * 4, hipMemcpyHostToDevice);
  hipMemcpy(pc, tab.data(), tab.size() * 8, hipMemcpyHostToDevice);
  launch_logmel(d_samples, (const int64_t*)pc, (int)n_clips, groups, Ftot, (float*)pw, (float*)pt, (float*)pf, d_out, (float*)pm, st);
  hipError_t e = hipGetLastError();
  hipStreamSynchronize(st);
  for (void* p : fake.owned) hipFree(p);
  if (e != hipSuccess) {
    set_error(std::string("logmel launch failed: ") + hipGetErrorString(e));
    return AHA_ERR_HIP;
  }
  return AHA_OK;
}

}  // namespace aha
