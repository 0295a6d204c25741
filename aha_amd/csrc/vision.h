// Qwen3-VL specific host pieces: M-RoPE position bookkeeping (M2), the vision tower (V1-V7) and the visual-token
// scatter / DeepStack adds (M3).  SURVEY.md section 8a.
#pragma once
#include "model.h"

namespace aha {

int vision_create(aha_model* m, const aha_tensor_view* w, size_t nw);
void vision_destroy(aha_model* m);
// get_rope_index (/root/reference/src/models/qwen3vl/model.rs:901-1133): fills pos (3, n) rows T,H,W and sets
// m->rope_delta.  mm == nullptr => text only: rows = arange(n) + offset, delta 0.
int rope_index_core(const aha_model_desc& c, const uint32_t* ids, size_t S, const uint32_t* grid_thw, int n_images,
                    const uint32_t* video_grid_thw, int n_videos, int32_t* pos, int64_t* rope_delta);
int vl_rope_index(aha_model* m, const uint32_t* ids, size_t n, size_t offset, const aha_mm_input* mm, int32_t* pos);
int vision_forward_and_scatter(aha_model* m, const uint32_t* ids, size_t n, const aha_mm_input* mm, void* x);
// One request of a tower pass: its images / videos, its ids, the row of x its ids start at; seq >= 0 names it in error messages.
struct VisRequest {
  const aha_mm_input* mm;
  const uint32_t* ids;
  size_t n;
  int64_t row0;
  int seq;
};
// Every check of a request's images / videos, no device work: pixel values and grids given, the pixel dtype, h and w multiples of the merge
// size, the patch rows the grids describe, and (ids given) its placeholder counts.  n_img / n_vid: its image / video patch rows.
int vision_check_request(const aha_model_desc& c, const VisRequest& r, int64_t* n_img, int64_t* n_vid);
// The tower over every request's images and videos in ONE pass (no image_embeds), the merged rows scattered to each request's
// placeholder rows of x; vision_deepstack_add then adds to those rows.  vision_forward_and_scatter = one request at row 0.
int vision_forward_requests(aha_model* m, const VisRequest* reqs, size_t n_reqs, void* x);
// The host tables of a tower pass (vision_tower.hip vision_host_tables): idx / wt (4, N) corner indices and f32 weights of the position
// embedding, rowcol (N, 2), page_of / slot_of (N), page_first / page_cnt (pages), and one attention segment per (grid, frame).
struct VisSeg { int64_t start, len, page0; bool small; };
struct VisHostTables {
  int64_t N = 0, pages = 0;
  std::vector<int32_t> idx, rowcol, page_of, slot_of, page_first, page_cnt;
  std::vector<float> wt;
  std::vector<VisSeg> segs;
};
void vision_host_tables(const uint32_t* const* grids, size_t n_grids, int G, int ms, VisHostTables* out);
int vision_deepstack_add(aha_model* m, int layer, void* x);
bool vision_has_deepstack(aha_model* m, int layer);   // vision_deepstack_add(layer) would change rows
int vision_debug_embeds(aha_model* m, int which, float* out, size_t n);
int vision_encode(aha_model* m, const aha_mm_input* mm, void* out_dev, int64_t* n_tokens);

}  // namespace aha
