"""Worker of tests/test_generate_batch_mm_gpu.py::test_vit_single_launch_is_bit_identical: one Qwen3-VL request with five small images
of mixed sizes, one image large enough for the 64-row attention form and a video, through forward_initial and through
generate_batch_mm with two more requests.  Prints a digest of the image embeddings, the DeepStack features and the prefill logits,
and the attention launches of the tower.  Run with AHA_VIT_SEG_ATTN=0 (one launch per segment) and =1 (the small segments in one
launch): the digests must be equal."""
import hashlib
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

SMALL = [(2, 2), (4, 6), (6, 4), (2, 8), (8, 8)]   # (h, w) patch grids
LARGE = (128, 256)                                 # 32768 patches x 2 heads: the 64-row form fills the chip
VIDEO = (2, 4, 4)                                  # (t, h, w): two frame segments


def request(cfg, g, small, large, video):
    from aha_amd.model import MultiModalData
    pd = 3 * 2 * 16 * 16
    grids = [(1, h, w) for (h, w) in small] + ([(1,) + large] if large else [])
    ids = [int(x) for x in g.integers(0, 1900, size=5)]
    for (t, h, w) in grids:
        ids += [cfg.vision_start_token_id] + [cfg.image_token_id] * (t * h * w // 4) + [cfg.vision_end_token_id]
        ids += [int(x) for x in g.integers(0, 1900, size=2)]
    n_img = sum(t * h * w for (t, h, w) in grids)
    pv = torch.from_numpy(g.standard_normal((n_img, pd)).astype(np.float32)).to(torch.bfloat16)
    data = MultiModalData(pv, np.asarray(grids, dtype=np.uint32))
    if video:
        t, h, w = video
        for _ in range(t):
            ids += [int(x) for x in g.integers(0, 1900, size=2)]
            ids += [cfg.vision_start_token_id] + [cfg.video_token_id] * (h * w // 4) + [cfg.vision_end_token_id]
        data.pixel_values_video = torch.from_numpy(g.standard_normal((t * h * w, pd)).astype(np.float32)).to(torch.bfloat16)
        data.video_grid_thw = np.asarray([video], dtype=np.uint32)
    ids += [int(x) for x in g.integers(0, 1900, size=7)]
    return ids, data


def main():
    from aha_amd.configs import tiny_qwen3vl
    from aha_amd.model import HipInferenceModel
    from aha_amd.weights import qwen3vl_weights
    cfg = tiny_qwen3vl()
    m = HipInferenceModel(cfg, qwen3vl_weights(cfg, seed=0))
    g = np.random.default_rng(41)
    ids, data = request(cfg, g, SMALL, LARGE, VIDEO)
    h = hashlib.sha256()
    m.clear_cache()
    m.set_profiling(True)
    lg, _ = m.forward_initial(ids, 0, data)
    launches = m.get_profile("attn_vit")["launches"]
    m.set_profiling(False)
    n4 = (sum(h_ * w_ for (h_, w_) in SMALL) + LARGE[0] * LARGE[1] + VIDEO[0] * VIDEO[1] * VIDEO[2]) // 4
    for k in range(1 + len(cfg.vision.deepstack_visual_indexes)):
        h.update(m.debug_image_embeds(k, n4).tobytes())
    h.update(lg.tobytes())
    m.clear_cache()
    # the same request in a batch, next to two small-image requests in the same prefill pass: tokens and step logits
    ids2, data2 = request(cfg, g, [(4, 4), (2, 6)], None, None)
    ids3, data3 = request(cfg, g, [(6, 6)], None, (1, 2, 4))
    m.set_profiling(True)
    toks, step = m.generate_batch_mm([ids, ids2, ids3], [data, data2, data3], 4, want_step_logits=True)
    batch_launches = m.get_profile("attn_vit")["launches"]
    m.set_profiling(False)
    h.update(np.asarray(toks, dtype=np.uint32).tobytes())
    h.update(step.tobytes())
    m.close()
    print("VIT_SEG_DIGEST", h.hexdigest())
    print("VIT_SEG_LAUNCHES", json.dumps({"forward_initial": launches, "batch": batch_launches, "depth": cfg.vision.depth,
                                          "segments": len(SMALL) + 1 + VIDEO[0],
                                          "batch_segments": len(SMALL) + 1 + VIDEO[0] + 2 + 1 + 1}))


if __name__ == "__main__":
    main()
