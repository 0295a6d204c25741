"""Output digests of the packed prefill launches WITHOUT a per-segment cache prefix (AttnPrefillArgs::seg_kv0 == nullptr): embed_batch,
generate_batch (greedy tokens and logits) and a Qwen3-VL image request through generate_batch_mm (the ViT's block-diagonal segment
launch).  tests/golden/engine_parent_digests.json holds them as computed by the library before the engine's attention change
(`python tests/engine_digests.py OUT.json` on an MI355X); tests/test_engine_gpu.py recomputes them.  The audio tower's launch has its own
recorded digests (tests/golden/asr_single_clip_digests.json)."""
import hashlib
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def sha(*arrays) -> str:
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def compute() -> dict:
    from aha_amd.configs import tiny_qwen3, tiny_qwen3vl
    from aha_amd.model import HipInferenceModel, MultiModalData
    from aha_amd.vision_host import image_prompt_ids
    from aha_amd.weights import qwen3_text_weights, qwen3vl_weights
    from oracle import qwen3vl as ov
    from oracle.numerics import Numerics

    out = {}
    cfg = tiny_qwen3(layers=2, hidden=256, heads=4, kv_heads=2, inter=512, vocab=1024)
    m = HipInferenceModel(cfg, qwen3_text_weights(cfg, seed=11))
    g = np.random.default_rng(12)
    prompts = [[int(x) for x in g.integers(0, cfg.vocab_size, size=n)] for n in (70, 130, 5, 64, 200)]
    emb = m.embed_batch(prompts)
    out["embed_batch"] = sha(emb)
    toks, lg = m.generate_batch(prompts, 6, want_logits=True)
    out["generate_batch"] = sha(np.asarray([t for row in toks for t in row], np.uint32), lg)
    m.close()

    vcfg = tiny_qwen3vl()
    vm = HipInferenceModel(vcfg, qwen3vl_weights(vcfg, seed=0))
    nm = Numerics("bf16", matmul_f64=True)
    g = np.random.default_rng(13)
    pv, grid = ov.process_images(nm, [g.integers(0, 256, size=(64, 96, 3), dtype=np.uint8)])
    ids = image_prompt_ids(vcfg, grid, [5, 6, 7], [int(x) for x in g.integers(0, 1900, size=9)])
    data = MultiModalData(pv.to(torch.bfloat16), grid)
    vt, vl = vm.generate_batch_mm([ids, [int(x) for x in g.integers(0, 1900, size=40)]], [data, None], 5, want_step_logits=True)
    out["generate_batch_mm_image"] = sha(np.asarray([t for row in vt for t in row], np.uint32), vl)
    vm.close()
    return out


if __name__ == "__main__":
    res = compute()
    print(json.dumps(res, indent=1))
    if len(sys.argv) > 1:
        os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
        with open(sys.argv[1], "w") as f:
            json.dump(res, f, indent=1, sort_keys=True)
