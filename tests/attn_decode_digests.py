"""Output digests of the batch-1 decode step at the smallest shapes that reach each path of the fused decode attention
(aha_amd/csrc/attn_decode_body.h): sha256 over the greedy tokens and the last step's f32 logits of forward_initial + decode_greedy(.., 8)
on two-layer tiny models.  tests/golden/attn_decode_parent_digests.json holds them as computed by the library before the kernel formed
its page addresses by arithmetic and its LDS staging image was re-laid (`python tests/attn_decode_digests.py OUT.json` on an MI355X, on
that commit); tests/test_attn_decode_chain_gpu.py recomputes them: the change moves addresses and requests, so every bit must stay.

Head shapes (heads / kv heads):  4 / 2: g = 2, 64 merge items;  8 / 2: g = 4 (the 8B ratio): two merging waves, the min(c, g - 1)
clamp of the q rows, the k head as wave 0's second prologue item.
Prompts:  40: one page, a single split, nothing published;  60: the eight steps cross L_old = 64 (the append moves to slot 0 of a new
page, a full page's tail mask);  300: five pages, two splits;  700: eleven pages, three splits (the final merge sees more than two
partials, the rest of its sixteen registers re-reading the last one);  1100: five splits."""
import hashlib
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

HEAD_SHAPES = ((4, 2), (8, 2))
PROMPTS = (40, 60, 300, 700, 1100)
STEPS = 8


def sha(*arrays) -> str:
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def config(heads, kv_heads):
    from aha_amd.configs import tiny_qwen3
    return tiny_qwen3(layers=2, hidden=512, heads=heads, kv_heads=kv_heads, inter=1024, vocab=2048)


def make_model(heads, kv_heads, kv_reserve_tokens=0):
    from aha_amd.model import HipInferenceModel
    from aha_amd.weights import qwen3_text_weights
    cfg = config(heads, kv_heads)
    return HipInferenceModel(cfg, qwen3_text_weights(cfg, seed=3), kv_reserve_tokens=kv_reserve_tokens)


def prompt_ids(n_prompt):
    g = torch.Generator().manual_seed(1000 + n_prompt)
    return torch.randint(0, 1900, (n_prompt,), generator=g).tolist()


def run_case(m, n_prompt, steps=STEPS):
    """(tokens: the prefill's argmax and the steps', last step's logits) of a fresh request on `m` (whose cache is cleared first)."""
    m.clear_cache()
    _, tok = m.forward_initial(prompt_ids(n_prompt), 0, want_logits=False)
    toks = m.decode_greedy(tok, n_prompt, steps)
    return np.asarray([int(tok)] + toks, np.uint32), m.last_logits()


def key(heads, kv_heads, n_prompt):
    return f"heads{heads}_kv{kv_heads}_prompt{n_prompt}"


def compute(scramble=False, prompts=PROMPTS) -> dict:
    out = {}
    for heads, kv_heads in HEAD_SHAPES:
        m = make_model(heads, kv_heads)
        if scramble:
            m.debug_scramble_pages(True)   # before the first slab exists: its pages are handed out in a shuffled order
        for n in prompts:
            toks, last = run_case(m, n)
            out[key(heads, kv_heads, n)] = sha(toks, last)
        m.close()
    return out


if __name__ == "__main__":
    res = compute()
    print(json.dumps(res, indent=1))
    if len(sys.argv) > 1:
        os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
        with open(sys.argv[1], "w") as f:
            json.dump(res, f, indent=1, sort_keys=True)
