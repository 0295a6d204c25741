"""Output digests of the batch-1 decode kernels: the weight-streaming matvec through aha_amd.ops at the smallest shapes that reach each of
its code paths, and the decode step (matvecs, fused decode attention, lm_head with its argmax partials, the step's state kernels) through
forward_initial + decode_greedy on tiny models.  tests/golden/decode_parent_digests.json holds them as computed by the library before the
decode kernels took their leading arguments as plain (preloaded) parameters (`python tests/decode_digests.py OUT.json` on an MI355X);
tests/test_decode_preload_gpu.py recomputes them: the change moves kernel arguments, so every bit must stay."""
import hashlib
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

# lm_head rows planted for the argmax tie (logits epilogue, N = 2051, K = 512: 513 four-row tiles, the last one ragged): rows TIE_POS
# hold +v, rows TIE_NEG hold -v, |v| = 0.5 per element against N(0, 0.02) everywhere else -- whichever sign the final hidden state gives
# v . h, one pair is the maximum twice over, in different tiles and blocks, and the lower index must win.
TIE_POS, TIE_NEG = (7, 2049), (300, 2050)
LOGITS_VOCAB, LOGITS_HIDDEN = 2051, 512


def sha(*arrays) -> str:
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def bf16_bits(t: torch.Tensor) -> np.ndarray:
    return t.detach().contiguous().view(torch.int16).cpu().numpy()


def rand_bf16(g, *shape, scale=1.0):
    return (torch.randn(*shape, generator=g) * scale).to(torch.bfloat16)


def gemv_cases() -> dict:
    """(N, K) = (20, 520): not FAST, ragged last tile, zero-filled chunk tail; (1028, 1024): FAST with U = 2, clamped last tile."""
    from aha_amd import ops
    out = {}
    g = torch.Generator().manual_seed(31)
    for N, K in ((20, 520), (1028, 1024)):
        W = rand_bf16(g, N, K, scale=0.05).cuda()
        x = rand_bf16(g, K).cuda()
        nw = (1.0 + 0.1 * torch.randn(K, generator=g)).to(torch.bfloat16).cuda()
        res = rand_bf16(g, N).cuda()
        for with_norm in (False, True):
            for with_res in (False, True):
                y = ops.gemv(W, x, norm_w=nw if with_norm else None, eps=1e-6, residual=res if with_res else None)
                torch.cuda.synchronize()
                out[f"gemv_{N}x{K}_norm{int(with_norm)}_res{int(with_res)}"] = sha(bf16_bits(y))
    N, K = 72, 512
    Wg, Wu = rand_bf16(g, N, K, scale=0.05).cuda(), rand_bf16(g, N, K, scale=0.05).cuda()
    x = rand_bf16(g, K).cuda()
    nw = (1.0 + 0.1 * torch.randn(K, generator=g)).to(torch.bfloat16).cuda()
    for with_norm in (False, True):
        y = ops.gemv_gate_up(Wg, Wu, x, norm_w=nw if with_norm else None, eps=1e-6)
        torch.cuda.synchronize()
        out[f"gemv_gate_up_{N}x{K}_norm{int(with_norm)}"] = sha(bf16_bits(y))
    return out


def logits_model():
    """One-layer model whose lm_head (2051 x 512, untied) holds the planted rows."""
    from aha_amd.configs import tiny_qwen3
    from aha_amd.weights import qwen3_text_weights
    cfg = tiny_qwen3(layers=1, hidden=LOGITS_HIDDEN, heads=4, kv_heads=2, inter=1024, vocab=LOGITS_VOCAB, tie=False)
    w = qwen3_text_weights(cfg, seed=5)
    key = [k for k in w if "lm_head" in k]
    assert len(key) == 1, key
    head = w[key[0]].clone()
    assert tuple(head.shape) == (LOGITS_VOCAB, LOGITS_HIDDEN)
    g = torch.Generator().manual_seed(6)
    v = (torch.randint(0, 2, (LOGITS_HIDDEN,), generator=g).float() - 0.5).to(head.dtype)   # +-0.5: exact in bf16
    for r in TIE_POS:
        head[r] = v
    for r in TIE_NEG:
        head[r] = -v
    w[key[0]] = head
    return cfg, w


def logits_case():
    """Prefill of 5 tokens, then 3 greedy steps: returns (prefill logits, prefill argmax, step tokens, last logits)."""
    from aha_amd.model import HipInferenceModel
    cfg, w = logits_model()
    m = HipInferenceModel(cfg, w)
    lg, am = m.forward_initial([3, 1, 4, 1, 5], 0)
    lg = np.array(lg, copy=True)
    toks = m.decode_greedy(am, 5, 3)
    last = m.last_logits()
    m.close()
    return lg, int(am), toks, last


def decode_case(cfg, w, n_prompt, steps=8, seed=0):
    from aha_amd.model import HipInferenceModel
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(0, 1900, (n_prompt,), generator=g).tolist()
    m = HipInferenceModel(cfg, w)
    _, tok = m.forward_initial(ids, 0, want_logits=False)
    toks = m.decode_greedy(tok, n_prompt, steps)
    last = m.last_logits()
    m.close()
    return [int(tok)] + toks, last


def compute() -> dict:
    from aha_amd.configs import tiny_qwen3, tiny_qwen3vl
    from aha_amd.weights import qwen3_text_weights, qwen3vl_weights
    out = gemv_cases()
    lg, am, toks, last = logits_case()
    out["logits_2051x512"] = sha(lg, np.asarray([am] + toks, np.uint32), last)
    cfg = tiny_qwen3(layers=2, hidden=512, heads=4, kv_heads=2, inter=1024, vocab=2048)
    w = qwen3_text_weights(cfg, seed=3)
    for n in (40, 300):   # one KV page: a single split; five pages: two splits, the published-partials path
        toks, last = decode_case(cfg, w, n, seed=n)
        out[f"decode_prompt{n}"] = sha(np.asarray(toks, np.uint32), last)
    vcfg = tiny_qwen3vl()
    toks, last = decode_case(vcfg, qwen3vl_weights(vcfg, seed=0), 40, seed=41)   # text-only prompt: the three-axis rope table
    out["decode_qwen3vl_prompt40"] = sha(np.asarray(toks, np.uint32), last)
    return out


if __name__ == "__main__":
    res = compute()
    print(json.dumps(res, indent=1))
    if len(sys.argv) > 1:
        os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
        with open(sys.argv[1], "w") as f:
            json.dump(res, f, indent=1, sort_keys=True)
