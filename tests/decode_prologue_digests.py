"""Output digests of the batch-1 decode kernels at the shapes a clamped, unconditional request can break: the matvec
(aha_amd/csrc/gemv_body.h) through aha_amd.ops, and the fused decode attention (attn_decode_body.h) in its table form through
ops.debug_attn_decode_fused and in its linear form through a one-layer model.  tests/golden/decode_prologue_parent_digests.json holds
them as computed by the library before the prologue's inputs, the first weight tile and the first KV page were requested without
conditions (`python tests/decode_prologue_digests.py OUT.json` on an MI355X, on that commit); tests/test_decode_prologue_edges_gpu.py
recomputes them: the change moves requests, no arithmetic, so every bit must stay.

Matvec (N, K), each with and without norm weights, epilogues store / + residual / silu(gate) * up:
  (3, 512):      fewer rows than one tile of any plan: every row index of the first request is clamped;
  (4100, 4096):  the decode width, ragged last tile (4100 = 1025 * 4);
  (64, 520):     K tail inside a chunk: not the FAST form, the zero-filled tail of the general prologue;
  (16, 16896):   33 chunks: beyond the 8 * 2048 elements the straight-line prologue preloads, the FAST form's general prologue.
Attention, heads / kv heads 32 / 8 (g = 4: the k head is wave 0's second prologue item) and 16 / 8 (g = 2: no wave has a second
item, every wave requests the clamped one), cache length after the step:
  1:    no old token, no old page: every unit requests the append slot's page and computes nothing;
  2:    one old token: unit 0 alone owns a page;
  64:   a full old page minus one: the append fills the page's last slot;
  65:   the append opens a second page, which holds no old token and is no unit's;
  257:  four full old pages and the append's own; the split rule counts all five: two splits, eight units for four old pages -- every
        wave of the first block owns one page, no wave of the last block owns any (its partial is empty).
"""
import hashlib
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

GEMV_SHAPES = ((3, 512), (4100, 4096), (64, 520), (16, 16896))
HEAD_SHAPES = ((32, 8), (16, 8))
CACHE_LENS = (1, 2, 64, 65, 257)
LINEAR, TABLE = 1, 0


def sha(*arrays) -> str:
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def bits(t: torch.Tensor) -> np.ndarray:
    return t.detach().contiguous().view(torch.int16).cpu().numpy()


def rnd(shape, seed, std=1.0, mean=0.0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(shape, generator=g) * std + mean).to(torch.bfloat16).cuda()


def gemv_key(N, K, with_norm, epi):
    return f"gemv_{N}x{K}_norm{int(with_norm)}_{epi}"


def gemv_case(N, K) -> dict:
    """The six digests of one shape: {store, residual, silu_mul} x {no norm, norm}."""
    from aha_amd import ops
    W, W2 = rnd((N, K), 100 + N, 0.05), rnd((N, K), 200 + N, 0.05)
    x, nw, res = rnd((K,), 300 + K), rnd((K,), 400 + K, 0.1, 1.0), rnd((N,), 500 + N)
    out = {}
    for with_norm in (False, True):
        n = nw if with_norm else None
        out[gemv_key(N, K, with_norm, "store")] = sha(bits(ops.gemv(W, x, norm_w=n, eps=1e-6)))
        out[gemv_key(N, K, with_norm, "residual")] = sha(bits(ops.gemv(W, x, norm_w=n, eps=1e-6, residual=res)))
        out[gemv_key(N, K, with_norm, "silu_mul")] = sha(bits(ops.gemv_gate_up(W, W2, x, norm_w=n, eps=1e-6)))
    torch.cuda.synchronize()
    return out


def attn_key(form, heads, kv_heads, L):
    return f"attn_{'linear' if form == LINEAR else 'table'}_heads{heads}_kv{kv_heads}_len{L}"


def attn_table_case(heads, kv_heads, L) -> str:
    """The single-sequence kernel on shuffled pages of the caller (always the table form): digest of the output and of the pages after
    the append."""
    from aha_amd import ops
    page_elems = 2 * kv_heads * 64 * 128
    P = (L + 63) // 64 + 2
    pool = rnd((P, page_elems), 11 + L)
    perm = torch.randperm(P, generator=torch.Generator().manual_seed(12 + L))
    ptrs = (pool.data_ptr() + perm.to(torch.int64) * page_elems * 2).cuda()
    qkv = rnd(((heads + 2 * kv_heads) * 128,), 13 + L)
    qn, kn = rnd((128,), 14, 0.1, 1.0), rnd((128,), 15, 0.1, 1.0)
    ang = torch.rand(64, generator=torch.Generator().manual_seed(16 + L)) * 6.0
    rope = torch.cat([torch.cos(ang), torch.sin(ang)]).to(torch.bfloat16).float().cuda().contiguous()
    scale = float(torch.tensor(128 ** -0.5).to(torch.bfloat16))
    o = ops.debug_attn_decode_fused(qkv, qn, kn, rope, ptrs, L, heads, kv_heads, 1e-6, scale)
    torch.cuda.synchronize()
    return sha(bits(o), bits(pool))


def make_model(heads, kv_heads):
    from aha_amd.configs import tiny_qwen3
    from aha_amd.model import HipInferenceModel
    from aha_amd.weights import qwen3_text_weights
    cfg = tiny_qwen3(layers=1, hidden=512, heads=heads, kv_heads=kv_heads, inter=1024, vocab=2048)
    return HipInferenceModel(cfg, qwen3_text_weights(cfg, seed=3))


def attn_linear_case(m, L):
    """One decode step that leaves the cache L long, on a fresh request of `m`: (digest of the token and the logits, form, cache length).
    L = 1: the step runs on the empty cache (no prefill)."""
    m.clear_cache()
    if L == 1:
        tok = 7
    else:
        g = torch.Generator().manual_seed(2000 + L)
        _, tok = m.forward_initial(torch.randint(0, 1900, (L - 1,), generator=g).tolist(), 0, want_logits=False)
    toks = m.decode_greedy(tok, L - 1, 1)
    return sha(np.asarray([int(tok)] + toks, np.uint32), m.last_logits()), m.debug_attn_decode_form(), m.cache_len()


def compute() -> dict:
    out = {}
    for N, K in GEMV_SHAPES:
        out.update(gemv_case(N, K))
    for heads, kv_heads in HEAD_SHAPES:
        for L in CACHE_LENS:
            out[attn_key(TABLE, heads, kv_heads, L)] = attn_table_case(heads, kv_heads, L)
        m = make_model(heads, kv_heads)
        for L in CACHE_LENS:
            dig, form, n = attn_linear_case(m, L)
            assert form == LINEAR and n == L, (heads, kv_heads, L, form, n)
            out[attn_key(LINEAR, heads, kv_heads, L)] = dig
        m.close()
    return out


if __name__ == "__main__":
    res = compute()
    print(json.dumps(res, indent=1))
    if len(sys.argv) > 1:
        os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
        with open(sys.argv[1], "w") as f:
            json.dump(res, f, indent=1, sort_keys=True)
