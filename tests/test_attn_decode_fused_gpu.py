"""-m gpu: the fused decode attention (attn_decode_fused_body, aha_amd/csrc/attn_decode_body.h) against an f64 reference of the operation.

The kernel under test is the one every decode step runs: q/k RMSNorm + RoPE from a table + KV append + split-KV attention over
fragment-major pages + the four-wave merge through LDS + the merge of the splits by the last block to arrive.  It is reached through
ops.attn_decode_batch (all cache lengths of a head shape as rows of ONE launch) and, for the lengths {1, 65, 257, 4097}, through
ops.debug_attn_decode_fused (the single-sequence entry) as well.  (ops.attn_decode, which tests/test_ops_gpu.py covers, is the
three-launch fallback.)

Reference (fused_ref): torch f64 on the CPU from the same inputs -- norm, rotate-half RoPE, q and k rounded to bf16 at the model dtype's
materialisation points (the ones oracle.qwen3.rms_norm / apply_rotary_pos_emb have, i.e. test_qknorm_rope's reference: the norm's output,
the two RoPE products, their sum; each rounded once, everything between them in f64), then scores, softmax and P.V in f64 without any
rounding.  tests/test_kv_pages_cpu.py holds it against oracle.qwen3 without a kernel involved.

Inputs: every element of the page pool starts as finite garbage (normal x 100, bf16), so a slot the kernel must not read (page tails
past the cache length, spare pages) is loud if read; the cached tokens are then written with tests/kv_pages.pack_pages, and the pages of
a row are a seeded permutation of the pool.

Bound: 3 bf16 ulps, the project's stated bound for decode attention (test_ops_gpu.py::test_attn_decode), per head at the head's largest
|output| and for the row at its rms.  The shapes are the smallest that reach each path of the kernel, none is a workload shape: group
sizes g = 1, 2, 3, 4, 5, 8, 16 (a second prologue round from g = 4, more merge items than threads above g = 8, the k head on wave 1 at
g = 1), empty waves (kv_len <= 193), an empty split (257), 5 and 17 splits (1025, 4097: the second merge batch), 64 splits with a second
page on unit 0 only (16449), units with 2 and 3 pages (40000).  At 257, 1025 and 4097 the LAST split is the empty one and at 16449 and
40000 the split count is a multiple of 16, so an error in how the merge weighs or re-reads its last partial would pass all of them
(tried: a weight guard of `s0 + j <= nsplit`); 300 (2 splits, the last with one page) and 4500 (18 splits, the last with three pages, in
the second merge batch) are there for that.

Measured on an MI355X: worst distance from the bf16-rounded f64 reference in bf16 ulps, "per-head scale / row-rms scale", per
(g, kv_len); g = 4 is the larger of (8, 2) and (32, 8), g = 8 is (8, 1):

  kv_len        g = 1       g = 2       g = 3       g = 4       g = 5       g = 8      g = 16
       1  0.00 / 0.00 0.00 / 0.00 0.00 / 0.00 0.00 / 0.00 0.00 / 0.00 0.00 / 0.00 0.00 / 0.00
       2  0.50 / 1.00 0.50 / 1.00 1.00 / 1.50 1.00 / 1.50 1.00 / 2.25 1.00 / 1.00 0.50 / 1.00
      64  0.50 / 1.00 0.50 / 1.50 1.00 / 1.00 1.00 / 2.50 1.00 / 1.00 1.00 / 1.00 1.00 / 1.50
      65  1.00 / 1.00 1.00 / 1.00 1.00 / 1.00 1.00 / 1.00 1.00 / 2.00 1.00 / 1.00 1.00 / 1.00
      66  1.00 / 1.75 1.00 / 1.00 1.00 / 1.00 1.00 / 1.00 1.00 / 1.00 1.00 / 1.50 1.00 / 1.00
     129  1.00 / 1.00 1.00 / 1.00 1.00 / 1.00 1.00 / 1.00 1.00 / 1.00 1.00 / 1.00 1.00 / 1.50
     193  0.50 / 1.00 0.50 / 1.00 1.00 / 1.00 1.00 / 1.00 1.00 / 1.00 1.00 / 1.09 1.00 / 1.00
     257  1.00 / 1.00 1.00 / 1.00 1.00 / 1.00 1.00 / 1.00 1.00 / 1.00 1.00 / 1.00 1.00 / 1.25
     300  0.50 / 1.00 1.00 / 1.00 1.00 / 1.00 1.00 / 2.00 1.00 / 1.00 1.00 / 1.00 1.00 / 1.00
    1025  1.00 / 1.00 0.50 / 1.00 1.00 / 1.00 1.00 / 1.00 1.00 / 1.00 1.00 / 1.00 1.00 / 1.18
    4097  0.50 / 1.00 1.00 / 1.00 1.00 / 1.00 1.00 / 1.00 1.00 / 1.00 1.00 / 1.00 1.00 / 1.00
    4500  1.00 / 1.00 0.50 / 1.00 1.00 / 1.00 1.00 / 1.00 1.00 / 1.00 1.00 / 1.00 1.00 / 1.00
   16449            -           -           - 1.00 / 1.00           - 1.00 / 1.00 1.00 / 1.00
   40000            -           -           - 1.00 / 1.00           - 1.00 / 1.00 1.00 / 1.00

Peaky and uniform cases (per-head scale), (8, 2) at 700 / (16, 1) at 4097: page0 1 / 1, last_page 1 / 1, new_token 1 / 1,
new_token_far_below 3 / 2, uniform 0 / 0.  The 3 is head 1 of the (8, 2) case, not head 0: for the other heads k_new = -7 q_0 is a key
like any other with a wide score spread, and head 1 gives the new token a score of 4.67 and a probability of 0.08.  The kernel scores the
new token as bf16(bf16(q.k) * scale) (the reference implementation's rounding points for every score, modules.rs:782-783) = 4.656, the
cached tokens in f32; that 0.014 alone moves the unrounded output by 2.9 ulp of the head's scale.  The mixed convention is inside the
3-ulp bound on every case here, but it is what uses the bound up: an error of up to 2^-8 of the new token's score times p (1 - p) |dV|.
"""
import functools
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kv_pages  # noqa: E402
from rope_ref import D, SPARE_PAGES, Pool, _r, norm_rope_ref, norm_weights, prologue_ref, prologue_rows_ref, rnd  # noqa: E402,F401
from test_ops_gpu import assert_close_ulps, ulp_bf16  # noqa: E402

pytestmark = pytest.mark.gpu

EPS = 1e-6
ULPS = 3                       # test_ops_gpu.py::test_attn_decode
K_ULPS, K_EXACT = 2, 0.97      # test_ops_gpu.py::test_qknorm_rope
SHAPES = [(2, 2), (4, 2), (6, 2), (8, 2), (5, 1), (8, 1), (16, 1), (32, 8)]
LENS = [1, 2, 64, 65, 66, 129, 193, 257, 300, 1025, 4097, 4500]
LONG_SHAPES = [(8, 2), (8, 1), (16, 1)]
LONG_LENS = [16449, 40000]
SINGLE_LENS = [1, 65, 257, 4097]   # also through the single-sequence entry


def lens_of(nh, kvh):
    return LENS + (LONG_LENS if (nh, kvh) in LONG_SHAPES else [])


def bf16_scale():
    return float(torch.tensor(D ** -0.5).to(torch.bfloat16))


# ---- the reference ---------------------------------------------------------------------------------------------------------------
def fused_ref(qkv_row, q_norm_w, k_norm_w, rope_row, k_cache, v_cache, nh, kvh, eps, scale):
    """The fused decode attention of one sequence in f64.  k_cache, v_cache: (kv_len - 1, kvh * 128) bf16, the tokens already cached.
    -> (o (nh * 128) f64, k_new (kvh * 128) bf16, v_new (kvh * 128) bf16)."""
    g = nh // kvh
    q, k_new, v_new = prologue_ref(qkv_row, q_norm_w, k_norm_w, rope_row, nh, kvh, eps)
    K = torch.cat([k_cache.view(-1, kvh, D), k_new[None]]).double()
    V = torch.cat([v_cache.view(-1, kvh, D), v_new[None]]).double()
    qg = q.double().view(kvh, g, D)                                  # head h uses kv head h // g
    p = torch.softmax(torch.einsum("kgd,lkd->kgl", qg, K) * scale, -1)
    o = torch.einsum("kgl,lkd->kgd", p, V)
    return o.reshape(nh * D), k_new.reshape(-1), v_new.reshape(-1)


# ---- inputs ----------------------------------------------------------------------------------------------------------------------
def rope_rows(R, seed=10):
    ang = torch.rand(R, 64, generator=torch.Generator().manual_seed(seed)) * 6.0
    return torch.cat([torch.cos(ang), torch.sin(ang)], 1).to(torch.bfloat16).float().contiguous()


def ulp_distance(got, ref, scale):
    return float(((got.float() - ref.float()).abs() / ulp_bf16(torch.maximum(ref.float().abs(), scale))).max())


def check_rows(what, rows, lens, nh, kvh, o, ref_o, ref_k, qkv, pool, report=False):
    """Every assertion on the rows `rows` of one launch: o (R, nh * 128) bf16 on the CPU, the pool on the device as the launch left it."""
    g = nh // kvh
    for r in rows:
        L = lens[r]
        got, ref = o[r].float(), ref_o[r].to(torch.bfloat16).float()
        if report:
            d_head = ulp_distance(got.view(nh, D), ref.view(nh, D), ref.view(nh, D).abs().amax(-1, keepdim=True))
            d_rms = ulp_distance(got, ref, ref.pow(2).mean().sqrt())
            print(f"ULP nh={nh} kvh={kvh} g={g} kv_len={L} head={d_head:.3f} rms={d_rms:.3f}")
    changed = pool.changed()
    allowed = torch.cat([pool.slot_elems(r)[0] for r in rows])
    assert torch.isin(changed, allowed).all(), f"{what}: {int((~torch.isin(changed, allowed)).sum())} pool elements outside the appended slots changed"
    k_got = []
    for r in rows:
        L = lens[r]
        got, ref = o[r], ref_o[r].to(torch.bfloat16)
        assert_close_ulps(got.view(nh, D), ref.view(nh, D), ULPS, None, f"{what}: kv_len {L}, per head", row_scale=True)
        assert_close_ulps(got, ref, ULPS, None, f"{what}: kv_len {L}, row rms")
        v_row = qkv[r, (nh + kvh) * D:]
        if L == 1:   # p = 1 and sum = 1: the output IS the new v
            assert torch.equal(got.view(kvh, g, D).view(torch.int16), v_row.view(kvh, 1, D).expand(kvh, g, D).contiguous().view(torch.int16)), \
                f"{what}: kv_len 1 must return the new v bit for bit"
        _, pg, t = pool.slot_elems(r)
        k_slot, v_slot = kv_pages.unpack_slot(pool.dev[pg].cpu(), kvh, t)
        assert torch.equal(v_slot.view(torch.int16), v_row.view(torch.int16)), f"{what}: kv_len {L}: appended v differs from the qkv row's"
        assert_close_ulps(k_slot, ref_k[r], K_ULPS, None, f"{what}: kv_len {L}: appended k")
        k_got.append(k_slot)
    k_got, k_ref = torch.stack(k_got), torch.stack([ref_k[r] for r in rows])
    exact = float((k_got.float() == k_ref.float()).float().mean())
    assert exact >= K_EXACT, f"{what}: only {exact:.4f} of the appended k bit-identical to the reference"


@functools.lru_cache(maxsize=None)
def case(nh, kvh):
    """Inputs and reference of one head shape, built once: every cache length is one sequence of the pool and one row of the launch."""
    lens = lens_of(nh, kvh)
    R = len(lens)
    pool = Pool(kvh, lens, 5)
    qkv = rnd((R, (nh + 2 * kvh) * D), 7)
    qn, kn = norm_weights()
    rope = rope_rows(R)
    scale = bf16_scale()
    ref_o, ref_k = [], []
    for r, L in enumerate(lens):
        kc, vc = rnd((L - 1, kvh * D), 100 + r), rnd((L - 1, kvh * D), 200 + r)
        pool.write(r, kc, vc)
        o, k_new, _ = fused_ref(qkv[r], qn, kn, rope[r], kc, vc, nh, kvh, EPS, scale)
        ref_o.append(o)
        ref_k.append(k_new)
    return dict(nh=nh, kvh=kvh, lens=lens, pool=pool, qkv=qkv, qn=qn, kn=kn, rope=rope, scale=scale, ref_o=ref_o, ref_k=ref_k)


def launch_batch(c, rows=None):
    from aha_amd import ops
    rows = list(range(len(c["lens"]))) if rows is None else rows
    pool = c["pool"]
    o = ops.attn_decode_batch(c["qkv"][rows].contiguous().to("cuda"), c["qn"].to("cuda"), c["kn"].to("cuda"), c["rope"][rows].contiguous().to("cuda"),
                              pool.ptrs, [pool.page0[r] for r in rows], [c["lens"][r] for r in rows], c["nh"], c["kvh"], EPS, c["scale"])
    torch.cuda.synchronize()
    return o.cpu()


# ---- tests -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nh,kvh", SHAPES)
def test_batch_launch_against_the_f64_reference(gpu, nh, kvh):
    """All cache lengths of the head shape as rows of one launch: output, kv_len 1, the append and the untouched rest of the pool; the
    same launch again on the restored pool gives the same bits (the merging block is whichever arrives last)."""
    c = case(nh, kvh)
    pool = c["pool"]
    pool.upload()
    try:
        o = launch_batch(c)
        check_rows(f"batch nh {nh} kvh {kvh}", range(len(c["lens"])), c["lens"], nh, kvh, o, c["ref_o"], c["ref_k"], c["qkv"], pool, report=True)
        after = pool.dev.clone()
        pool.restore()
        o2 = launch_batch(c)
        assert torch.equal(o.view(torch.int16), o2.view(torch.int16)), "the same launch twice gave different output bits"
        assert torch.equal(after.view(torch.int16), pool.dev.view(torch.int16)), "the same launch twice gave different appends"
    finally:
        del pool.dev, pool.before, pool.ptrs


@pytest.mark.parametrize("nh,kvh", SHAPES)
def test_single_sequence_entry_against_the_f64_reference(gpu, nh, kvh):
    from aha_amd import ops
    c = case(nh, kvh)
    pool, lens = c["pool"], c["lens"]
    pool.upload()
    try:
        rows = [lens.index(L) for L in SINGLE_LENS]
        o = {}
        qn, kn = c["qn"].to("cuda"), c["kn"].to("cuda")
        for r in rows:
            o[r] = ops.debug_attn_decode_fused(c["qkv"][r].contiguous().to("cuda"), qn, kn, c["rope"][r].contiguous().to("cuda"),
                                               pool.ptrs[pool.page0[r]:].contiguous(), lens[r], nh, kvh, EPS, c["scale"]).cpu()
        torch.cuda.synchronize()
        check_rows(f"single nh {nh} kvh {kvh}", rows, lens, nh, kvh, o, c["ref_o"], c["ref_k"], c["qkv"], pool)
    finally:
        del pool.dev, pool.before, pool.ptrs


PEAKY_SHAPES = [(8, 2, 700), (16, 1, 4097)]
PEAKY_KINDS = ["page0", "last_page", "new_token", "new_token_far_below", "uniform"]


@pytest.mark.parametrize("kind", PEAKY_KINDS)
@pytest.mark.parametrize("nh,kvh,L", PEAKY_SHAPES)
def test_peaky_and_uniform_scores(gpu, nh, kvh, L, kind):
    """Large score spreads, where the online softmax's rescaling and the merges' weights do the work.  One key is 2 x (q of head 0),
    a score of about 2 * 128 / sqrt(128) = 22 against a spread of 1: in page 0; in the last cached page; as the new token itself (all
    that was accumulated is rescaled by the final step); a new token about 80 below the maximum (its probability vanishes).  Uniform:
    every cached k and the new one are 0, the output is the plain mean of V."""
    qkv = rnd((1, (nh + 2 * kvh) * D), 40)
    qn, kn = norm_weights()
    rope = rope_rows(1, 41)
    scale = bf16_scale()
    kc, vc = rnd((L - 1, kvh * D), 42), rnd((L - 1, kvh * D), 43)
    q_raw0 = qkv[0, :D].clone()
    if kind in ("page0", "last_page"):
        q = prologue_ref(qkv[0], qn, kn, rope[0], nh, kvh, EPS)[0]
        kc[5 if kind == "page0" else L - 7] = (q[0].float() * 2.0).to(torch.bfloat16).repeat(kvh)
    elif kind == "new_token":            # the k heads are q head 0 under twice the q norm weight: k_new = 2 q exactly
        qkv[0, nh * D: (nh + kvh) * D] = q_raw0.repeat(kvh)
        kn = (qn.float() * 2.0).to(torch.bfloat16)
    elif kind == "new_token_far_below":  # k_new = -7 q: its score is about -7 * 128 * scale = -79, the others' within a few units of 0
        qkv[0, nh * D: (nh + kvh) * D] = q_raw0.repeat(kvh)
        kn = (qn.float() * -7.0).to(torch.bfloat16)
    else:
        kc.zero_()
        kn = torch.zeros_like(kn)
    ref_o, ref_k, _ = fused_ref(qkv[0], qn, kn, rope[0], kc, vc, nh, kvh, EPS, scale)
    if kind == "uniform":
        assert not ref_k.any()
        mean_v = torch.cat([vc, qkv[:, (nh + kvh) * D:]]).double().view(L, kvh, 1, D).mean(0).expand(kvh, nh // kvh, D).reshape(-1)
        assert torch.allclose(ref_o, mean_v, rtol=0, atol=1e-12)
    pool = Pool(kvh, [L], 44)
    pool.write(0, kc, vc)
    pool.upload()
    c = dict(nh=nh, kvh=kvh, lens=[L], pool=pool, qkv=qkv, qn=qn, kn=kn, rope=rope, scale=scale)
    o = launch_batch(c)
    got, ref = o[0].float(), ref_o.to(torch.bfloat16).float()
    print(f"ULP-PEAKY nh={nh} kvh={kvh} kv_len={L} {kind} head={ulp_distance(got.view(nh, D), ref.view(nh, D), ref.view(nh, D).abs().amax(-1, keepdim=True)):.3f}")
    check_rows(f"{kind} nh {nh} kvh {kvh}", [0], [L], nh, kvh, o, [ref_o], [ref_k], qkv, pool)
