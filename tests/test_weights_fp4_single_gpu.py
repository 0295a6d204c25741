"""-m gpu: single-sequence decode from MXFP4 weights (gemv_mxfp4_kernel) is the bf16 matvec on the dequantised weights, bit for bit.

  1. ops.gemv_mxfp4(q, s, x, ...) == ops.gemv_epi(W', x, ...) on every output bit (and the argmax) for (q, s, W') of the reference
     quantiser, every epilogue, with and without norm weights, over shapes that between them select EVERY instantiation the library ships
     (asserted through the plan query) -- the two kernels' plans differ in R, U and grid, so this is also the proof that a row's bits do
     not depend on them, and the hardware's E2M1 conversion is held to the reference's table, -0.0 for the code 0x8 included;
  2. a model quantised in place equals a model created from the reference's W' through forward_initial + forward_step, decode_greedy and
     a seeded generate_generic loop, while its profile shows gemv_fp4 launches (4 per layer and step, plus the head with lm_head) and
     never a gemv_fp8 one; the switch aha_hip_debug_fp4_single in its three values; the argmax partials of the kernel that ran;
  3. aha_hip_gemv_mxfp4 refuses bad arguments before anything is launched.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

from aha_amd._lib import AhaHipError
from aha_amd.configs import tiny_qwen3
from aha_amd.weights import qwen3_text_weights

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_weights_fp4_cpu import bf16_bits  # noqa: E402
from test_weights_fp4_gpu import bits, prompts, reference_weights  # noqa: E402
from test_weights_fp4_single_cpu import shipped  # noqa: E402
from test_weights_fp8_single_gpu import MULTI_TILE_FAST, SHAPES, cases_of  # noqa: E402  (the plans select alike: 16 loads per buffer)

pytestmark = pytest.mark.gpu

STORE, RESIDUAL, SILU_MUL, LOGITS = 0, 1, 2, 3


def test_the_shapes_select_every_shipped_instantiation(hip_lib):
    from aha_amd import ops
    for want in ((40, 160), (4100, 1024), (8224, 512), (16416, 256), (64, 4096), (64, 12288), (32, 16896), (64, 1056), (100000, 64)):
        assert want in SHAPES
    assert MULTI_TILE_FAST == [(16416, 512), (16416, 1024), (16416, 2048), (16416, 4096), (6400, 4096)] and set(MULTI_TILE_FAST) <= set(SHAPES)
    hit = set()
    for N, K in SHAPES:
        for epi, norm in cases_of(N, K):
            r, u, grid, form = ops.plan_gemv_mxfp4(N, K, epi, norm)
            hit.add((r, u, epi, int(form != 0), max(form - 1, 0)))
    assert hit == shipped(), (sorted(shipped() - hit), sorted(hit - shipped()))
    # the FAST forms walk several tiles per block, for every epilogue, with and without norm weights
    for N, K in MULTI_TILE_FAST:
        for epi, norm in cases_of(N, K):
            r, u, grid, form = ops.plan_gemv_mxfp4(N, K, epi, norm)
            rows = N // 2 if epi == SILU_MUL else N
            assert -(-rows // (4 * r)) > grid and form != 0, (N, K, epi, norm, r, u, grid, form)
    # and the general form does
    assert ops.plan_gemv_mxfp4(16416, 256, LOGITS, False)[:3] == (4, 1, 768) and ops.plan_gemv_mxfp4(100000, 64, STORE, False)[2] == 768


_CASES = {}


def kernel_case(gpu, N, K):
    """The reference's (q, scales, W') of a seeded W on the GPU, x, a residual and norm weights; built once per shape."""
    if (N, K) not in _CASES:
        from aha_amd import quant
        g = torch.Generator().manual_seed(2000 + N + K)
        # per-block magnitudes spread over 2^-6 .. 2^2 so that the scales differ from block to block
        W = (torch.randn(N, K, generator=g) * torch.exp2(torch.randint(-6, 3, (N, K // 32, 1), generator=g).float()).expand(N, K // 32, 32)
             .reshape(N, K) * 0.05).bfloat16()
        q, s, wr = quant.quantize_mxfp4(W)
        x = torch.randn(K, generator=g).bfloat16()
        res = torch.randn(N, generator=g).bfloat16()
        nw = (1.0 + 0.1 * torch.randn(K, generator=g)).bfloat16()
        _CASES.clear()       # one shape resident at a time
        _CASES[(N, K)] = tuple(t.to(gpu) for t in (q, s, wr, x, res, nw))
    return _CASES[(N, K)]


@pytest.mark.parametrize("N,K", SHAPES)
def test_fp4_matvec_is_bit_identical_to_bf16_matvec_on_dequantised_weights(gpu, N, K):
    from aha_amd import ops
    q, s, wr, x, res, nw = kernel_case(gpu, N, K)
    # the case holds what the conversion must get right: every code, -0 among them (W' holds -0.0 there), and scales that differ
    assert int(((q & 0xf) == 8).sum()) + int(((q >> 4) == 8).sum()) > 0 and int((bf16_bits(wr) == -32768).sum()) > 0
    assert len(torch.unique(q & 0xf)) == 16 and len(torch.unique(s)) >= 5
    for epi, norm in cases_of(N, K):
        kw = dict(norm_w=nw if norm else None, eps=1e-6, residual=res if epi == RESIDUAL else None)
        got = ops.gemv_mxfp4(q, s, x, epi, **kw)
        want = ops.gemv_epi(wr, x, epi, **kw)
        if epi == LOGITS:
            assert got[0].shape == (N,) and torch.equal(got[0].view(torch.int32), want[0].view(torch.int32)), (epi, norm)
            assert got[1] == want[1] == int(torch.argmax(want[0])), (epi, norm)       # the first maximal index
            got = got[0]
        else:
            assert got.shape == (N // 2 if epi == SILU_MUL else N,) and torch.equal(bf16_bits(got), bf16_bits(want)), (epi, norm)
        assert bool(torch.isfinite(got.float()).all()), (epi, norm)
        assert bool((got.float() != 0).any())
        if epi == RESIDUAL:      # the output aliasing the residual
            ya, yb = res.clone(), res.clone()
            ops.gemv_mxfp4(q, s, x, epi, norm_w=kw["norm_w"], residual=ya, out=ya)
            ops.gemv_epi(wr, x, epi, norm_w=kw["norm_w"], residual=yb, out=yb)
            assert torch.equal(bf16_bits(ya), bf16_bits(yb)) and torch.equal(bf16_bits(ya), bf16_bits(got)), norm


def test_every_code_at_the_extreme_block_exponents(gpu):
    """One-hot activations read single weights back: all 16 codes at the scale bytes 2, 127 and 252 (e = -125, 0, 125) come out with the
    magnitude the reference dequantiser gives, and with the bits of the bf16 kernel on W' (y = bf16(1 * w + 0): exact, W' is bf16; the
    sign of a zero is lost in the sum, the shapes above hold it)."""
    from aha_amd import ops, quant
    row = np.resize(np.array([lo | hi << 4 for lo, hi in zip(range(0, 16, 2), range(1, 16, 2))], dtype=np.uint8), 48)     # 96 k: 3 blocks
    q = torch.from_numpy(np.tile(row, (32, 1)).copy())
    s = torch.tensor([[2, 127, 252]], dtype=torch.uint8).repeat(32, 1)
    wr = quant.dequantize_mxfp4(q, s)
    assert float(wr.float().abs().max()) == 6.0 * 2.0 ** 125 and float(wr.float().abs()[wr != 0].min()) == 2.0 ** -126
    qg, sg, wg = q.to(gpu), s.to(gpu), wr.to(gpu)
    for k in range(96):
        x = torch.zeros(96, dtype=torch.bfloat16)
        x[k] = 1.0
        xg = x.to(gpu)
        got = ops.gemv_mxfp4(qg, sg, xg, STORE)
        assert torch.equal(bf16_bits(got), bf16_bits(ops.gemv_epi(wg, xg, STORE))), k
        assert torch.equal(got.float().cpu(), wr[:, k].float() + 0.0), k


# ---- 2. the model ----------------------------------------------------------------------------------------------------------------
def classes(m):
    return {c: m.get_profile(c)["launches"] for c in ("gemv", "gemv_fp4", "gemv_fp8")}


def profiled_decode(m, first, offset, new):
    """decode_greedy under a fresh profile: (tokens, {class: launches})."""
    m.set_profiling(True)
    toks = m.decode_greedy(first, offset, new)
    prof = classes(m)
    m.set_profiling(False)
    return toks, prof


def greedy_run(m, ids, new):
    m.clear_cache()
    _, tok = m.forward_initial(ids, 0)
    toks, prof = profiled_decode(m, tok, len(ids), new)
    return [tok] + toks, prof, m.last_logits().copy()


# hidden 256 / inter 512: every matvec in the general or a short straight-line form; hidden 1024 / inter 2048: U = 2 and 4 straight-line
@pytest.mark.parametrize("hidden,heads,inter", [(256, 4, 512), (1024, 8, 2048)])
@pytest.mark.parametrize("tie,lm_head", [(True, False), (True, True), (False, False), (False, True)])
def test_quantised_model_decodes_single_sequences_as_the_model_created_from_dequantised_weights(gpu, hidden, heads, inter, tie, lm_head):
    from aha_amd import ops
    from aha_amd import sampling as hs
    from aha_amd.model import HipInferenceModel
    cfg = tiny_qwen3(layers=2, hidden=hidden, heads=heads, kv_heads=2, inter=inter, vocab=1024, tie=tie)
    w = qwen3_text_weights(cfg, seed=41)
    A = HipInferenceModel(cfg, w)
    B = HipInferenceModel(cfg, reference_weights(w, tie, lm_head))
    try:
        A.quantize_weights("mxfp4", lm_head=lm_head)
        # by default the plan keeps matrices this small on the bf16 kernel (ops.gemv_mxfp4_by_plan): 2 = every matrix with a copy
        A.debug_fp4_single(2)
        L = cfg.num_hidden_layers
        ids = prompts(12, (37,))[0]

        def steps(m):
            m.clear_cache()
            lg, tok = m.forward_initial(ids, 0)
            out = [(lg.copy(), tok)]
            for i in range(6):
                lg, tok = m.forward_step(tok, len(ids) + i)
                out.append((lg.copy(), tok))
            return out

        for (la, ta), (lb, tb) in zip(steps(A), steps(B)):
            assert ta == tb and np.array_equal(bits(la), bits(lb))

        ga, pa, lga = greedy_run(A, ids, 24)
        gb, pb, lgb = greedy_run(B, ids, 24)
        assert ga == gb and len(ga) == 25 and np.array_equal(bits(lga), bits(lgb))
        # B: gemv only; 4 matvecs per layer and step plus one head per step.  A: the layer matvecs (and the head with lm_head) as gemv_fp4.
        n_steps = pb["gemv"] // (4 * L + 1)
        assert pb == {"gemv": n_steps * (4 * L + 1), "gemv_fp4": 0, "gemv_fp8": 0} and n_steps >= 24, pb
        assert pa == ({"gemv": 0, "gemv_fp4": n_steps * (4 * L + 1), "gemv_fp8": 0} if lm_head else
                      {"gemv": n_steps, "gemv_fp4": n_steps * 4 * L, "gemv_fp8": 0}), (pa, pb)

        def sampled(m):
            m.clear_cache()
            ctx = hs.GenerationContext(0.8, 0.9, 20, 1.1, 64, seed=17, initial_seq_len=len(ids), max_tokens=12)
            toks = hs.generate_generic_sampled(m, ids, ctx)
            return toks, m.last_logits().copy()

        sa, lsa = sampled(A)
        sb, lsb = sampled(B)
        assert sa == sb and len(sa) == 12 and np.array_equal(bits(lsa), bits(lsb))
        # the switch: the bf16 kernel on W' -- B's classes, the same bits
        A.debug_fp4_single(0)
        go, po, lgo = greedy_run(A, ids, 24)
        assert po == pb and go == ga and np.array_equal(bits(lgo), bits(lga))
        A.debug_fp4_single(2)
        assert greedy_run(A, ids, 24)[1] == pa
        # the FP8 switch reads FP8 copies only: it moves nothing here
        A.debug_fp8_single(0)
        assert greedy_run(A, ids, 24)[1] == pa
        A.debug_fp8_single(1)
        # the default: by plan, and the plan takes none of these shapes -- bf16 launches, the same bits again
        assert not any(ops.gemv_mxfp4_by_plan(n, k, e) for n, k, e in ((hidden + 4 * 128, hidden, STORE), (hidden, heads * 128, RESIDUAL),
                                                                        (2 * inter, hidden, SILU_MUL), (hidden, inter, RESIDUAL), (1024, hidden, LOGITS)))
        A.debug_fp4_single(1)
        gd, pd, lgd = greedy_run(A, ids, 24)
        assert pd == pb and gd == ga and np.array_equal(bits(lgd), bits(lga))
        with pytest.raises(AhaHipError) as e:
            A.debug_fp4_single(3)
        assert e.value.code == -1 and "debug_fp4_single: on must be 0 (bf16), 1 (by plan) or 2" in str(e.value)
    finally:
        A.close()
        B.close()


def test_argmax_partials_follow_the_grid_of_the_kernel_that_ran(gpu):
    """Vocabulary 10000: the FP4 lm_head writes 625 (max, index) partials, the bf16 one 768.  The device-resident loop's fused tail and the
    argmax launch of forward_step must reduce the count of the kernel that ran: a bf16 pass first leaves 768 real partials of other
    steps behind, which a reduction over the wrong count would pick up."""
    from aha_amd import ops
    from aha_amd.model import HipInferenceModel
    assert ops.plan_gemv_mxfp4(10000, 256, LOGITS, True)[2] == 625 != 768
    cfg = tiny_qwen3(layers=2, hidden=256, heads=4, kv_heads=2, inter=512, vocab=10000, tie=False)
    w = qwen3_text_weights(cfg, seed=43)
    A = HipInferenceModel(cfg, w)
    B = HipInferenceModel(cfg, reference_weights(w, False, True))
    try:
        A.quantize_weights("mxfp4", lm_head=True)
        ids = prompts(14, (29,))[0]
        gb, pb, lgb = greedy_run(B, ids, 24)
        assert len(set(gb)) > 4      # the tokens move: a stale partial would not go unnoticed
        for mode in (0, 2, 0, 2):
            A.debug_fp4_single(mode)
            ga, pa, lga = greedy_run(A, ids, 24)
            assert ga == gb and np.array_equal(bits(lga), bits(lgb)), mode
            assert (pa["gemv_fp4"] > 0) == (mode == 2) and pa["gemv_fp8"] == 0
            A.clear_cache()
            _, tok = A.forward_initial(ids, 0)
            B.clear_cache()
            B.forward_initial(ids, 0)
            for i in range(3):       # the launch-per-step path: enqueue_lm_head's own argmax launch
                la, ta = A.forward_step(tok, len(ids) + i)
                lb, tb = B.forward_step(tok, len(ids) + i)
                assert ta == tb == int(np.argmax(lb)) and np.array_equal(bits(la), bits(lb)), (mode, i)
                tok = ta
    finally:
        A.close()
        B.close()


def test_default_switch_follows_the_measured_plan(gpu):
    """The default (by plan) in a model whose untied lm_head of 16416 x 1024 the plan takes (1026 tiles on 768 blocks, the multi-tile LOGITS
    walk): the head runs as gemv_fp4, the small layer matrices as gemv; the same tokens and logit bits as the model made of W'."""
    from aha_amd import ops
    from aha_amd.model import HipInferenceModel
    assert ops.gemv_mxfp4_by_plan(16416, 1024, LOGITS) and ops.plan_gemv_mxfp4(16416, 1024, LOGITS, True) == (4, 2, 768, 3)
    assert not ops.gemv_mxfp4_by_plan(16416, 1056, LOGITS)       # as large, but the general form: kept on bf16
    cfg = tiny_qwen3(layers=2, hidden=1024, heads=8, kv_heads=2, inter=2048, vocab=16416, tie=False)
    w = qwen3_text_weights(cfg, seed=44)
    A = HipInferenceModel(cfg, w)
    B = HipInferenceModel(cfg, reference_weights(w, False, True))
    try:
        A.quantize_weights("mxfp4", lm_head=True)
        L = cfg.num_hidden_layers
        ids = prompts(15, (33,))[0]
        gb, pb, lgb = greedy_run(B, ids, 16)
        ga, pa, lga = greedy_run(A, ids, 16)
        assert ga == gb and np.array_equal(bits(lga), bits(lgb))
        n_steps = pb["gemv"] // (4 * L + 1)
        assert pb["gemv_fp4"] == 0 and pa == {"gemv": n_steps * 4 * L, "gemv_fp4": n_steps, "gemv_fp8": 0}, (pa, pb)
    finally:
        A.close()
        B.close()


def test_models_without_fp4_copies_never_launch_the_fp4_matvec(gpu):
    from aha_amd.model import HipInferenceModel
    cfg = tiny_qwen3(layers=2, hidden=256, heads=4, kv_heads=2, inter=512, vocab=1024)
    w = qwen3_text_weights(cfg, seed=42)
    wn = {k: v.clone() for k, v in w.items()}
    wn["model.layers.1.mlp.down_proj.weight"][5, 77] = float("nan")
    plain, refused, fp8 = HipInferenceModel(cfg, w), HipInferenceModel(cfg, wn), HipInferenceModel(cfg, w)
    try:
        with pytest.raises(AhaHipError):
            refused.quantize_weights("mxfp4", lm_head=True)
        fp8.quantize_weights("mxfp8", lm_head=True)
        ids = prompts(13, (20,))[0]
        L = cfg.num_hidden_layers
        for m in (plain, refused, fp8):
            m.debug_fp4_single(2)             # nothing to take: no FP4 copy
            m.forward_initial(ids, 0)
            m.set_profiling(True)
            m.forward_step(7, len(ids))       # a fixed token: the refused model's logits are NaN
            got = classes(m)
            assert got["gemv_fp4"] == 0 and got["gemv"] + got["gemv_fp8"] == 4 * L + 1 and (got["gemv_fp8"] == 0 or m is fp8), got
            m.set_profiling(False)
        toks, prof = profiled_decode(plain, 7, len(ids) + 1, 4)
        assert prof["gemv_fp4"] == 0 and prof["gemv"] >= 4 * (4 * L + 1) and len(toks) == 4, prof
        fp8.debug_fp8_single(2)
        toks, prof = profiled_decode(fp8, 7, len(ids) + 1, 4)
        assert prof["gemv_fp4"] == 0 and prof["gemv_fp8"] >= 4 * (4 * L + 1) and len(toks) == 4, prof
    finally:
        plain.close()
        refused.close()
        fp8.close()


# ---- 3. errors -------------------------------------------------------------------------------------------------------------------
def test_gemv_mxfp4_refuses_bad_arguments_before_any_launch(gpu):
    from aha_amd import _lib, ops
    L = _lib.lib()
    q = torch.zeros(32, 32, dtype=torch.uint8, device=gpu)
    words = torch.full((32, 1), 0x7f7f7f7f, dtype=torch.int32, device=gpu)
    x = torch.ones(64, dtype=torch.bfloat16, device=gpu)
    y = torch.full((32,), 7.0, dtype=torch.bfloat16, device=gpu)
    st = torch.cuda.current_stream().cuda_stream

    def call(qp, sp, K, epi=STORE, N=32):
        return L.aha_hip_gemv_mxfp4(qp, sp, x.data_ptr(), y.data_ptr(), N, K, epi, None, C.c_float(1e-6), None, None, None, st)

    for args, msg in (((q.data_ptr(), words.data_ptr(), 40), "K must be a positive multiple of 32"),
                      ((q.data_ptr(), words.data_ptr(), 32800), "K must be at most 32768"),
                      ((q.data_ptr(), None, 64), "null scales"),
                      ((None, words.data_ptr(), 64), "null matrix or x"),
                      ((q.data_ptr(), words.data_ptr(), 64, RESIDUAL), "epi 1 needs a residual"),
                      ((q.data_ptr(), words.data_ptr(), 64, SILU_MUL, 48), "epi 2 needs N % 32 == 0"),
                      ((q.data_ptr(), words.data_ptr(), 64, LOGITS), "epi 3 needs logits and argmax_out"),
                      ((q.data_ptr(), words.data_ptr(), 64, 4), "epi must be 0..3")):
        with pytest.raises(AhaHipError) as e:
            _lib.check(call(*args))
        assert e.value.code == -1 and "gemv_mxfp4: " in str(e.value) and msg in str(e.value)
    torch.cuda.synchronize()
    assert bool((y.float() == 7.0).all())        # nothing was launched
    # and the same arguments made good run: zero codes give zeros
    out = ops.gemv_mxfp4(q, torch.full((32, 2), 127, dtype=torch.uint8), x)
    assert out.shape == (32,) and bool((out.float() == 0).all())
