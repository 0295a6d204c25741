"""-m gpu: single-sequence decode from MXFP8 weights (gemv_mxfp8_kernel) is the bf16 matvec on the dequantised weights, bit for bit.

  1. ops.gemv_mxfp8(q, s, x, ...) == ops.gemv_epi(W', x, ...) on every output bit (and the argmax) for (q, s, W') of the reference
     quantiser, every epilogue, with and without norm weights, over shapes that between them select EVERY instantiation the library ships
     (asserted through the plan query) -- the two kernels' plans differ in R, U and grid, so this is also the proof that a row's bits do
     not depend on them;
  2. a model quantised in place equals a model created from the reference's W' through forward_initial + forward_step, decode_greedy and
     a seeded generate_generic loop, while its profile shows gemv_fp8 launches (4 per layer and step, plus the head with lm_head);
  3. aha_hip_gemv_mxfp8 refuses bad arguments before anything is launched.
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
from test_weights_fp8_cpu import bf16_bits  # noqa: E402
from test_weights_fp8_gpu import bits, prompts, reference_weights  # noqa: E402
from test_weights_fp8_single_cpu import shipped  # noqa: E402

pytestmark = pytest.mark.gpu

STORE, RESIDUAL, SILU_MUL, LOGITS = 0, 1, 2, 3

# (N, K).  The first eight are the smallest shapes that reach each branch of the kernel; the rest complete the cover of the shipped
# instantiations: rows per wave R by N (1 below 4089 output rows, 2 up to 8176, then 4; gate+up: 1 / 2 over N / 2), chunks per item U by K
# (512 * U: FAST and straight-line; + 32: the general form with a partial last chunk), and K past the straight-line limit (8192 with norm
# weights, 16384 without) for the FAST form with the general prologue.
SHAPES = [(40, 160),        # one partial chunk, ragged last tile, fewer tiles than any grid
          (4100, 1024),     # two rows per wave, 513 tiles
          (8224, 512),      # four rows per wave (gate+up: two), one chunk
          (16416, 256),     # the lm_head-style plan: 1026 tiles on 768 blocks, a block walks two tiles; half a chunk
          (64, 4096),       # straight-line, U = 8
          (64, 12288),      # without norm: straight-line past 8192; with: FAST, general prologue
          (32, 16896),      # 33 chunks: past the straight-line limit, the last group of 8 holds one chunk
          (64, 1056),       # general form, whole chunks plus a partial last chunk
          (64, 160), (64, 512), (64, 1024), (64, 2048), (64, 2080), (64, 4128), (32, 20480),
          (4100, 160), (4100, 512), (4100, 1056), (4100, 2048), (4100, 2080), (4100, 4096), (4100, 4128), (4100, 12288),
          (8224, 256), (8224, 1024), (8224, 1056), (8224, 2048), (8224, 2080), (8224, 10240),
          (100000, 64),     # 6250 tiles on 768 blocks: the persistent walk, uneven (some blocks 9 tiles, some 8); the general form
          # the FAST forms with more tiles than blocks -- what the large decode matrices run (8B gate+up: 1536 tiles on 768 blocks, the
          # lm_head 9496): a tile change between issue and consume, the accumulator reset and the residual buffers at a tile boundary, the
          # argmax carried over a block's tiles
          (16416, 512), (16416, 1024), (16416, 2048),   # 1026 tiles on 768 blocks, R = 4 (gate+up: R = 2), one chunk group per tile
          (16416, 4096),    # the same with two chunk groups per tile (gate+up: U = 4, two as well)
          (6400, 4096)]     # R = 2, U = 8 (the 8B qkv / o_proj / down instantiations): 800 tiles on 768 blocks
MULTI_TILE_FAST = [(16416, 512), (16416, 1024), (16416, 2048), (16416, 4096), (6400, 4096)]


def cases_of(N, K):
    for epi in (STORE, RESIDUAL, SILU_MUL, LOGITS):
        if epi == SILU_MUL and N % 32:
            continue   # the gate / up block layout needs whole 32-row blocks (the entries refuse it)
        for norm in (False, True):
            yield epi, norm


def test_the_shapes_select_every_shipped_instantiation(hip_lib):
    from aha_amd import ops
    hit = set()
    for N, K in SHAPES:
        for epi, norm in cases_of(N, K):
            r, u, grid, form = ops.plan_gemv_mxfp8(N, K, epi, norm)
            hit.add((r, u, epi, int(form != 0), max(form - 1, 0)))
    assert hit == shipped(), (sorted(shipped() - hit), sorted(hit - shipped()))
    # the FAST forms walk several tiles per block, for every epilogue, with and without norm weights
    for N, K in MULTI_TILE_FAST:
        for epi, norm in cases_of(N, K):
            r, u, grid, form = ops.plan_gemv_mxfp8(N, K, epi, norm)
            rows = N // 2 if epi == SILU_MUL else N
            assert -(-rows // (4 * r)) > grid and form != 0, (N, K, epi, norm, r, u, grid, form)
    assert ops.plan_gemv_mxfp8(16416, 4096, STORE, True)[:2] == (4, 4) and ops.plan_gemv_mxfp8(6400, 4096, RESIDUAL, False)[:2] == (2, 8)
    # and the general form does
    assert ops.plan_gemv_mxfp8(16416, 256, LOGITS, False)[:3] == (4, 1, 768) and ops.plan_gemv_mxfp8(100000, 64, STORE, False)[2] == 768


_CASES = {}


def kernel_case(gpu, N, K):
    """The reference's (q, scales, W') of a seeded W on the GPU, x, a residual and norm weights; built once per shape."""
    if (N, K) not in _CASES:
        from aha_amd import quant
        g = torch.Generator().manual_seed(1000 + N + K)
        # per-block magnitudes spread over 2^-6 .. 2^2 so that the scales differ from block to block
        W = (torch.randn(N, K, generator=g) * torch.exp2(torch.randint(-6, 3, (N, K // 32, 1), generator=g).float()).expand(N, K // 32, 32)
             .reshape(N, K) * 0.05).bfloat16()
        q, s, wr = quant.quantize_mxfp8(W)
        x = torch.randn(K, generator=g).bfloat16()
        res = torch.randn(N, generator=g).bfloat16()
        nw = (1.0 + 0.1 * torch.randn(K, generator=g)).bfloat16()
        _CASES.clear()       # one shape resident at a time
        _CASES[(N, K)] = tuple(t.to(gpu) for t in (q, s, wr, x, res, nw))
    return _CASES[(N, K)]


@pytest.mark.parametrize("N,K", SHAPES)
def test_fp8_matvec_is_bit_identical_to_bf16_matvec_on_dequantised_weights(gpu, N, K):
    from aha_amd import ops
    q, s, wr, x, res, nw = kernel_case(gpu, N, K)
    for epi, norm in cases_of(N, K):
        kw = dict(norm_w=nw if norm else None, eps=1e-6, residual=res if epi == RESIDUAL else None)
        got = ops.gemv_mxfp8(q, s, x, epi, **kw)
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
            ops.gemv_mxfp8(q, s, x, epi, norm_w=kw["norm_w"], residual=ya, out=ya)
            ops.gemv_epi(wr, x, epi, norm_w=kw["norm_w"], residual=yb, out=yb)
            assert torch.equal(bf16_bits(ya), bf16_bits(yb)) and torch.equal(bf16_bits(ya), bf16_bits(got)), norm


# ---- 2. the model ----------------------------------------------------------------------------------------------------------------
def classes(m):
    return {c: m.get_profile(c)["launches"] for c in ("gemv", "gemv_fp8")}


def profiled_decode(m, first, offset, new):
    """decode_greedy under a fresh profile: (tokens, {class: launches})."""
    m.set_profiling(True)
    toks = m.decode_greedy(first, offset, new)
    prof = classes(m)
    m.set_profiling(False)
    return toks, prof


# hidden 256 / inter 512: every matvec in the general or a short straight-line form; hidden 1024 / inter 2048: U = 2 and 4 straight-line
@pytest.mark.parametrize("hidden,heads,inter", [(256, 4, 512), (1024, 8, 2048)])
@pytest.mark.parametrize("tie,lm_head", [(True, False), (True, True), (False, False), (False, True)])
def test_quantised_model_decodes_single_sequences_as_the_model_created_from_dequantised_weights(gpu, hidden, heads, inter, tie, lm_head):
    from aha_amd import sampling as hs
    from aha_amd.model import HipInferenceModel
    cfg = tiny_qwen3(layers=2, hidden=hidden, heads=heads, kv_heads=2, inter=inter, vocab=1024, tie=tie)
    w = qwen3_text_weights(cfg, seed=41)
    A = HipInferenceModel(cfg, w)
    B = HipInferenceModel(cfg, reference_weights(w, tie, lm_head))
    try:
        A.quantize_weights("mxfp8", lm_head=lm_head)
        # by default the plan keeps matrices this small on the bf16 kernel (ops.gemv_mxfp8_by_plan): 2 = every matrix with a copy
        A.debug_fp8_single(2)
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

        def greedy(m):
            m.clear_cache()
            _, tok = m.forward_initial(ids, 0)
            toks, prof = profiled_decode(m, tok, len(ids), 24)
            return [tok] + toks, prof, m.last_logits().copy()

        ga, pa, lga = greedy(A)
        gb, pb, lgb = greedy(B)
        assert ga == gb and len(ga) == 25 and np.array_equal(bits(lga), bits(lgb))
        # B: no FP8 launch; 4 matvecs per layer and step plus one head per step.  A: the layer matvecs (and the head with lm_head) as gemv_fp8.
        n_steps = pb["gemv"] // (4 * L + 1)
        assert pb == {"gemv": n_steps * (4 * L + 1), "gemv_fp8": 0} and n_steps >= 24, pb
        assert pa == ({"gemv": 0, "gemv_fp8": n_steps * (4 * L + 1)} if lm_head else {"gemv": n_steps, "gemv_fp8": n_steps * 4 * L}), (pa, pb)

        def sampled(m):
            m.clear_cache()
            ctx = hs.GenerationContext(0.8, 0.9, 20, 1.1, 64, seed=17, initial_seq_len=len(ids), max_tokens=12)
            toks = hs.generate_generic_sampled(m, ids, ctx)
            return toks, m.last_logits().copy()

        sa, lsa = sampled(A)
        sb, lsb = sampled(B)
        assert sa == sb and len(sa) == 12 and np.array_equal(bits(lsa), bits(lsb))
        # the switch: the bf16 kernel on W' -- B's classes, the same bits
        A.debug_fp8_single(False)
        go, po, lgo = greedy(A)
        assert po == pb and go == ga and np.array_equal(bits(lgo), bits(lga))
        A.debug_fp8_single(2)
        assert greedy(A)[1] == pa
        # the default: by plan, and the plan takes none of these shapes -- bf16 launches, the same bits again
        from aha_amd import ops
        assert not any(ops.gemv_mxfp8_by_plan(n, k, e) for n, k, e in ((hidden + 4 * 128, hidden, STORE), (hidden, heads * 128, RESIDUAL),
                                                                        (2 * inter, hidden, SILU_MUL), (hidden, inter, RESIDUAL), (1024, hidden, LOGITS)))
        A.debug_fp8_single(True)
        gd, pd, lgd = greedy(A)
        assert pd == pb and gd == ga and np.array_equal(bits(lgd), bits(lga))
    finally:
        A.close()
        B.close()


def greedy_run(m, ids, new):
    m.clear_cache()
    _, tok = m.forward_initial(ids, 0)
    toks, prof = profiled_decode(m, tok, len(ids), new)
    return [tok] + toks, prof, m.last_logits().copy()


def test_argmax_partials_follow_the_grid_of_the_kernel_that_ran(gpu):
    """Vocabulary 10000: the FP8 lm_head writes 625 (max, index) partials, the bf16 one 768.  The device-resident loop's fused tail and the
    argmax launch of forward_step must reduce the count of the kernel that ran: a bf16 pass first leaves 768 real partials of other
    steps behind, which a reduction over the wrong count would pick up."""
    from aha_amd import ops
    from aha_amd.model import HipInferenceModel
    assert ops.plan_gemv_mxfp8(10000, 256, LOGITS, True)[2] == 625
    cfg = tiny_qwen3(layers=2, hidden=256, heads=4, kv_heads=2, inter=512, vocab=10000, tie=False)
    w = qwen3_text_weights(cfg, seed=43)
    A = HipInferenceModel(cfg, w)
    B = HipInferenceModel(cfg, reference_weights(w, False, True))
    try:
        A.quantize_weights("mxfp8", lm_head=True)
        ids = prompts(14, (29,))[0]
        gb, pb, lgb = greedy_run(B, ids, 24)
        assert len(set(gb)) > 4      # the tokens move: a stale partial would not go unnoticed
        for mode in (0, 2, 0, 2):
            A.debug_fp8_single(mode)
            ga, pa, lga = greedy_run(A, ids, 24)
            assert ga == gb and np.array_equal(bits(lga), bits(lgb)), mode
            assert (pa["gemv_fp8"] > 0) == (mode == 2)
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


def test_default_switch_sends_a_large_fast_lm_head_to_the_fp8_kernel(gpu):
    """The default (by plan) in a model: an lm_head of 16416 x 1024 = 2^24 + elements in the FAST form is read from its copy -- 1026 tiles on
    768 blocks, the multi-tile LOGITS walk -- while the small layer matrices stay on bf16; the same tokens and logit bits either way."""
    from aha_amd import ops
    from aha_amd.model import HipInferenceModel
    assert ops.gemv_mxfp8_by_plan(16416, 1024, LOGITS) and ops.plan_gemv_mxfp8(16416, 1024, LOGITS, True) == (4, 2, 768, 3)
    assert not ops.gemv_mxfp8_by_plan(16416, 1056, LOGITS)       # as large, but the general form: kept on bf16
    cfg = tiny_qwen3(layers=2, hidden=1024, heads=8, kv_heads=2, inter=2048, vocab=16416, tie=False)
    w = qwen3_text_weights(cfg, seed=44)
    A = HipInferenceModel(cfg, w)
    B = HipInferenceModel(cfg, reference_weights(w, False, True))
    try:
        A.quantize_weights("mxfp8", lm_head=True)
        L = cfg.num_hidden_layers
        ids = prompts(15, (33,))[0]
        gb, pb, lgb = greedy_run(B, ids, 16)
        ga, pa, lga = greedy_run(A, ids, 16)
        assert ga == gb and np.array_equal(bits(lga), bits(lgb))
        n_steps = pb["gemv"] // (4 * L + 1)
        assert pb["gemv_fp8"] == 0 and pa == {"gemv": n_steps * 4 * L, "gemv_fp8": n_steps}, (pa, pb)
    finally:
        A.close()
        B.close()


def test_models_without_copies_never_launch_the_fp8_matvec(gpu):
    from aha_amd.model import HipInferenceModel
    cfg = tiny_qwen3(layers=2, hidden=256, heads=4, kv_heads=2, inter=512, vocab=1024)
    w = qwen3_text_weights(cfg, seed=42)
    wn = {k: v.clone() for k, v in w.items()}
    wn["model.layers.1.mlp.down_proj.weight"][5, 77] = float("nan")
    plain, refused = HipInferenceModel(cfg, w), HipInferenceModel(cfg, wn)
    try:
        with pytest.raises(AhaHipError):
            refused.quantize_weights("mxfp8", lm_head=True)
        ids = prompts(13, (20,))[0]
        L = cfg.num_hidden_layers
        for m in (plain, refused):
            m.forward_initial(ids, 0)
            m.set_profiling(True)
            m.forward_step(7, len(ids))       # a fixed token: the refused model's logits are NaN
            assert classes(m) == {"gemv": 4 * L + 1, "gemv_fp8": 0}
            m.set_profiling(False)
        toks, prof = profiled_decode(plain, 7, len(ids) + 1, 4)
        assert prof["gemv_fp8"] == 0 and prof["gemv"] >= 4 * (4 * L + 1) and len(toks) == 4, prof
    finally:
        plain.close()
        refused.close()


# ---- 3. errors -------------------------------------------------------------------------------------------------------------------
def test_gemv_mxfp8_refuses_bad_arguments_before_any_launch(gpu):
    from aha_amd import _lib, ops
    L = _lib.lib()
    q = torch.zeros(32, 64, dtype=torch.uint8, device=gpu)
    words = torch.full((32, 1), 0x7f7f7f7f, dtype=torch.int32, device=gpu)
    x = torch.ones(64, dtype=torch.bfloat16, device=gpu)
    y = torch.full((32,), 7.0, dtype=torch.bfloat16, device=gpu)
    st = torch.cuda.current_stream().cuda_stream

    def call(qp, sp, K):
        return L.aha_hip_gemv_mxfp8(qp, sp, x.data_ptr(), y.data_ptr(), 32, K, STORE, None, C.c_float(1e-6), None, None, None, st)

    for args, msg in (((q.data_ptr(), words.data_ptr(), 40), "K must be a positive multiple of 32"),
                      ((q.data_ptr(), words.data_ptr(), 32800), "K must be at most 32768"),
                      ((q.data_ptr(), None, 64), "null scales")):
        with pytest.raises(AhaHipError) as e:
            _lib.check(call(*args))
        assert e.value.code == -1 and "gemv_mxfp8" in str(e.value) and msg in str(e.value)
    torch.cuda.synchronize()
    assert bool((y.float() == 7.0).all())        # nothing was launched
    # and the same arguments made good run: zero codes give zeros
    out = ops.gemv_mxfp8(q, torch.full((32, 2), 127, dtype=torch.uint8), x)
    assert bool((out.float() == 0).all())
