"""-m gpu: the single-sequence matvec from exact 13-bit weight copies (gemv_kernel_pk13) is the bf16 matvec on the same W, bit for bit.

  1. the device pack and check equal aha_amd/quant.py byte for byte;
  2. ops.gemv_pk13(pack(W), x, ...) == ops.gemv_epi(W, x, ...) on every output bit (and the argmax) for every shipped instantiation --
     epilogues STORE / RESIDUAL / SILU_MUL / LOGITS, K = 4096 and 12288, with and without norm weights (which between them select the
     three prologue forms), and per epilogue the row counts 8 (fewer tiles than blocks), 4 R + 1 (clamped rows) and 3080 (R = 1) / 6160
     (R = 2): more tiles than the 768 blocks, ragged last round.  The fused gate / up layout comes in whole 32-row blocks (the entries
     refuse anything else), so SILU_MUL takes the nearest output-row counts 16, 32 and 3088.  The weights hold +-0, bf16 subnormals, E = 1
     and both edges of the window.  The two kernels' plans differ in R, U and grid, so this also shows that a row's bits depend on neither;
  3. a model the plan takes (two layers, hidden 4096, intermediate 4096, vocabulary 4096) decodes the same tokens and logit bits with the
     switch at 0 and at its default; one out-of-window weight leaves that matrix unpacked and the output as it was; quantize_weights
     frees the copies, and the quantised model equals one created without copies and quantised the same way.
"""
import os
import sys

import numpy as np
import pytest
import torch

from aha_amd.configs import tiny_qwen3
from aha_amd.weights import qwen3_text_weights

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_weights_fp8_cpu import bf16_bits  # noqa: E402
from test_weights_fp8_gpu import bits, prompts  # noqa: E402
from test_wpack_cpu import LOGITS, RESIDUAL, SILU_MUL, STORE, edge_weights, shipped  # noqa: E402

pytestmark = pytest.mark.gpu

TOP, BH = 63, 48          # the planted maximum has E >> 1 = 63: the window's codes are E >> 1 = 49 .. 63


def rows_of(epi):
    """Output rows per case: fewer tiles than blocks, clamped rows, more tiles than 768 blocks with a ragged last round."""
    return (16, 32, 3088) if epi == SILU_MUL else (8, 9, 6160) if epi == LOGITS else (8, 5, 3080)


# ---- 1. the pack kernel ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,K", [(64, 4096), (48, 12288)])
def test_device_pack_equals_the_python_restatement_byte_for_byte(gpu, N, K):
    from aha_amd import ops, quant
    W = edge_weights(N, K, seed=N)
    bh, bad = quant.check_pk13(W)
    P, gbh, gbad = ops.pack_pk13(W.to(gpu))
    assert (gbh, gbad) == (bh, bad) == (bh, 0)
    assert P.shape == (N, K // 4096, 6656) and torch.equal(P.cpu(), quant.pack_pk13(W, bh))
    # a matrix the format cannot hold: the same count on both sides, nothing packed
    Wb = W.clone()
    Wb[1, 7] = float("inf")
    Wb[2, 4000] = float("nan")
    Wb[3, K - 1] = 1e-30          # finite, far below the window
    P2, gbh2, gbad2 = ops.pack_pk13(Wb.to(gpu))
    assert P2 is None and (gbh2, gbad2) == quant.check_pk13(Wb) == (bh, 3)


# ---- 2. the matvec --------------------------------------------------------------------------------------------------------------------
_W = {}


def big_matrix(gpu, K):
    """(6176, K) normal(0, 0.02) bf16 on the GPU with the format's special values planted in every row: every case reads its first rows."""
    if K not in _W:
        g = torch.Generator(device=gpu).manual_seed(500 + K)
        W = torch.randn(6176, K, generator=g, device=gpu) * 0.02
        W = torch.where(W.abs() < 2.0 ** -24, torch.zeros_like(W), W).bfloat16()          # the random part stays inside the window, with zeros
        b = W.view(torch.int16)
        plant = {3: 0x8000, 5: 0x0000, 64: 0x0001, 65: 0x807f, 700: 0x0080, 1031: 0x80ff,           # +-0, subnormals, E = 1
                 8: (TOP << 8) | 0x80, 519: 0x8000 | (TOP << 8) | 0xff, 1500: (TOP << 8) | 0x00,        # the top code, both E
                 2048: ((BH + 1) << 8) | 0x00, 4095: 0x8000 | ((BH + 1) << 8) | 0xff, K - 9: ((BH + 1) << 8) | 0x80,      # the lowest code
                 K - 1: 0x8000, K - 512: (TOP << 8) | 0x7f}
        for col, v in plant.items():
            b[:, col] = v - 0x10000 if v >= 0x8000 else v
        _W.clear()          # one K resident at a time
        x = torch.randn(K, generator=g, device=gpu).bfloat16()
        res = torch.randn(6176, generator=g, device=gpu).bfloat16()
        nw = (1.0 + 0.1 * torch.randn(K, generator=g, device=gpu)).bfloat16()
        _W[K] = (W, x, res, nw)
    return _W[K]


def test_the_cases_select_every_shipped_instantiation(hip_lib):
    from aha_amd import ops
    hit = set()
    for epi in (STORE, RESIDUAL, SILU_MUL, LOGITS):
        for K in (4096, 12288):
            for norm in (False, True):
                for n in rows_of(epi):
                    r, u, grid, form = ops.plan_gemv_pk13(2 * n if epi == SILU_MUL else n, K, epi, norm)
                    hit.add((r, epi, form - 1))
                r = 2 if epi == LOGITS else 1
                n = rows_of(epi)
                assert ops.plan_gemv_pk13(2 * n[0] if epi == SILU_MUL else n[0], K, epi, norm)[2] == -(-n[0] // (4 * r)) < 768
                assert n[1] % (4 * r) or epi == SILU_MUL
                assert ops.plan_gemv_pk13(2 * n[2] if epi == SILU_MUL else n[2], K, epi, norm)[2] == 768 and -(-n[2] // (4 * r)) % 768
    assert hit == shipped()


@pytest.mark.parametrize("K", [4096, 12288])
@pytest.mark.parametrize("epi", [STORE, RESIDUAL, SILU_MUL, LOGITS])
def test_packed_matvec_is_bit_identical_to_the_bf16_matvec(gpu, epi, K):
    from aha_amd import ops
    Wall, x, res_all, nw = big_matrix(gpu, K)
    for n_out in rows_of(epi):
        N = 2 * n_out if epi == SILU_MUL else n_out          # matrix rows
        W = Wall[:N].contiguous()
        P, bh, bad = ops.pack_pk13(W)
        assert bad == 0 and bh == BH
        res = res_all[:n_out].contiguous()
        for norm in (False, True):
            kw = dict(norm_w=nw if norm else None, eps=1e-6, residual=res if epi == RESIDUAL else None)
            got = ops.gemv_pk13(P, bh, x, epi, **kw)
            want = ops.gemv_epi(W, x, epi, **kw)
            if epi == LOGITS:
                assert got[0].shape == (N,) and torch.equal(got[0].view(torch.int32), want[0].view(torch.int32)), (n_out, norm)
                assert got[1] == want[1] == int(torch.argmax(want[0])), (n_out, norm)          # the first maximal index
                got = got[0]
            else:
                assert got.shape == (n_out,) and torch.equal(bf16_bits(got), bf16_bits(want)), (n_out, norm)
            assert bool(torch.isfinite(got.float()).all()) and bool((got.float() != 0).any()), (n_out, norm)
            if epi == RESIDUAL:      # the output aliasing the residual
                ya, yb = res.clone(), res.clone()
                ops.gemv_pk13(P, bh, x, epi, norm_w=kw["norm_w"], residual=ya, out=ya)
                ops.gemv_epi(W, x, epi, norm_w=kw["norm_w"], residual=yb, out=yb)
                assert torch.equal(bf16_bits(ya), bf16_bits(yb)) and torch.equal(bf16_bits(ya), bf16_bits(got)), (n_out, norm)


# ---- 3. the model ---------------------------------------------------------------------------------------------------------------------
_MODEL = {}


def model_weights():
    if not _MODEL:
        cfg = tiny_qwen3(layers=2, hidden=4096, heads=32, kv_heads=8, inter=4096, vocab=4096, tie=False)
        _MODEL["cfg"], _MODEL["w"] = cfg, qwen3_text_weights(cfg, seed=71)
    return _MODEL["cfg"], _MODEL["w"]


def greedy(m, ids, new=12):
    m.clear_cache()
    _, tok = m.forward_initial(ids, 0)
    m.set_profiling(True)
    toks = m.decode_greedy(tok, len(ids), new)
    prof = m.get_profile("gemv")
    m.set_profiling(False)
    return [tok] + toks, bits(m.last_logits().copy()), prof


def test_model_decodes_the_same_bits_from_the_copies(gpu):
    from aha_amd import ops
    from aha_amd.model import HipInferenceModel
    cfg, w = model_weights()
    # by plan the step reads gate+up from its copy (2^25 elements); the switch at 2 adds qkv, o_proj, down_proj and lm_head
    assert [ops.gemv_pk13_by_plan(n, k, e) for n, k, e in ((6144, 4096, STORE), (4096, 4096, RESIDUAL), (8192, 4096, SILU_MUL),
                                                            (4096, 4096, LOGITS))] == [False, False, True, False]
    m = HipInferenceModel(cfg, w)
    try:
        st = m.pk13_status()
        assert len(st) == 4 * 2 + 1 and set(st.values()) == {"packed"}, st
        ids = prompts(21, (19,), vocab=4096)[0]
        td, ld, pd = greedy(m, ids)
        m.debug_pk13_single(0)
        t0, l0, p0 = greedy(m, ids)
        m.debug_pk13_single(2)
        t2, l2, p2 = greedy(m, ids)
        assert td == t0 == t2 and len(td) == 13 and len(set(td)) > 3
        assert np.array_equal(ld, l0) and np.array_equal(ld, l2)
        # the same launches in the same class, with the bytes each kernel reads
        assert pd["launches"] == p0["launches"] == p2["launches"] > 0 and p2["bytes"] < 0.85 * p0["bytes"] and p2["bytes"] < pd["bytes"] < p0["bytes"]
        # the launch-per-step path, whose argmax launch reduces the packed lm_head's own partial count
        m.debug_pk13_single(1)
        m.clear_cache()
        _, tok = m.forward_initial(ids, 0)
        for i in range(3):
            lg, tok = m.forward_step(tok, len(ids) + i)
            assert tok == td[i + 1] == int(np.argmax(lg))
    finally:
        m.close()


def test_one_out_of_window_weight_leaves_its_matrix_unpacked_and_the_output_unchanged(gpu):
    from aha_amd.model import HipInferenceModel
    cfg, w = model_weights()
    name = "model.layers.1.mlp.down_proj.weight"
    wn = dict(w)
    wn[name] = w[name].clone()
    wn[name][77, 1234] = 1e-30
    m = HipInferenceModel(cfg, wn)
    try:
        st = m.pk13_status()
        why = st.pop("layers.1.mlp.down_proj.weight")
        assert why.startswith("1 weights outside the window") and set(st.values()) == {"packed"}, (why, st)
        ids = prompts(22, (17,), vocab=4096)[0]
        td, ld, _ = greedy(m, ids)
        m.debug_pk13_single(0)
        t0, l0, _ = greedy(m, ids)
        assert td == t0 and np.array_equal(ld, l0)
    finally:
        m.close()


def test_quantize_weights_frees_the_copies(gpu):
    from aha_amd.model import HipInferenceModel
    cfg, w = model_weights()
    ids = prompts(23, (18,), vocab=4096)[0]
    a = HipInferenceModel(cfg, w)
    try:
        assert set(a.pk13_status().values()) == {"packed"}
        a.quantize_weights("mxfp8", lm_head=True)
        assert set(a.pk13_status().values()) == {"freed by quantize_weights"}
        ta, la, _ = greedy(a, ids)
        a.debug_pk13_single(2)          # nothing left to read
        t2, l2, _ = greedy(a, ids)
        assert ta == t2 and np.array_equal(la, l2)
    finally:
        a.close()
    old = os.environ.get("AHA_WPACK")
    os.environ["AHA_WPACK"] = "0"
    try:
        b = HipInferenceModel(cfg, w)
    finally:
        if old is None:
            del os.environ["AHA_WPACK"]
        else:
            os.environ["AHA_WPACK"] = old
    try:
        assert set(b.pk13_status().values()) == {"off (AHA_WPACK=0)"}
        b.quantize_weights("mxfp8", lm_head=True)
        tb, lb, _ = greedy(b, ids)
        assert ta == tb and np.array_equal(la, lb)
    finally:
        b.close()
