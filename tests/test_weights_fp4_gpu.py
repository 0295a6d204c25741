"""-m gpu: MXFP4 weight copies (aha_hip_model_quantize_weights with "mxfp4") end to end.

As with MXFP8, everything is bit-checkable: W' = dequantised W is exact in bf16, the FP4 matvec converts its nibbles to exactly the bf16
operands the bf16 matvec loads from W' (-0.0 for the code 0x8 included) and accumulates in the same order.  So
  * the library's quantiser equals the reference quantiser (aha_amd/quant.py) byte for byte;
  * gemv_rows_mxfp4(q, scales, x) equals gemv_rows(W', x) bit for bit, on every epilogue, row count and plan branch of gemv_rows_plan;
  * a model quantised in place equals, token for token and logit bit for logit bit, a model created from the reference's W' with nothing
    quantised -- through generate_batch, generate_batch_sampled, generate_batch_spec, the engine and forward_step -- while the profile
    shows that its batched decode steps ran the FP4 kernel and its single-sequence steps never read the copies.
"""
import os
import sys

import numpy as np
import pytest
import torch

from aha_amd._lib import AhaHipError
from aha_amd.configs import tiny_qwen3
from aha_amd.sampling import SamplingParams
from aha_amd.weights import qwen3_text_weights

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_weights_fp4_cpu import TIES, bf16_bits, edge_matrix  # noqa: E402

pytestmark = pytest.mark.gpu

STORE, RESIDUAL, SILU_MUL, LOGITS = 0, 1, 2, 3
QUANTISED = ("q_proj", "k_proj", "v_proj", "o_proj", "gate_proj", "up_proj", "down_proj")


def bits(x):
    return np.asarray(x, dtype=np.float32).view(np.uint32)


# ---- 1. the quantiser ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["edge", "random"])
def test_quantiser_equals_reference_byte_for_byte(gpu, which):
    from aha_amd import ops, quant
    W = edge_matrix() if which == "edge" else (torch.randn(256, 1024, generator=torch.Generator().manual_seed(3)) * 0.02).bfloat16()
    q, s, wr = quant.quantize_mxfp4(W)
    gq, gs, gwr = ops.quantize_mxfp4(W.to(gpu))
    assert gq.dtype == torch.uint8 and gs.dtype == torch.uint8 and gwr.dtype == torch.bfloat16
    assert gq.shape == (W.shape[0], W.shape[1] // 2)
    assert torch.equal(gs.cpu(), s)
    assert torch.equal(gq.cpu(), q)
    assert torch.equal(bf16_bits(gwr.cpu()), bf16_bits(wr))


# ---- 2. the kernel ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def kernel_cases(gpu):
    """Per (N, K): the reference's (q, scales, W') of a seeded W on the GPU, and 32 rows of x / residual."""
    from aha_amd import quant
    out = {}
    for i, (N, K) in enumerate(((40, 160), (96, 1024), (8192, 1024), (4096, 2048))):
        g = torch.Generator().manual_seed(200 + i)
        # per-block magnitudes spread over 2^-6 .. 2^2 so that the scales differ from block to block
        W = (torch.randn(N, K, generator=g) * torch.exp2(torch.randint(-6, 3, (N, K // 32, 1), generator=g).float()).expand(N, K // 32, 32)
             .reshape(N, K) * 0.05).bfloat16()
        # a block of planted ties of both signs under an amax of 6 * 2^-5 (the random part holds ties and -0 codes of its own)
        W[1, 32:64] = 0.0
        W[1, 32] = 6.0 * 2.0 ** -5
        for j, (v, _) in enumerate(TIES):
            W[1, 33 + 2 * j], W[1, 34 + 2 * j] = v * 2.0 ** -5, -v * 2.0 ** -5
        q, s, wr = quant.quantize_mxfp4(W)
        # the case really holds what the kernel must get right: -0 codes, and weights half way between two codes
        codes = quant.unpack_nibbles(q)
        v = W.double().abs() / torch.exp2((s.to(torch.int32) - 127).double()).repeat_interleave(32, dim=1)
        n_ties = int(torch.isin(v, torch.tensor([t for t, _ in TIES], dtype=torch.float64)).sum())
        assert int((codes == 8).sum()) > 0 and n_ties >= 2 * len(TIES), (N, K, n_ties)
        assert len(torch.unique(s)) >= 5                                       # neighbouring scales differ
        x = torch.randn(32, K, generator=g).bfloat16()
        res = torch.randn(32, N, generator=g).bfloat16()
        out[(N, K)] = (q.to(gpu), s.to(gpu), wr.to(gpu), x.to(gpu), res.to(gpu))
    return out


@pytest.mark.parametrize("N,K", [(40, 160), (96, 1024), (8192, 1024), (4096, 2048)])
def test_fp4_matvec_is_bit_identical_to_bf16_matvec_on_dequantised_weights(gpu, kernel_cases, N, K):
    from aha_amd import ops
    q, s, wr, x, res = kernel_cases[(N, K)]
    assert int((bf16_bits(wr) == -32768).sum()) > 0                            # W' holds -0.0 where the copy holds 0x8
    first = {}
    for R in (1, 16, 17, 32):
        xs, rs = x[:R].contiguous(), res[:R].contiguous()
        for epi in (STORE, RESIDUAL, SILU_MUL, LOGITS):
            if epi == SILU_MUL and N % 32:
                continue   # the gate / up block layout needs whole 32-row blocks (aha_hip_gemv_rows refuses it too)
            r = rs if epi == RESIDUAL else None
            got = ops.gemv_rows_mxfp4(q, s, xs, epi, r)
            want = ops.gemv_rows(wr, xs, epi, r)
            if epi == LOGITS:
                assert torch.equal(got[0].view(torch.int32), want[0].view(torch.int32)), (R, epi)
                assert torch.equal(got[1], want[1]), (R, epi)
                got = got[0]
            else:
                assert torch.equal(bf16_bits(got), bf16_bits(want)), (R, epi)
            assert bool(torch.isfinite(got.float()).all())
            if R == 1:
                first[epi] = got.clone()
            elif R == 32:   # row isolation: row 0 of the 32-row call is the 1-row call
                a, b = got[0], first[epi][0]
                assert torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else bf16_bits(a),
                                   b.view(torch.int32) if b.dtype == torch.float32 else bf16_bits(b)), epi


# ---- 3. the model ----------------------------------------------------------------------------------------------------------------
def reference_weights(w, tie, lm_head):
    """The weights of model B: every matrix quantize_weights touches replaced by the reference quantiser's W'."""
    from aha_amd import quant
    out = {}
    for name, t in w.items():
        hit = any(name.endswith(f".{p}.weight") for p in QUANTISED)
        if lm_head and (name.endswith("lm_head.weight") or (tie and name.endswith("embed_tokens.weight"))):
            hit = True
        out[name] = quant.quantize_mxfp4(t)[2] if hit else t
    return out


def prompts(seed, lens, vocab=1024):
    g = np.random.default_rng(seed)
    return [[int(x) for x in g.integers(0, vocab, size=n)] for n in lens]


def engine_run(m, ps, max_new):
    from aha_amd.model import HipEngine
    eng = HipEngine(m, max_running=8, kv_pages=64)
    try:
        rid = {eng.submit(p, max_new): i for i, p in enumerate(ps)}
        toks, lgs = {i: [] for i in range(len(ps))}, {i: [] for i in range(len(ps))}
        for _ in range(4 * max_new + 8):
            evs, lg = eng.step(want_logits=True)
            for k, ev in enumerate(evs):
                toks[rid[ev.req_id]].append(ev.token)
                lgs[rid[ev.req_id]].append(lg[k].copy())
            st = eng.stats()
            if st["running"] == 0 and st["waiting"] == 0:
                break
        return toks, lgs
    finally:
        eng.close()


def decode_classes(m):
    return {c: m.get_profile(c)["launches"] for c in ("gemv_rows", "gemv_rows_fp8", "gemv_rows_fp4")}


def single_classes(m):
    return {c: m.get_profile(c)["launches"] for c in ("gemv", "gemv_fp8")}


@pytest.mark.parametrize("tie,lm_head", [(True, False), (True, True), (False, False), (False, True)])
def test_quantised_model_equals_model_created_from_dequantised_weights(gpu, tie, lm_head):
    from aha_amd.model import HipInferenceModel
    cfg = tiny_qwen3(layers=2, hidden=256, heads=4, kv_heads=2, inter=512, vocab=1024, tie=tie)
    w = qwen3_text_weights(cfg, seed=33)
    A = HipInferenceModel(cfg, w)
    B = HipInferenceModel(cfg, reference_weights(w, tie, lm_head))
    try:
        assert A.weight_format is None and B.weight_format is None
        A.quantize_weights("mxfp4", lm_head=lm_head)
        assert A.weight_format == ("mxfp4", lm_head)
        A.quantize_weights("mxfp4", lm_head=lm_head)    # the same arguments again: nothing happens
        ps, new = prompts(5, (3, 70, 17, 33, 64)), 24
        sp = [SamplingParams(0.8, 0.9, 20, repeat_penalty=1.1, seed=11 + j) for j in range(len(ps))]
        L = cfg.num_hidden_layers

        def runs(m):
            m.set_profiling(True)
            out = {"greedy": m.generate_batch(ps, new, want_logits=True)}
            prof = decode_classes(m)
            m.set_profiling(False)
            out["sampled"] = m.generate_batch_sampled(ps, sp, new, want_step_logits=True)
            out["spec"] = m.generate_batch_spec(ps, new, want_logits=True)
            out["engine"] = engine_run(m, ps, new)
            return out, prof

        ra, pa = runs(A)
        rb, pb = runs(B)
        for k in ("greedy", "sampled", "spec"):
            assert ra[k][0] == rb[k][0], k
            assert all(len(t) == new for t in ra[k][0]), k
            assert np.array_equal(bits(ra[k][1]), bits(rb[k][1])), k
        for i in range(len(ps)):
            assert ra["engine"][0][i] == rb["engine"][0][i] and len(ra["engine"][0][i]) == new, i
            assert np.array_equal(bits(np.stack(ra["engine"][1][i])), bits(np.stack(rb["engine"][1][i]))), i
        # the profile of the greedy run: A's layer matvecs (and its head with lm_head) ran the FP4 kernel and none the FP8 one, B's the
        # bf16 one.  The first tokens come from the prefill's head, so there are new - 1 decode steps of 4 matvecs per layer, plus the
        # head launches.
        layer_launches = 4 * L * (new - 1)
        assert pb["gemv_rows_fp4"] == 0 and pb["gemv_rows_fp8"] == 0 and pb["gemv_rows"] > layer_launches, pb
        heads = pb["gemv_rows"] - layer_launches
        if lm_head:
            assert pa == {"gemv_rows": 0, "gemv_rows_fp8": 0, "gemv_rows_fp4": layer_launches + heads}, (pa, pb)
        else:
            assert pa == {"gemv_rows": heads, "gemv_rows_fp8": 0, "gemv_rows_fp4": layer_launches}, (pa, pb)
        # the debug switch of the batched matvec holds for this format too: the bf16 kernel on W', the same bits
        A.debug_fp8_rows(False)
        A.set_profiling(True)
        off = A.generate_batch(ps, new, want_logits=True)
        assert decode_classes(A) == pb
        A.set_profiling(False)
        A.debug_fp8_rows(True)
        assert off[0] == ra["greedy"][0] and np.array_equal(bits(off[1]), bits(ra["greedy"][1]))
        # prefill + single-sequence decode read W' and never the FP4 bytes, whatever the single-sequence switch says
        B.clear_cache()
        lb0, tb = B.forward_initial(ps[1], 0)
        lb1, tb2 = B.forward_step(tb, len(ps[1]))
        for mode in (0, 1, 2):
            A.clear_cache()
            A.debug_fp8_single(mode)
            A.set_profiling(True)
            la0, ta = A.forward_initial(ps[1], 0)
            la1, ta2 = A.forward_step(ta, len(ps[1]))
            prof = single_classes(A)
            A.set_profiling(False)
            assert ta == tb and np.array_equal(bits(la0), bits(lb0)), mode
            assert ta2 == tb2 and np.array_equal(bits(la1), bits(lb1)), mode
            assert prof["gemv_fp8"] == 0 and prof["gemv"] >= 4 * L + 1, (mode, prof)
        A.debug_fp8_single(1)
    finally:
        A.close()
        B.close()


def test_33_sequences_cross_the_row_group_boundary(gpu):
    from aha_amd.model import HipInferenceModel
    cfg = tiny_qwen3(layers=2, hidden=256, heads=4, kv_heads=2, inter=512, vocab=1024, tie=True)
    w = qwen3_text_weights(cfg, seed=34)
    A = HipInferenceModel(cfg, w)
    B = HipInferenceModel(cfg, reference_weights(w, True, True))
    try:
        A.quantize_weights("mxfp4", lm_head=True)
        ps = prompts(6, [3 + (7 * j) % 40 for j in range(33)])
        ta, la = A.generate_batch(ps, 6, want_logits=True)
        tb, lb = B.generate_batch(ps, 6, want_logits=True)
        assert ta == tb and np.array_equal(bits(la), bits(lb))
    finally:
        A.close()
        B.close()


# ---- 4. errors -------------------------------------------------------------------------------------------------------------------
def test_quantize_weights_errors(gpu):
    from aha_amd.model import HipInferenceModel
    cfg = tiny_qwen3(layers=2, hidden=256, heads=4, kv_heads=2, inter=512, vocab=1024)
    w = qwen3_text_weights(cfg, seed=35)
    m8, m4 = HipInferenceModel(cfg, w), HipInferenceModel(cfg, w)
    try:
        m8.quantize_weights("mxfp8", lm_head=False)
        with pytest.raises(AhaHipError) as e:     # a model holds copies of one format
            m8.quantize_weights("mxfp4", lm_head=False)
        assert e.value.code == -7 and "already quantised with format 1, flags 0" in str(e.value)
        assert m8.weight_format == ("mxfp8", False)
        m4.quantize_weights("mxfp4", lm_head=True)
        with pytest.raises(AhaHipError) as e:
            m4.quantize_weights("mxfp8", lm_head=True)
        assert e.value.code == -7 and "already quantised with format 2, flags 1" in str(e.value)
        with pytest.raises(AhaHipError) as e:     # the same format with other flags
            m4.quantize_weights("mxfp4", lm_head=False)
        assert e.value.code == -7 and "already quantised with format 2, flags 1" in str(e.value)
        m4.quantize_weights("mxfp4", lm_head=True)    # the same arguments twice: a no-op
        assert m4.weight_format == ("mxfp4", True)
        with pytest.raises(ValueError):
            m4.quantize_weights("int4")
    finally:
        m8.close()
        m4.close()
    # a NaN weight: refused naming the tensor, before any matrix is modified -- the model still computes what an untouched one does
    wn = {k: v.clone() for k, v in w.items()}
    wn["model.layers.1.mlp.down_proj.weight"][5, 77] = float("nan")
    a, b = HipInferenceModel(cfg, wn), HipInferenceModel(cfg, wn)
    try:
        with pytest.raises(AhaHipError) as e:
            a.quantize_weights("mxfp4", lm_head=True)
        assert e.value.code == -1 and "layers.1.mlp.down_proj.weight" in str(e.value) and "not finite" in str(e.value)
        assert a.weight_format is None
        ids = prompts(9, (40,))[0]
        la, ta = a.forward_initial(ids, 0)
        lb, tb = b.forward_initial(ids, 0)
        assert ta == tb and np.array_equal(bits(la), bits(lb))       # (NaN logits compare by their bits)
        a.set_profiling(True)
        a.generate_batch([ids], 3)
        assert decode_classes(a)["gemv_rows_fp4"] == 0 and decode_classes(a)["gemv_rows"] > 0
    finally:
        a.close()
        b.close()
    # an intermediate size that is a multiple of 16 but not of 32: down_proj's K
    cfg2 = tiny_qwen3(layers=1, hidden=256, heads=4, kv_heads=2, inter=528, vocab=1024)
    m2 = HipInferenceModel(cfg2, qwen3_text_weights(cfg2, seed=36))
    try:
        with pytest.raises(AhaHipError) as e:
            m2.quantize_weights("mxfp4")
        assert e.value.code == -6 and "mlp.down_proj.weight has K = 528, not a multiple of 32" in str(e.value)
        assert m2.weight_format is None
    finally:
        m2.close()
