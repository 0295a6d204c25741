"""-m gpu: the batched decode matvec for 33 .. 128 rows in one pass over the weights (csrc/gemv_rows_wide_body.h).

  1. bit identity, op level: one call with R rows equals the same rows through the same entry in groups of at most 32 -- every form, every
     epilogue, R in {33, 64, 65, 128}, one shape per branch of gemv_rows_plan and per tail;
  2. exactness: R = 128, K = 1152 on integer data whose f32 sums are exact (tests/gemv_rows_exact.py), against the f64 dot products -- an
     error both sides of 1 could share;
  3. model level: generate_batch (sampled entry at temperature 0, for its step logits) and generate_batch_spec with 40 sequences give the
     same tokens and logit bits with debug_rows_wide 0 and 2, on a bf16 and on an MXFP8 model.
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gemv_exact as gx  # noqa: E402
import gemv_rows_exact as gr  # noqa: E402
from gemv_exact import LOGITS, RESIDUAL, SILU_MUL, STORE  # noqa: E402
from test_generate_batch_gpu import prompts_for  # noqa: E402

pytestmark = pytest.mark.gpu

FORMS = ("bf16", "mxfp8", "mxfp4")
ROWS = (33, 64, 65, 128)          # one row into the third tile, four full tiles, one row into the 8-tile kernel, eight full tiles
# (N, K): (cw, nks) and what the shape reaches
SHAPES = {(48, 128): (1, 1),          # one chunk, ragged column block
          (272, 640): (1, 2),
          (8192, 640): (2, 1),
          (4096, 1152): (2, 2),       # the last chunk of a split past K
          (48, 136): (1, 1)}          # bf16 only: the ragged K % 8 tail


def wide_inputs(N, K, dev):
    """W (N, K), x (128, K) with rows that differ (row r scaled by 1 + r / 64), residual (128, N); one seed per shape."""
    g = torch.Generator(device=dev).manual_seed(31 * N + K)
    W = (torch.randn(N, K, generator=g, device=dev) * 0.05).to(torch.bfloat16)
    x = (torch.randn(128, K, generator=g, device=dev) * (1 + torch.arange(128, device=dev)[:, None] / 64)).to(torch.bfloat16)
    return W, x, torch.randn(128, N, generator=g, device=dev).to(torch.bfloat16)


def runner(form, W):
    """x, epi, residual -> the outputs of the form's op entry on W (an MX form: on its quantised copy)."""
    from aha_amd import ops
    if form == "bf16":
        return lambda x, epi, res: ops.gemv_rows(W, x, epi, res)
    quantize, run = (ops.quantize_mxfp8, ops.gemv_rows_mxfp8) if form == "mxfp8" else (ops.quantize_mxfp4, ops.gemv_rows_mxfp4)
    q, scales, _ = quantize(W)
    return lambda x, epi, res: run(q, scales, x, epi, res)


@pytest.mark.parametrize("N,K,form", [(N, K, f) for N, K in SHAPES for f in FORMS if f in gr.forms(K)])
def test_wide_call_equals_groups_of_32_bit_for_bit(gpu, N, K, form):
    from aha_amd import ops
    for epi in (STORE, RESIDUAL, SILU_MUL, LOGITS):
        n = (N + 31) // 32 * 32 if epi == SILU_MUL else N          # the gate / up layout comes in 32-row blocks: 288 for 272, 64 for 48
        assert ops.plan_gemv_rows(n, K) == SHAPES[N, K]
        W, x, res = wide_inputs(n, K, gpu)
        run = runner(form, W)
        groups = [run(x[r0:r0 + 32].contiguous(), epi, res[r0:r0 + 32].contiguous() if epi == RESIDUAL else None) for r0 in range(0, 128, 32)]
        want = tuple(torch.cat([g[i] for g in groups]) for i in (0, 1)) if epi == LOGITS else torch.cat(groups)
        for R in ROWS:
            got = run(x[:R].contiguous(), epi, res[:R].contiguous() if epi == RESIDUAL else None)
            gr.assert_rows(got, tuple(t[:R] for t in want) if epi == LOGITS else want[:R], epi, f"{form} {n} x {K} R={R} epi={epi}")


@pytest.mark.parametrize("form", FORMS)
def test_wide_call_gives_the_exact_sums(gpu, form):
    N, K, R = 4096, 1152, 128
    c = gx.make_inputs(N, K, form == "mxfp4", gpu, gr.seed_of(N, K, form == "mxfp4"))
    g = torch.Generator(device=gpu).manual_seed(7)
    x = (torch.randint(1, 9, (R, K), generator=g, device=gpu) * (torch.randint(0, 2, (R, K), generator=g, device=gpu) * 2 - 1)).to(torch.bfloat16)
    sums, sabs = gr.sums_of({"W": c["W"], "x": x})
    assert float(sabs.max()) < gx.EXACT_BOUND          # on the inputs: every f32 partial sum is exact in any order
    from aha_amd import ops
    if form == "bf16":
        got = ops.gemv_rows(c["W"], x, LOGITS)
    else:
        got = (ops.gemv_rows_mxfp8 if form == "mxfp8" else ops.gemv_rows_mxfp4)(*(gx.encode_mxfp8 if form == "mxfp8" else gx.encode_mxfp4)(c), x, LOGITS)
    gr.assert_rows(got, gr.epilogue(sums, None, LOGITS), LOGITS, f"{form} {N} x {K} R={R}")


@pytest.mark.parametrize("fmt", [None, "mxfp8"])
def test_model_steps_of_40_rows_do_not_depend_on_the_switch(gpu, fmt):
    from aha_amd.configs import tiny_qwen3
    from aha_amd.model import HipInferenceModel
    from aha_amd.sampling import SamplingParams
    from aha_amd.weights import qwen3_text_weights
    cfg = tiny_qwen3(layers=2, hidden=512, heads=4, kv_heads=2, inter=1024, vocab=4096)
    m = HipInferenceModel(cfg, qwen3_text_weights(cfg, seed=0))
    try:
        if fmt:
            m.quantize_weights(fmt, lm_head=True)
        prompts = prompts_for(40, 41, cfg.vocab_size, [1, 63, 64, 65, 7])
        out = {}
        for sw in (0, 2):
            m.debug_rows_wide(sw)
            m.set_profiling(True)
            toks, step = m.generate_batch_sampled(prompts, SamplingParams(), 6, want_step_logits=True)
            wide = sum(m.get_profile(c)["launches"] for c in ("gemv_rows_wide", "gemv_rows_wide_fp8"))
            m.set_profiling(False)
            assert (wide > 0) == (sw == 2)          # the switch reaches the step: 40 rows are one wide pass, or groups of 32 + 8
            spec, last = m.generate_batch_spec(prompts, 6, predictions=toks, want_logits=True)
            out[sw] = (toks, step, spec, last)
        assert out[0][0] == out[2][0] and out[0][2] == out[2][2] and out[0][0] == out[0][2]
        assert np.array_equal(out[0][1].view(np.uint32), out[2][1].view(np.uint32))
        assert np.array_equal(out[0][3].view(np.uint32), out[2][3].view(np.uint32))
    finally:
        m.close()
