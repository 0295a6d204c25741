"""-m gpu: prefill from the MXFP8 copies (quantize_weights_with("mxfp8", prefill=True), AHA_WQ_PREFILL) end to end, on the small text config of
the FP8 tests.  Three models from the same weights: U unquantised, Q quantised, P quantised with the flag.

4. Reach: a prefill of P runs 4 x layers quant_rows + gemm_fp8 launches in place of as many gemm launches, Q runs none; a decode step of
   P launches the profile classes of Q's.
5. Deviation: d_a = rms(logits_P - logits_Q) / std(logits_Q) <= 2 d_w = 2 rms(logits_Q - logits_U) / std(logits_U) on one prefill of 200
   ids -- activations and weights are quantised in the same format and block size, so each GEMM takes comparable noise from either side,
   and the bf16 paths behind d_w are the yardstick.  Greedy tokens of P and Q agree for 8 steps on a decisive-margin checkpoint.
6. The flag's rules.
"""
import os
import sys

import numpy as np
import pytest

from aha_amd._lib import AhaHipError
from aha_amd.configs import tiny_qwen3
from aha_amd.weights import qwen3_text_weights

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import decisive  # noqa: E402

pytestmark = pytest.mark.gpu

CLASSES = ("gemm", "gemm_fp8", "quant_rows", "gemv", "gemv_fp8", "attn_decode", "attn_prefill", "elem", "argmax")


def cfg_weights(seed=41):
    cfg = tiny_qwen3(layers=2, hidden=256, heads=4, kv_heads=2, inter=512, vocab=1024, tie=True)
    return cfg, qwen3_text_weights(cfg, seed=seed)


def build(cfg, w, fmt=None, prefill=False):
    from aha_amd.model import HipInferenceModel
    m = HipInferenceModel(cfg, w)
    if fmt:
        m.quantize_weights_with(fmt, prefill=prefill)
    return m


@pytest.fixture(scope="module")
def models(gpu):
    cfg, w = cfg_weights()
    ms = {"U": build(cfg, w), "Q": build(cfg, w, "mxfp8"), "P": build(cfg, w, "mxfp8", prefill=True)}
    yield cfg, ms
    for m in ms.values():
        m.close()


def launches(m, fn):
    m.set_profiling(True)
    fn()
    out = {c: m.get_profile(c)["launches"] for c in CLASSES}
    m.set_profiling(False)
    return out


@pytest.mark.parametrize("n_ids", [200, 3])
def test_prefill_reaches_the_fp8_gemm_and_decode_does_not(models, n_ids):
    cfg, ms = models
    ids = [int(x) for x in np.random.default_rng(2).integers(0, cfg.vocab_size, size=n_ids)]
    L, tok, pre = cfg.num_hidden_layers, {}, {}
    for k in ("Q", "P"):
        ms[k].clear_cache()
        pre[k] = launches(ms[k], lambda: tok.__setitem__(k, ms[k].forward_initial(ids, 0)[1]))
    assert pre["Q"]["gemm_fp8"] == 0 and pre["Q"]["quant_rows"] == 0 and pre["Q"]["gemm"] >= 4 * L, pre
    assert pre["P"]["gemm_fp8"] == 4 * L and pre["P"]["quant_rows"] == 4 * L and pre["P"]["gemm"] == pre["Q"]["gemm"] - 4 * L, pre
    step = {k: launches(ms[k], lambda: ms[k].forward_step(tok[k], n_ids)) for k in ("Q", "P")}
    assert step["P"] == step["Q"] and step["P"]["gemm_fp8"] == 0 and step["P"]["quant_rows"] == 0, step


def test_activation_quantisation_deviates_no_more_than_twice_the_weight_quantisation(models):
    cfg, ms = models
    ids = [int(x) for x in np.random.default_rng(3).integers(0, cfg.vocab_size, size=200)]
    lg = {}
    for k, m in ms.items():
        m.clear_cache()
        lg[k] = np.asarray(m.forward_initial(ids, 0)[0], dtype=np.float64)
        assert np.isfinite(lg[k]).all(), k
    d_a = float(np.sqrt(((lg["P"] - lg["Q"]) ** 2).mean()) / lg["Q"].std())
    d_w = float(np.sqrt(((lg["Q"] - lg["U"]) ** 2).mean()) / lg["U"].std())
    print(f"d_a = {d_a:.5f}, d_w = {d_w:.5f}, ratio {d_a / d_w:.3f}")
    assert 0 < d_a <= 2 * d_w, (d_a, d_w)


def test_greedy_tokens_agree_on_a_decisive_checkpoint(gpu):
    from aha_amd.model import generate_generic
    cfg, w = cfg_weights(seed=42)
    decisive.make_tied_decisive(w, "model.embed_tokens.weight", "model.norm.weight", scale=32.0, seed=7, n_text=cfg.vocab_size)
    ids = [int(x) for x in np.random.default_rng(4).integers(0, cfg.vocab_size, size=40)]
    q, p = build(cfg, w, "mxfp8"), build(cfg, w, "mxfp8", prefill=True)
    try:
        assert decisive.margin_std(q.forward_initial(ids, 0)[0]) >= 0.5
        q.clear_cache()
        tq, tp = generate_generic(q, ids, 8)[0], generate_generic(p, ids, 8)[0]
        assert len(tq) == 8 and tq == tp
    finally:
        q.close()
        p.close()


def test_flag_rules(gpu):
    from aha_amd import _lib
    cfg, w = cfg_weights()
    q, f = build(cfg, w, "mxfp8"), build(cfg, w)
    try:
        with pytest.raises(AhaHipError) as e:
            f.quantize_weights_with("mxfp4", prefill=True)
        assert e.value.code == -6 and "AHA_WQ_PREFILL needs AHA_WQ_MXFP8_E4M3" in str(e.value) and f.weight_format is None
        with pytest.raises(AhaHipError) as e:     # Q again, now with the flag: other arguments
            q.quantize_weights_with("mxfp8", prefill=True)
        assert e.value.code == -7 and "already quantised with format 1, flags 0" in str(e.value)
        assert q.weight_format == ("mxfp8", False)
        f.quantize_weights_with("mxfp8", prefill=True)
        f.quantize_weights_with("mxfp8", prefill=True)   # the same arguments again: nothing happens
        assert f.weight_format == ("mxfp8", False, "prefill")
        fl = _lib.C.c_uint32()
        _lib.check(_lib.lib().aha_hip_model_weight_format(f.handle, None, _lib.C.byref(fl)))
        assert fl.value == _lib.AHA_WQ_PREFILL
    finally:
        q.close()
        f.close()
