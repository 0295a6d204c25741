"""-m gpu: the E4M3 KV cache behind generate_batch (HipInferenceModel.set_kv_format("e4m3")).

1. Greedy tokens: on a decisive-margin checkpoint (tests/decisive.py) the KV8 model returns the bf16-cache model's tokens exactly, through
   generate_batch and generate_batch_spec; the prompts (60 and 126 tokens) cross a page boundary during the 12 decode steps.
2. Deviation on a plain checkpoint: the logits of the last of 33 steps, d = rms(difference) / std in logit-std units.  All three models
   are walked down ONE token sequence (a mask that allows one id per step), so the figures compare caches, not diverged texts.
   d_kv: the KV8 model against the bf16-cache model; the yardstick d_w, measured here: what quantize_weights("mxfp8") alone does to the
   same request -- the same element format on the other operand stream.  d_kv <= 2 d_w (the factor of tests/test_prefill_fp8_gpu.py).
3. The rules: what a KV8 model refuses, when the format may be set, the default.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import decisive  # noqa: E402

from aha_amd import guided  # noqa: E402
from aha_amd._lib import AhaHipError  # noqa: E402
from aha_amd.configs import tiny_qwen3  # noqa: E402
from aha_amd.weights import qwen3_text_weights  # noqa: E402

pytestmark = pytest.mark.gpu


def cfg_weights(seed):
    cfg = tiny_qwen3(layers=2, hidden=256, heads=4, kv_heads=2, inter=512, vocab=1024, tie=True)
    return cfg, qwen3_text_weights(cfg, seed=seed)


def build(cfg, w, kv=None, wq=None):
    from aha_amd.model import HipInferenceModel
    m = HipInferenceModel(cfg, w)
    if wq:
        m.quantize_weights(wq)
    if kv:
        m.set_kv_format(kv)
    return m


def prompts_of(cfg, lens, seed):
    rng = np.random.default_rng(seed)
    return [[int(x) for x in rng.integers(0, cfg.vocab_size, size=n)] for n in lens]


@pytest.mark.parametrize("spec", [False, True])
def test_greedy_tokens_equal_the_bf16_cache_models(gpu, spec):
    cfg, w = cfg_weights(42)
    decisive.make_tied_decisive(w, "model.embed_tokens.weight", "model.norm.weight", scale=32.0, seed=7, n_text=cfg.vocab_size)
    prompts = prompts_of(cfg, [60, 126, 5], 4)
    u, k = build(cfg, w), build(cfg, w, kv="e4m3")
    try:
        assert k.kv_format == "e4m3" and u.kv_format == "bf16"
        want = u.generate_batch(prompts, 12)
        got = k.generate_batch_spec(prompts, 12, predictions=want) if spec else k.generate_batch(prompts, 12)
        assert [len(t) for t in want] == [12, 12, 12] and got == want
        k.set_profiling(True)
        k.generate_batch(prompts, 3)
        assert k.get_profile("attn_decode_batch_kv8")["launches"] == 2 * cfg.num_hidden_layers and k.get_profile("attn_decode_batch")["launches"] == 0
        assert k.get_profile("kv_pages_quantize")["launches"] == 1
    finally:
        u.close()
        k.close()


def test_kv8_deviates_no_more_than_twice_the_weight_quantisation(gpu):
    cfg, w = cfg_weights(41)
    prompts, steps = prompts_of(cfg, [100, 40], 5), 33
    path = [[int(x) for x in np.random.default_rng(6 + j).integers(0, cfg.vocab_size, size=steps)] for j in range(2)]
    lg = {}
    for name, kw in (("U", {}), ("K", dict(kv="e4m3")), ("Q", dict(wq="mxfp8"))):
        m = build(cfg, w, **kw)
        try:
            toks, _, step_logits = m.generate_batch_masked(prompts, steps, want_step_logits=True,
                                                           constraint=lambda seq, gen: guided.pack_mask([path[seq][len(gen)]], cfg.vocab_size))
            assert toks == path, name
            lg[name] = np.asarray(step_logits[:, steps - 1], dtype=np.float64)
            assert np.isfinite(lg[name]).all(), name
        finally:
            m.close()
    d_kv = float(np.sqrt(((lg["K"] - lg["U"]) ** 2).mean()) / lg["U"].std())
    d_w = float(np.sqrt(((lg["Q"] - lg["U"]) ** 2).mean()) / lg["U"].std())
    print(f"d_kv = {d_kv:.5f}, d_w = {d_w:.5f}, ratio {d_kv / d_w:.3f}")
    assert 0 < d_kv <= 2 * d_w, (d_kv, d_w)


def test_format_rules(gpu):
    from aha_amd.model import HipEngine
    cfg, w = cfg_weights(41)
    m = build(cfg, w)
    try:
        assert m.kv_format == "bf16"                      # never asked
        _, tok = m.forward_initial([1, 2, 3], 0)
        with pytest.raises(AhaHipError) as e:             # a non-empty cache
            m.set_kv_format("e4m3")
        assert e.value.code == -7 and m.kv_format == "bf16"
        m.clear_cache()
        m.set_kv_format("e4m3")
        for call in (lambda: m.forward_step(tok, 0), lambda: m.decode_greedy(tok, 0, 4), lambda: HipEngine(m), m.kv_export):
            with pytest.raises(AhaHipError) as e:
                call()
            assert e.value.code == -6, str(e.value)
        m.set_kv_format("bf16")
        assert m.kv_format == "bf16" and len(m.generate_batch([[1, 2, 3]], 2)[0]) == 2
    finally:
        m.close()
