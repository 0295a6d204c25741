"""-m gpu: single-sequence decode over the E4M3 KV cache (set_kv_format_with("e4m3", single=True)) on the tiny config
of tests/test_kv8_model_gpu.py: greedy tokens equal to the bf16-cache model's on a decisive-margin checkpoint (prompts of 60 and 126 tokens
cross a page boundary in 12 steps; linear form and, pages shuffled, table form); the logit deviation after 100 prompt and 33 GIVEN tokens
against that of quantize_weights("mxfp8") alone (d_kv <= 2 d_w, test_kv8_model_gpu.py's factor and yardstick); the rules of the flag."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import decisive  # noqa: E402
from test_kv8_model_gpu import build, cfg_weights, prompts_of  # noqa: E402

from aha_amd._lib import AhaHipError  # noqa: E402

pytestmark = pytest.mark.gpu


def flagged(cfg, w, scramble=False):
    m = build(cfg, w)
    m.debug_scramble_pages(scramble)
    m.set_kv_format_with("e4m3", single=True)
    return m


def step_loop(m, tok, offset, n):
    out = [tok]
    for i in range(n):
        out.append(m.forward_step(out[-1], offset + i)[1])
    return out[1:]


@pytest.mark.parametrize("scramble", [False, True])
def test_greedy_tokens_equal_the_bf16_cache_models(gpu, scramble):
    cfg, w = cfg_weights(42)
    decisive.make_tied_decisive(w, "model.embed_tokens.weight", "model.norm.weight", scale=32.0, seed=7, n_text=cfg.vocab_size)
    u, k = build(cfg, w), flagged(cfg, w, scramble)
    try:
        k.set_profiling(True)
        for prompt in prompts_of(cfg, [60, 126], 4):
            u.clear_cache()
            tok = u.forward_initial(prompt, 0)[1]
            want = u.decode_greedy(tok, len(prompt), 12)
            for decode in (lambda: k.decode_greedy(tok, len(prompt), 12), lambda: step_loop(k, tok, len(prompt), 12)):
                k.clear_cache()
                assert k.forward_initial(prompt, 0)[1] == tok and k.kv_format == ("e4m3", "single")
                assert len(want) == 12 and decode() == want
                assert k.debug_attn_decode_form() == (0 if scramble else 1)
        assert k.get_profile("attn_decode_kv8")["launches"] == 4 * 12 * cfg.num_hidden_layers and k.get_profile("attn_decode")["launches"] == 0
        assert k.get_profile("kv_pages_quantize")["launches"] == 4     # one per forward_initial
    finally:
        u.close()
        k.close()


def test_kv8_deviates_no_more_than_twice_the_weight_quantisation(gpu):
    cfg, w = cfg_weights(41)
    prompt, steps, lg = prompts_of(cfg, [100], 5)[0], 33, {}
    path = [int(x) for x in np.random.default_rng(6).integers(0, cfg.vocab_size, size=steps)]
    for name, make in (("U", build), ("K", flagged), ("Q", lambda c, x: build(c, x, wq="mxfp8"))):
        m = make(cfg, w)
        try:
            m.forward_initial(prompt, 0, want_logits=False)
            for i, t in enumerate(path):
                logits, _ = m.forward_step(t, len(prompt) + i, want_logits=i == steps - 1)
            lg[name] = np.asarray(logits, dtype=np.float64)
        finally:
            m.close()
    d_kv = float(np.sqrt(((lg["K"] - lg["U"]) ** 2).mean()) / lg["U"].std())
    d_w = float(np.sqrt(((lg["Q"] - lg["U"]) ** 2).mean()) / lg["U"].std())
    print(f"d_kv = {d_kv:.5f}, d_w = {d_w:.5f}, ratio {d_kv / d_w:.3f}")
    assert 0 < d_kv <= 2 * d_w, (d_kv, d_w)


def test_flag_rules(gpu):
    from aha_amd.model import HipEngine
    cfg, w = cfg_weights(41)
    m, u = build(cfg, w), build(cfg, w)
    prompt = prompts_of(cfg, [70], 9)[0]
    try:
        _, tok = u.forward_initial(prompt, 0)
        # the flag needs the format; a flagged model refuses the engine, kv_export and (its steps append to the E4M3 pages only) a continuation prefill
        for code, call in ((-1, lambda: m.set_kv_format_with("bf16", single=True)), (0, lambda: m.set_kv_format_with("e4m3", single=True)),
                           (-6, lambda: HipEngine(m)), (-6, m.kv_export), (0, lambda: m.forward_initial(prompt, 0)),
                           (-6, lambda: m.forward_initial([1, 2, 3], len(prompt)))):
            if code == 0:
                call()
                continue
            with pytest.raises(AhaHipError) as e:
                call()
            assert e.value.code == code, str(e.value)
        after_refusal = step_loop(m, tok, len(prompt), 3)  # ... and leaves the cache as it was: the tokens of an undisturbed run
        m.clear_cache()
        assert m.forward_initial(prompt, 0)[1] == tok and step_loop(m, tok, len(prompt), 3) == after_refusal
        m.clear_cache()
        m.set_kv_format("bf16")                            # back to today's behaviour: the bf16 kernel on the bf16 pages
        assert m.kv_format == "bf16" and m.forward_initial(prompt, 0)[1] == tok
        m.set_profiling(True)
        assert step_loop(m, tok, len(prompt), 3) == step_loop(u, tok, len(prompt), 3)
        assert m.get_profile("attn_decode_kv8")["launches"] == 0 and m.get_profile("attn_decode")["launches"] == 3 * cfg.num_hidden_layers
    finally:
        m.close()
        u.close()
