"""-m gpu: the decode kernels after their arguments moved into plain leading (preloaded) parameters, and the fused step tail.

  * bit for bit against the library before the change: tests/golden/decode_parent_digests.json (tests/decode_digests.py, run once on that
    commit on an MI355X) against the same digests recomputed here;
  * the logits epilogue's argmax rule on planted equal maxima (the lower index wins);
  * the device-resident loop (one step_tail_kernel per step) against the host loop (argmax, advance and embed launches) on the same
    matvecs: identical tokens and identical last logits, single-split and split-KV attention;
  * a stop token still bounds the steps the device loop executes.
"""
import json
import os
import sys

import numpy as np
import pytest
import torch

from aha_amd.configs import tiny_qwen3
from aha_amd.weights import qwen3_text_weights

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import decode_digests  # noqa: E402

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "decode_parent_digests.json")


@pytest.fixture(scope="module")
def text_model(gpu):
    from aha_amd.model import HipInferenceModel
    cfg = tiny_qwen3(layers=2, hidden=512, heads=4, kv_heads=2, inter=1024, vocab=2048)
    m = HipInferenceModel(cfg, qwen3_text_weights(cfg, seed=3))
    yield cfg, m
    m.close()


def test_decode_kernels_match_the_parent_digests(gpu):
    with open(GOLDEN) as f:
        want = json.load(f)
    got = decode_digests.compute()
    assert sorted(got) == sorted(want)
    diff = {k: (got[k][:12], want[k][:12]) for k in want if got[k] != want[k]}
    assert not diff, f"outputs differ from the parent commit's: {diff}"


def test_planted_equal_maxima_pick_the_lower_index(gpu):
    # The planted rows are equal element for element (+-0.5, exact in bf16), so their f32 sums -- one wave per row, the same order of
    # additions -- and the bf16 roundings of those sums are equal whatever the hidden state is: checked on the returned logits, together
    # with the pair being the maximum.
    lg, am, toks, last = decode_digests.logits_case()
    for logits, tok in ((lg, am), (last, toks[-1])):
        pos, neg = decode_digests.TIE_POS, decode_digests.TIE_NEG
        assert logits[pos[0]] == logits[pos[1]] and logits[neg[0]] == logits[neg[1]] and logits[pos[0]] == -logits[neg[0]]
        pair = pos if logits[pos[0]] > 0 else neg
        assert logits[pair[0]] == logits.max() and int((logits == logits.max()).sum()) == 2, "the planted pair is not the maximum"
        assert tok == min(pair) == int(np.argmax(logits))


@pytest.mark.parametrize("n_prompt", [40, 300])   # one KV page: a single split; five pages: two splits (published partials)
def test_fused_tail_equals_the_three_kernel_tail(text_model, n_prompt):
    cfg, m = text_model
    g = torch.Generator().manual_seed(100 + n_prompt)
    ids = torch.randint(0, cfg.vocab_size, (n_prompt,), generator=g).tolist()
    m.clear_cache()
    _, tok = m.forward_initial(ids, 0, want_logits=False)
    host, t, host_logits = [], tok, None
    for i in range(12):
        lg, t = m.forward_step(t, n_prompt + i)
        host.append(int(t))
        if i == 7:
            host_logits = np.array(lg, dtype=np.float32, copy=True)
    m.clear_cache()
    _, tok2 = m.forward_initial(ids, 0, want_logits=False)
    assert tok2 == tok
    dev = m.decode_greedy(tok, n_prompt, 8)
    dev_logits = m.last_logits()
    assert len(dev) == 8 and m.cache_len() == n_prompt + 8
    assert dev == host[:8]
    assert np.array_equal(host_logits.view(np.uint32), dev_logits.view(np.uint32))
    # the loop leaves a state a further call continues from
    dev += m.decode_greedy(dev[-1], n_prompt + 8, 4)
    assert dev == host


def test_stop_token_bounds_the_steps_of_the_fused_tail_loop(gpu):
    from aha_amd.model import HipInferenceModel
    cfg = tiny_qwen3(layers=2, hidden=512, heads=4, kv_heads=2, inter=1024, vocab=2048)
    w = qwen3_text_weights(cfg, seed=3)
    g = torch.Generator().manual_seed(77)
    ids = torch.randint(0, cfg.vocab_size, (40,), generator=g).tolist()
    m0 = HipInferenceModel(cfg, w)
    _, tok = m0.forward_initial(ids, 0, want_logits=False)
    base = m0.decode_greedy(tok, 40, 32)
    m0.close()
    stop_at = next(i for i in range(2, 32) if base[i] not in base[:i] and base[i] != tok)   # step index >= 2: the third step or later
    cfg.eos_token_ids = [base[stop_at]]
    ahead = max(1, min(64, int(os.environ.get("AHA_DECODE_RUNAHEAD", "4"))))
    try:
        m = HipInferenceModel(cfg, w)
        _, tok1 = m.forward_initial(ids, 0, want_logits=False)
        out = m.decode_greedy(tok1, 40, 32)
        assert tok1 == tok and out == base[: stop_at + 1]
        assert stop_at + 1 <= m.debug_steps_executed() <= stop_at + 1 + ahead - 1, (stop_at, m.debug_steps_executed())
        assert m.cache_len() == 40 + stop_at + 1
        m.close()
    finally:
        cfg.eos_token_ids = []
