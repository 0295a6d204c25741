"""-m gpu: HipInferenceModel.score_batch (aha_hip_score_batch) on the two tiny_qwen3 shapes of tests/test_embed_batch_gpu.py: every
scored position against the f64 log-softmax of the logits forward_initial produces for the same prefix alone, and the entry's contract
(sentinels, cache, passes, errors)."""
import numpy as np
import pytest

from aha_amd._lib import AhaHipError
from aha_amd.configs import tiny_qwen3
from aha_amd.weights import qwen3_text_weights

pytestmark = pytest.mark.gpu

LENS = [1, 2, 63, 64, 65, 200]
LONG_POSITIONS = [1, 31, 64, 65, 127, 128, 191, 199]   # of the 200-token prompt; the shorter prompts are checked at every position
# The deviation the tree already has between its two prefill paths, measured at the parent commit on these prompts' prefixes (every
# checked position's prefix as a prompt of its own): the largest |first-token logprob of generate_batch_logprobs (packed prefill)
# - f64 log-softmax of forward_initial's logits at that token| over 204 prefixes per shape was 0.015675 on the wide shape (two bf16 ulps of
# a logit near 4; p99 0.015641, median 3.3e-5) and 4.0e-5 on the narrow one (median 3.4e-7: there the two paths agree almost bit for bit).
# PARITY_MEASURED is the larger; score_batch is allowed twice that on both shapes: a second kernel's accumulation order sits on top of
# the pass's.  (profiles/score_batch.md)
PARITY_MEASURED = 0.015675440779759242
BOUND = 2 * PARITY_MEASURED
SENTINEL = (None, 0xFFFFFFFF, 0.0)


def positions(n):
    return list(range(1, n)) if n <= 65 else LONG_POSITIONS


def prompts_for(cfg):
    g = np.random.default_rng(21)
    return [[int(x) for x in g.integers(0, cfg.vocab_size, size=n)] for n in LENS]


@pytest.fixture(scope="module", params=["narrow", "wide"])
def setup(gpu, request):
    """The model, its prompts and, per checked (prompt, position), the reference: f64 log-softmax of forward_initial(ids[:p]) -> (log-probability
    of ids[p], argmax, top-two margin).  Computed once, read by every test."""
    from aha_amd.model import HipInferenceModel
    if request.param == "narrow":
        cfg = tiny_qwen3(layers=3, hidden=512, heads=4, kv_heads=2, inter=1024, vocab=4096)
    else:
        cfg = tiny_qwen3(layers=2, hidden=1024, heads=16, kv_heads=8, inter=3072, vocab=4096)
    m = HipInferenceModel(cfg, qwen3_text_weights(cfg, seed=0))
    prompts, ref = prompts_for(cfg), {}
    for j, ids in enumerate(prompts):
        for p in positions(len(ids)):
            m.clear_cache()
            m.forward_initial(ids[:p], 0)
            x = m.last_logits().astype(np.float64)
            ls = x - (x.max() + np.log(np.exp(x - x.max()).sum()))
            top2 = np.sort(x)[-2:]
            ref[j, p] = (float(ls[ids[p]]), int(x.argmax()), float(top2[1] - top2[0]))
    m.clear_cache()
    yield m, cfg, prompts, ref
    m.close()


def check_against_reference(scores, prompts, ref):
    worst = 0.0
    for (j, p), (lp, top, margin) in ref.items():
        got_lp, got_top, got_tlp = scores[j][p]
        worst = max(worst, abs(got_lp - lp))
        assert got_lp <= got_tlp <= 0.0
        if margin > BOUND:
            assert got_top == top, (j, p, margin)
    print("max |logprob - ref| = %.4f over %d positions" % (worst, len(ref)))
    assert worst <= BOUND


def test_parity_with_forward_initial(setup):
    m, cfg, prompts, ref = setup
    check_against_reference(m.score_batch(prompts), prompts, ref)


def test_contract(setup):
    m, cfg, prompts, ref = setup
    before = m.generate_batch(prompts[:3], 4)
    scores = m.score_batch(prompts)
    assert m.cache_len() == 0
    assert [len(s) for s in scores] == LENS and all(s[0] == SENTINEL for s in scores)
    assert all(lp is not None and top < cfg.vocab_size for s in scores for lp, top, _ in s[1:])
    assert m.generate_batch(prompts[:3], 4) == before
    # several passes (the 200-token prompt alone in its own): the same bound
    split = m.score_batch(prompts, max_tokens_per_pass=128)
    assert [len(s) for s in split] == LENS and all(s[0] == SENTINEL for s in split)
    check_against_reference(split, prompts, ref)


@pytest.mark.parametrize("bad,words", [([[1, 2], []], ("sequence 1",)), ([[1], [2, 3, 1 << 20]], ("sequence 1", "position 2")), ([], ("n_seqs",))])
def test_errors_name_the_sequence(setup, bad, words):
    m = setup[0]
    with pytest.raises(AhaHipError) as e:
        m.score_batch(bad)
    assert e.value.code == -1 and all(w in str(e.value) for w in words)   # AHA_ERR_INVALID
    assert m.cache_len() == 0
