"""-m gpu: draft-and-verify greedy decoding (aha_hip_generate_batch_spec / HipInferenceModel.generate_batch_spec).

The contract is equality, not closeness: tokens, n_out and logits are those of generate_batch on the same model in the same process
(np.array_equal on the logits' bit patterns), whatever the drafts are -- true predictions, wrong ones, corrupted ones, none.  On top of
that the call's statistics (decode steps, rows, proposed, accepted) must equal a host simulation of the documented scheduler: the
Python proposer (aha_amd/speculative.py), the row budget, the trim to max_new, acceptance = the longest draft prefix that equals the
greedy continuation.  The simulation also asserts, step by step, that the rows never pass the row budget.

Models: random-weight tiny Qwen3 (arbitrary, non-decisive tokens: nothing but row isolation makes the bits equal), the decisive tied
Qwen3 (alternates 2i <-> 2i+1: prompt lookup is right) and the decisive untied Qwen3-VL text model (walks a permutation: nothing
repeats, lookups stay silent)."""
import math
import os
import sys

import numpy as np
import pytest

from aha_amd._lib import AhaHipError
from aha_amd.configs import tiny_qwen3, tiny_qwen3vl
from aha_amd.speculative import SpecConfig, propose, row_budget
from aha_amd.weights import qwen3_text_weights, qwen3vl_weights

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import decisive  # noqa: E402

pytestmark = pytest.mark.gpu


def prompts_for(lens, seed, vocab):
    g = np.random.default_rng(seed)
    return [[int(x) for x in g.integers(0, vocab, size=n)] for n in lens]


@pytest.fixture(scope="module")
def rand_model(gpu):
    from aha_amd.model import HipInferenceModel
    cfg = tiny_qwen3(layers=3, hidden=512, heads=4, kv_heads=2, inter=1024, vocab=4096)
    m = HipInferenceModel(cfg, qwen3_text_weights(cfg, seed=0))
    yield cfg, m
    m.close()


@pytest.fixture(scope="module")
def wide_model(gpu):
    """g = 2 query heads per kv head on 8 kv heads, scrambled physical pages"""
    from aha_amd.model import HipInferenceModel
    cfg = tiny_qwen3(layers=2, hidden=1024, heads=16, kv_heads=8, inter=3072, vocab=4096)
    m = HipInferenceModel(cfg, qwen3_text_weights(cfg, seed=0))
    m.debug_scramble_pages(True)
    yield cfg, m
    m.close()


def tied_weights():
    cfg = tiny_qwen3(layers=3, hidden=512, heads=4, kv_heads=2, inter=1024, vocab=2048, tie=True)
    w = qwen3_text_weights(cfg, seed=0)
    decisive.make_tied_decisive(w, "model.embed_tokens.weight", "model.norm.weight", scale=32.0, seed=7, n_text=2000)
    return cfg, w


@pytest.fixture(scope="module")
def tied(gpu):
    from aha_amd.model import HipInferenceModel
    cfg, w = tied_weights()
    m = HipInferenceModel(cfg, w)
    yield cfg, m
    m.close()


@pytest.fixture(scope="module")
def untied_vl(gpu):
    from aha_amd.model import HipInferenceModel
    cfg = tiny_qwen3vl()
    w = qwen3vl_weights(cfg, seed=0)
    decisive.make_untied_decisive(w, "model.language_model.embed_tokens.weight", "lm_head.weight", scale=32.0, seed=7, n_text=2000)
    m = HipInferenceModel(cfg, w)
    yield cfg.text, m
    m.close()


def simulate(prompts, outs, max_new, spec, preds, stop=()):
    """The documented scheduler on the host, given the greedy outputs `outs`: per-sequence proposed / accepted, decode steps, rows."""
    n = len(prompts)
    gen = [o[:1] for o in outs]
    active = [j for j in range(n) if max_new > 1]
    proposed, accepted, steps, rows = [0] * n, [0] * n, 0, 0
    while active:
        budget = row_budget(len(active))
        extra = budget - len(active)
        step_rows, nxt = 0, []
        for j in active:
            t = len(gen[j])
            room = min(extra, max_new - t - 1)
            d = propose(spec, prompts[j] + gen[j], len(prompts[j]), None if preds is None else preds[j])[:room] if room > 0 else []
            extra -= len(d)
            step_rows += 1 + len(d)
            left = outs[j][t:]
            a = 0
            while a < len(d) and a < len(left) and d[a] == left[a]:
                a += 1
            kept = left[:a + 1]
            proposed[j] += len(d)
            accepted[j] += min(a, len(kept))
            gen[j] = gen[j] + kept
            assert len(kept) >= 1
            if not (kept[-1] in stop or len(gen[j]) == max_new):
                nxt.append(j)
        assert step_rows <= budget, "the row budget: rows of a step never pass the next multiple of 32 at or above its sequences"
        steps += 1
        rows += step_rows
        active = nxt
    assert gen == outs
    return proposed, accepted, steps, rows


def check(m, prompts, max_new, spec, preds, stop=(), **kw):
    """generate_batch_spec against generate_batch (tokens, n_out, logits: equal) and its statistics against the simulation."""
    base, lb = m.generate_batch(prompts, max_new, want_logits=True, **kw)
    assert m.cache_len() == 0
    got, lg, info = m.generate_batch_spec(prompts, max_new, spec, preds, want_logits=True, want_stats=True, **kw)
    assert m.cache_len() == 0, "the cache is cleared afterwards"
    assert got == base, "tokens / n_out differ from generate_batch"
    assert np.array_equal(lg.view(np.uint32), lb.view(np.uint32)), "logits differ from generate_batch"
    proposed, accepted, steps, rows = simulate(prompts, base, max_new, spec, preds, stop)
    st = info["stats"]
    assert info["proposed"] == proposed and info["accepted"] == accepted, (info, proposed, accepted)
    assert (st.decode_steps, st.rows, st.proposed, st.accepted) == (steps, rows, sum(proposed), sum(accepted)), (st, steps, rows)
    return base, info


def test_true_prediction_accepts_everything(rand_model, tied, untied_vl):
    """The test that fails without the feature.  Prediction = the greedy continuation itself: rule 1 drafts p[t : t + D] at every step, all
    of it is accepted, so a sequence needs exactly ceil((n_out - 1) / (D + 1)) decode steps."""
    for cfg, m in (rand_model, tied, untied_vl):
        vocab = min(cfg.vocab_size, 2000)
        prompts = prompts_for([5, 64, 130], 51, vocab)
        max_new = 40
        truth = m.generate_batch(prompts, max_new)
        for D in (1, 3, 7, 15):
            spec = SpecConfig(D, 1, 3)
            for j, p in enumerate(prompts):   # a single sequence: stats.decode_steps is its own
                base, info = check(m, [p], max_new, spec, [truth[j]])
                n_out = len(base[0])
                assert info["stats"].decode_steps == math.ceil((n_out - 1) / (D + 1)), (D, j)
                assert info["accepted"] == info["proposed"] == [n_out - 1 - info["stats"].decode_steps], (D, j, info)
            # two sequences (2 x 16 rows fit the budget at every D): the call takes the slower sequence's steps
            base, info = check(m, prompts[:2], max_new, spec, truth[:2])
            assert info["stats"].decode_steps == max(math.ceil((len(o) - 1) / (D + 1)) for o in base)
            assert info["accepted"] == info["proposed"] and all(a > 0 for a in info["accepted"])


def test_every_prediction_token_wrong(rand_model, tied, untied_vl):
    """p = (true + 1) mod vocab: rule 1 never fires.  On the untied model (a permutation walk, nothing repeats; n-grams of length >= 2, so
    that no chance 1-gram hit drafts anything right) no draft can be accepted: accepted == 0 and every token takes its own step.  On the
    other models lookups in the context may still be right; the output must be equal all the same."""
    cfg, m = untied_vl
    prompts = prompts_for([7, 63, 100], 52, 2000)
    truth = m.generate_batch(prompts, 30)
    wrong = [[(t + 1) % cfg.vocab_size for t in o] for o in truth]
    for D in (1, 7, 15):
        for ps, pr in (([prompts[0]], [wrong[0]]), (prompts, wrong)):
            base, info = check(m, ps, 30, SpecConfig(D, 2, 3), pr)
            assert info["accepted"] == [0] * len(ps)
            assert info["stats"].decode_steps == max(len(o) for o in base) - 1
    # a prediction whose first token is right and whose every other token is wrong: rule 1 drafts D wrong tokens once, none is kept
    lure = [[o[0]] + [(t + 1) % cfg.vocab_size for t in o[1:]] for o in truth]
    base, info = check(m, prompts, 30, SpecConfig(7, 2, 3), lure)
    assert info["accepted"] == [0, 0, 0] and all(p >= 7 for p in info["proposed"])
    assert info["stats"].decode_steps == 29
    for cfg2, m2 in (rand_model, tied):
        prompts2 = prompts_for([7, 63, 100], 53, min(cfg2.vocab_size, 2000))
        truth2 = m2.generate_batch(prompts2, 30)
        check(m2, prompts2, 30, SpecConfig(7, 1, 3), [[(t + 1) % cfg2.vocab_size for t in o] for o in truth2])


def test_seeded_partial_corruption(rand_model, untied_vl):
    for (cfg, m), seed in ((untied_vl, 61), (rand_model, 62)):
        prompts = prompts_for([9, 70, 129, 40], seed, min(cfg.vocab_size, 2000))
        truth = m.generate_batch(prompts, 48)
        g = np.random.default_rng(seed)
        preds = [[(t + 1) % cfg.vocab_size if g.random() < 0.25 else t for t in o] for o in truth]
        for D in (3, 7):
            _, info = check(m, prompts, 48, SpecConfig(D, 1, 3), preds)
            assert 0 < info["stats"].accepted < info["stats"].proposed, info


def test_prompt_lookup_without_predictions(rand_model, tied, wide_model):
    """No predictions: the drafts come from the context alone (rule 3).  Prompts are a repeated block."""
    for cfg, m in (tied, rand_model, wide_model):
        g = np.random.default_rng(71)
        prompts = [[int(x) for x in g.integers(0, min(cfg.vocab_size, 2000), size=b)] * r for b, r in ((8, 5), (3, 30), (21, 4), (2, 1))]
        for preds in (None, [None] * len(prompts), [[]] * len(prompts)):
            _, info = check(m, prompts, 32, SpecConfig(7, 1, 3), preds)
            assert info["stats"].proposed > 0
    # the tied model alternates 2i <-> 2i+1: from its third token on the lookup is right
    cfg, m = tied
    _, info = check(m, prompts_for([10], 72, 2000), 32, SpecConfig(7, 1, 3), None)
    assert info["stats"].accepted > 0 and info["stats"].decode_steps < 31


def test_page_and_split_boundaries(rand_model, wide_model):
    """Drafts that cross a 64-token page (prompt lengths 60 .. 66) and runs inside which the cache length crosses 256 and 512, where the
    attention's split count changes (one block per 4 pages): every row splits by its own length, as it would alone."""
    for cfg, m in (rand_model, wide_model):
        for lens, max_new in (([60, 61, 62, 63], 24), ([64, 65, 66], 24), ([250, 254, 505, 509], 20), ([241, 497], 40)):
            prompts = prompts_for(lens, 81, cfg.vocab_size)
            truth = m.generate_batch(prompts, max_new)
            for D in (7, 15):
                if len(prompts) * (D + 1) > 32 and D == 15:
                    continue
                base, info = check(m, prompts, max_new, SpecConfig(D, 1, 3), truth)
                assert info["accepted"] == info["proposed"]
                assert info["stats"].decode_steps == math.ceil((max_new - 1) / (D + 1))
            # corrupted predictions at the same boundaries: rejected rows leave K/V behind that the next steps overwrite
            g = np.random.default_rng(82)
            preds = [[(t + 1) % cfg.vocab_size if g.random() < 0.3 else t for t in o] for o in truth]
            check(m, prompts, max_new, SpecConfig(7, 1, 3), preds)


def test_stop_token_and_max_new_inside_an_accepted_run(tied):
    from aha_amd.model import HipInferenceModel
    a = 600
    cfg2, w = tied_weights()
    cfg2.eos_token_ids = [a]
    m = HipInferenceModel(cfg2, w)
    try:
        prompts = [[5, 9, a], [11, a ^ 1], [40, 41, 42, 43], [100] * 70, [7, a ^ 1, a ^ 1]]
        base = m.generate_batch(prompts, 9)
        assert base[0] == [a ^ 1, a] and base[1] == [a, a ^ 1, a]   # (tests/test_generate_batch_gpu.py::test_generate_batch_stop_tokens)
        # what the model would go on to say: the accepted run reaches past the stop token, the output is cut at it and keeps it
        preds = [[a ^ 1, a] * 5, [a, a ^ 1] * 5, [42, 43] * 5, [101, 100] * 5, [a, a ^ 1] * 5]
        for D in (1, 3, 7, 15):
            got, info = check(m, prompts, 9, SpecConfig(D, 1, 3), preds, stop=(a,))
            assert got[0] == [a ^ 1, a] and got[1] == [a, a ^ 1, a] and got[4] == [a, a ^ 1, a]
            check(m, prompts, 9, SpecConfig(D, 1, 3), None, stop=(a,))
    finally:
        m.close()
    # max_new inside a run the prediction would carry further, and max_new == 1 (no decode step at all)
    cfg, m = tied
    prompts = prompts_for([5, 64, 130], 91, 2000)
    long_pred = [[p[-1] ^ 1, p[-1]] * 20 for p in prompts]
    for max_new in (2, 3, 6, 9, 17):
        for D in (3, 7, 15):
            base, info = check(m, prompts[:2], max_new, SpecConfig(D, 1, 3), long_pred[:2])
            assert all(len(o) == max_new for o in base)
            assert info["stats"].decode_steps == math.ceil((max_new - 1) / (D + 1))
    base, info = check(m, prompts, 1, SpecConfig(7, 1, 3), long_pred)
    assert all(len(o) == 1 for o in base) and info["stats"].decode_steps == 0 and info["stats"].rows == 0


def test_batch_of_more_than_32_rows(rand_model, tied):
    """40 sequences of mixed lengths, every third without a prediction: two row groups, and drafts granted in submission order until the
    step's rows reach 64 (the simulation in check() asserts the budget step by step and the totals must equal it)."""
    for cfg, m in (rand_model, tied):
        lens = [1, 63, 64, 65, 300, 7, 129, 64] * 5
        prompts = prompts_for(lens, 101, min(cfg.vocab_size, 2000))
        truth = m.generate_batch(prompts, 20)
        g = np.random.default_rng(102)
        preds = [None if j % 3 == 2 else [(t + 1) % cfg.vocab_size if g.random() < 0.1 else t for t in o] for j, o in enumerate(truth)]
        for D in (3, 15):
            _, info = check(m, prompts, 20, SpecConfig(D, 1, 3), preds)
            assert info["stats"].proposed > 0 and info["stats"].rows <= info["stats"].decode_steps * 64
        # 33 sequences: 31 rows of drafts at most in the first steps
        check(m, prompts[:33], 20, SpecConfig(7, 1, 3), preds[:33])
        # several prefill passes
        check(m, prompts[:12], 20, SpecConfig(7, 1, 3), preds[:12], max_tokens_per_pass=256)


def test_qwen3vl_text_model_untied_head(untied_vl):
    cfg, m = untied_vl
    prompts = prompts_for([1, 63, 64, 65, 300, 7], 111, 2000)
    truth = m.generate_batch(prompts, 32)
    _, info = check(m, prompts, 32, SpecConfig(3, 1, 3), truth)
    assert info["accepted"] == info["proposed"]
    g = np.random.default_rng(112)
    check(m, prompts, 32, SpecConfig(7, 1, 2), [[(t + 1) % cfg.vocab_size if g.random() < 0.2 else t for t in o] for o in truth])
    check(m, prompts, 32, SpecConfig(7, 1, 2), None)


def test_speculation_off_cache_state_and_errors(tied):
    cfg, m = tied
    L = cfg.num_hidden_layers
    prompts = prompts_for([90, 5, 64], 121, 2000)
    truth = m.generate_batch(prompts, 12)

    def launches(spec, preds):
        m.set_profiling(False)
        m.set_profiling(True)
        got, info = m.generate_batch_spec(prompts, 12, spec, preds, want_stats=True)
        prof = {k: m.get_profile(k)["launches"] for k in ("kv_append_rows", "spec_accept_rows", "attn_decode_batch")}
        m.set_profiling(False)
        assert got == truth and m.cache_len() == 0
        return prof, info["stats"]

    # max_draft == 0: generate_batch's own steps, no new kernel is launched
    prof, st = launches(SpecConfig(0, 1, 3), truth)
    assert prof == {"kv_append_rows": 0, "spec_accept_rows": 0, "attn_decode_batch": L * 11}, prof
    assert (st.decode_steps, st.rows, st.proposed, st.accepted) == (11, 33, 0, 0)
    check(m, prompts, 12, SpecConfig(0, 1, 3), truth)
    # max_draft > 0 with drafts in every step: one append launch and one attention launch per layer per step
    prof, st = launches(SpecConfig(3, 1, 3), truth)
    assert st.decode_steps == 3
    assert prof == {"kv_append_rows": L * 3, "spec_accept_rows": 3, "attn_decode_batch": L * 3}, prof
    # a step without any draft takes the single-launch path: a 1-token context offers nothing to look up in its first step
    m.set_profiling(True)
    got, info = m.generate_batch_spec([[5]], 2, SpecConfig(3, 2, 3), None, want_stats=True)
    prof = m.get_profile("kv_append_rows")["launches"], m.get_profile("attn_decode_batch")["launches"]
    m.set_profiling(False)
    assert info["stats"].proposed == 0 and prof == (0, L), prof
    # errors: before any device work, the cache stays cleared
    for bad_pred in ([[1, 2], [3, cfg.vocab_size], [4]], [[0xFFFFFFFF], [], []]):
        with pytest.raises(AhaHipError, match="prediction id out of range"):
            m.generate_batch_spec(prompts, 12, SpecConfig(3, 1, 3), bad_pred)
        assert m.cache_len() == 0
    with pytest.raises(AhaHipError, match="max_draft must be in 0..15"):
        m.generate_batch_spec(prompts, 12, SpecConfig(16, 1, 3), truth)
    with pytest.raises(AhaHipError):
        m.generate_batch_spec([[1, 2], []], 4, SpecConfig(3, 1, 3), None)
    with pytest.raises(AhaHipError):
        m.generate_batch_spec(prompts, 0, SpecConfig(3, 1, 3), None)
    assert m.cache_len() == 0
    # the model still answers as before
    assert m.generate_batch(prompts, 12) == truth
    from aha_amd.model import generate_generic_batch_spec
    out, usage = generate_generic_batch_spec(m, prompts, 12, SpecConfig(3, 1, 3), truth)
    # per sequence 11 tokens after the first in 3 steps: 3 + 3 + 2 drafts, all kept
    assert out == truth and usage.accepted_prediction_tokens == 24 and usage.rejected_prediction_tokens == 0
