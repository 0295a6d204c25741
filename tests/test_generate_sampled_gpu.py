"""-m gpu: batched sampled generation (aha_hip_generate_batch_sampled / HipInferenceModel.generate_batch_sampled) and its candidate step.

  * sample_rows (the candidate step of R rows in one launch per stage): bit-identical per row to aha_hip_sample_candidates on the same
    logits, context, temperature and k, at a full-size and a tiny vocabulary; the logits are only read;
  * the driver: an exact replay of every sequence with the oracle sampler (oracle/sampling.py + oracle/rand_stdrng.py) on the step logits
    the call reports, on random-weight checkpoints whose distributions are spread; all-greedy params give aha_hip_generate_batch's tokens
    and logits; a sequence's tokens and logits do not depend on the batch; agreement with generate_generic_sampled on decisive
    checkpoints; stop tokens, the cache afterwards, and one candidate step per decode step.
"""
import os
import sys

import numpy as np
import pytest
import torch

from aha_amd._lib import AhaHipError
from aha_amd.configs import tiny_qwen3, tiny_qwen3vl
from aha_amd.sampling import SamplingParams
from aha_amd.weights import qwen3_text_weights, qwen3vl_weights
from oracle import rand_stdrng as ornd
from oracle import sampling as osamp

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import decisive  # noqa: E402

pytestmark = pytest.mark.gpu

QWEN3_DEFAULT = dict(temperature=0.6, top_p=0.95, top_k=20)   # generation_config.json of Qwen3 (qwen3/generate.rs get_temperature / ..)


def bits(x):
    return np.asarray(x, dtype=np.float32).view(np.uint32)


def prompts_for(n, seed, vocab, lens):
    g = np.random.default_rng(seed)
    return [[int(x) for x in g.integers(0, vocab, size=lens[i % len(lens)])] for i in range(n)]


# ---- the candidate step ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("vocab", [151936, 300])
def test_sample_rows_bit_identical_to_sample_candidates(gpu, vocab):
    from aha_amd import ops
    from aha_amd.model import HipInferenceModel
    cfg = tiny_qwen3(layers=1, hidden=256, heads=2, kv_heads=1, inter=512, vocab=vocab)
    m = HipInferenceModel(cfg, qwen3_text_weights(cfg, seed=3))
    g = np.random.default_rng(5)
    rows, want = [], []
    try:
        prompt = [int(x) for x in g.integers(0, vocab, size=9)]
        _, tok = m.forward_initial(prompt, 0, want_logits=False)
        off = len(prompt)
        for r in range(40):
            if r:
                _, tok = m.forward_step(int(g.integers(0, vocab)), off, want_logits=False)
                off += 1
            k = int(g.choice([1, 2, 20, 63, 64])) if r % 3 else int(g.integers(1, 65))
            t = float(g.choice([0.0, 0.6, 1.3, 7.0]))
            pen = float(g.choice([1.0, 1.2, 0.9]))
            ctx = [int(x) for x in g.integers(0, min(vocab, 64), size=int(g.integers(0, 30)))]   # repeated ids
            if r % 5 == 0:
                ctx += [vocab + 3, int(g.integers(0, vocab))]   # an id outside the vocabulary is ignored
            vals, idx, mx, se = m.sample_candidates(ctx, pen, t, k)
            rows.append((m.last_logits(), k, t, pen, ctx))
            want.append((np.asarray(vals, np.float32), np.asarray(idx, np.uint32), np.float32(mx), np.float32(se)))
        logits = torch.from_numpy(np.stack([r[0] for r in rows])).cuda()
        before = logits.clone()
        for R in (1, 7, 32, 40):
            sel = list(range(R)) if R != 7 else [3, 9, 0, 17, 30, 5, 39]
            lg = logits[sel].contiguous()
            vals, idx, ms = ops.sample_rows(lg, [rows[i][1] for i in sel], [rows[i][2] for i in sel], [rows[i][3] for i in sel],
                                            [rows[i][4] for i in sel])
            torch.cuda.synchronize()
            assert torch.equal(lg.view(torch.int32), before[sel].view(torch.int32)), "sample_rows wrote its input logits"
            vals, idx, ms = vals.cpu().numpy(), idx.cpu().numpy().view(np.uint32), ms.cpu().numpy()
            for s, i in enumerate(sel):
                k = rows[i][1]
                wv, wi, wm, ws = want[i]
                assert np.array_equal(bits(vals[s, :k]), bits(wv)), (R, i)
                assert np.array_equal(idx[s, :k], wi), (R, i)
                assert bits(ms[s, 0]) == bits(wm) and bits(ms[s, 1]) == bits(ws), (R, i, ms[s], wm, ws)
        assert torch.equal(logits.view(torch.int32), before.view(torch.int32))
    finally:
        m.close()


# ---- the driver -----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=["narrow", "wide", "vl"])
def rand_model(gpu, request):
    """Random weights as drawn: spread, undecided distributions (test_generate_batch_gpu.py's rand_model, plus text-only Qwen3-VL)."""
    from aha_amd.model import HipInferenceModel
    if request.param == "narrow":
        cfg = tiny_qwen3(layers=3, hidden=512, heads=4, kv_heads=2, inter=1024, vocab=4096)
        m = HipInferenceModel(cfg, qwen3_text_weights(cfg, seed=0))
    elif request.param == "wide":
        cfg = tiny_qwen3(layers=2, hidden=1024, heads=16, kv_heads=8, inter=3072, vocab=4096)
        m = HipInferenceModel(cfg, qwen3_text_weights(cfg, seed=0))
        m.debug_scramble_pages(True)
    else:
        cfg = tiny_qwen3vl()
        m = HipInferenceModel(cfg, qwen3vl_weights(cfg, seed=0))
    yield m.text_cfg, m
    m.close()


MIXED = [
    SamplingParams(),                                                    # greedy
    SamplingParams(0.0, repeat_penalty=1.3, repeat_last_n=5),            # greedy with a penalty
    SamplingParams(0.9, top_k=20, seed=1),                               # TopK
    SamplingParams(**QWEN3_DEFAULT, seed=2),                             # the Qwen3 default: TopKThenTopP
    SamplingParams(**QWEN3_DEFAULT, repeat_penalty=1.1, seed=3),
    SamplingParams(1.0, top_p=0.9, seed=4),                              # TopP
    SamplingParams(0.8, top_p=0.3, repeat_penalty=1.5, repeat_last_n=8, seed=5),
    SamplingParams(1.2, seed=6),                                         # All
    SamplingParams(1.0, top_k=100, seed=7),                              # k > 64: the full vector
    SamplingParams(0.7, top_p=0.8, top_k=100, repeat_penalty=0.9, seed=8),
    SamplingParams(2.0, top_k=1, seed=9),
    SamplingParams(**QWEN3_DEFAULT),                                     # the default seed
]
LENS = [1, 63, 64, 65, 130, 7, 20, 3, 64, 2, 41, 90]


def replay(params, prompt_toks, step_logits, V):
    """generate_generic's sampler on the reported step logits, in the oracle restatement; one RNG stream per sequence."""
    s = osamp.get_logit_processor(params.temperature, params.top_p, params.top_k)
    rng = ornd.StdRng.seed_from_u64(params.seed)
    pen_v = 1.0 if params.repeat_penalty is None else params.repeat_penalty
    out = []
    for t in range(len(prompt_toks)):
        pen = osamp.use_repeat_penalty(pen_v, params.repeat_last_n, step_logits[t], out)
        if s.kind == "ArgMax":
            tok = int(np.argmax(pen))
        else:
            w = osamp.final_weights(pen, s)
            if s.kind in ("TopK", "TopKThenTopP") and s.k < V:
                prs = osamp.softmax_last_dim(pen * np.float32(1.0 / s.temperature))
                keep = osamp.topk_order(prs, pen)[: s.k]
                tok = int(keep[ornd.sample_multinomial(rng, w[keep])])
            else:
                tok = ornd.sample_multinomial(rng, w)
        out.append(tok)
    return out


def test_generate_batch_sampled_exact_replay(rand_model):
    cfg, m = rand_model
    V = cfg.vocab_size
    prompts = prompts_for(len(MIXED), 51, V, LENS)
    toks, step = m.generate_batch_sampled(prompts, MIXED, 24, want_step_logits=True)
    assert m.cache_len() == 0
    for j, p in enumerate(MIXED):
        assert len(toks[j]) == 24, j
        assert replay(p, toks[j], step[j], V) == toks[j], f"sequence {j} ({p}) differs from the oracle replay"


def test_generate_batch_sampled_all_greedy_equals_generate_batch(rand_model):
    cfg, m = rand_model
    prompts = prompts_for(17, 52, cfg.vocab_size, [1, 63, 64, 65, 300, 7])
    greedy = [SamplingParams(), SamplingParams(0.0, 0.9, 20, seed=3), SamplingParams(-1.0, top_k=5), SamplingParams(1e-8)]
    params = [greedy[j % len(greedy)] for j in range(len(prompts))]
    want, wl = m.generate_batch(prompts, 20, want_logits=True)
    m.set_profiling(True)
    got, step = m.generate_batch_sampled(prompts, params, 20, want_step_logits=True)
    prof = m.get_profile("sample_rows_stage1")
    m.set_profiling(False)
    assert prof["launches"] == 0, prof   # no row samples: the device argmax decides every token
    assert got == want
    for j in range(len(prompts)):
        assert np.array_equal(bits(step[j, len(got[j]) - 1]), bits(wl[j])), j


def test_generate_batch_sampled_isolation_and_seeds(rand_model):
    """One prefill pass per prompt (max_tokens_per_pass=1): the packed prefill GEMM's plan depends on the pass's total rows, so a
    prompt packed with others differs in the last bf16 bits from the same prompt alone -- aha_hip_generate_batch does the same.  With
    the passes fixed, the decode steps, the candidate step and each sequence's sampler must not depend on the batch."""
    cfg, m = rand_model
    V = cfg.vocab_size
    prompts = prompts_for(len(MIXED), 53, V, LENS)
    base, bl = m.generate_batch_sampled(prompts, MIXED, 16, max_tokens_per_pass=1, want_step_logits=True)
    for j in range(len(prompts)):   # alone
        alone, al = m.generate_batch_sampled([prompts[j]], [MIXED[j]], 16, max_tokens_per_pass=1, want_step_logits=True)
        assert alone[0] == base[j], j
        assert np.array_equal(bits(al[0]), bits(bl[j])), j
    perm = np.random.default_rng(54).permutation(len(prompts))
    pg, pl = m.generate_batch_sampled([prompts[i] for i in perm], [MIXED[i] for i in perm], 16, max_tokens_per_pass=1,
                                      want_step_logits=True)
    for k, i in enumerate(perm):
        assert pg[k] == base[i], i
        assert np.array_equal(bits(pl[k]), bits(bl[i])), i
    # the same prompt and seed twice in one batch: the same tokens; a different seed moves a high-temperature row
    hot = SamplingParams(5.0, seed=11)
    twice = m.generate_batch_sampled([prompts[4], prompts[4], prompts[4]], [hot, hot, SamplingParams(5.0, seed=12)], 16)
    assert twice[0] == twice[1] and twice[2] != twice[0]
    assert m.cache_len() == 0


@pytest.fixture(scope="module")
def tied(gpu):
    from aha_amd.model import HipInferenceModel
    cfg = tiny_qwen3(layers=3, hidden=512, heads=4, kv_heads=2, inter=1024, vocab=2048, tie=True)
    w = qwen3_text_weights(cfg, seed=0)
    decisive.make_tied_decisive(w, "model.embed_tokens.weight", "model.norm.weight", scale=32.0, seed=7, n_text=2000)
    m = HipInferenceModel(cfg, w)
    yield cfg, w, m
    m.close()


def test_generate_batch_sampled_agrees_with_the_single_sequence_path(tied):
    from aha_amd import sampling as hs
    cfg, w, m = tied
    prompts = prompts_for(9, 55, 2000, [1, 63, 64, 65, 300, 7])
    params = [SamplingParams(**QWEN3_DEFAULT, seed=j) if j % 2 else SamplingParams(**QWEN3_DEFAULT, repeat_penalty=1.1, seed=j)
              for j in range(len(prompts))]
    got = m.generate_batch_sampled(prompts, params, 40)
    for j, p in enumerate(prompts):
        alone = hs.generate_generic_sampled(m, p, params[j].context(len(p), 40))
        assert got[j] == alone, j
    assert m.cache_len() == 0


def test_generate_batch_sampled_stops_state_and_launches(tied):
    from aha_amd.model import HipInferenceModel
    cfg, w, m = tied
    a = 600
    cfg2 = tiny_qwen3(layers=3, hidden=512, heads=4, kv_heads=2, inter=1024, vocab=2048, tie=True)
    cfg2.eos_token_ids = [a]
    m2 = HipInferenceModel(cfg2, w)
    try:
        got = m2.generate_batch_sampled([[5, 9, a], [11, a ^ 1], [40, 41, 42, 43]], SamplingParams(**QWEN3_DEFAULT), 9)
    finally:
        m2.close()
    assert got[0] == [a ^ 1, a]                # the second token is the stop token: kept, and the sequence ends
    assert got[1] == [a, a ^ 1, a]             # a first token equal to the stop token does not stop
    assert got[2] == [42, 43] * 4 + [42]
    prompts = prompts_for(5, 56, 2000, [3, 70, 9])
    params = [SamplingParams()] * 4 + [SamplingParams(**QWEN3_DEFAULT)]
    m.set_profiling(False)
    m.set_profiling(True)
    m.generate_batch_sampled(prompts, params, 12)
    launches = {s: m.get_profile(f"sample_rows_stage{s}")["launches"] for s in ("1", "2a", "2b")}
    m.set_profiling(False)
    assert launches == {"1": 12, "2a": 12, "2b": 12}, launches   # once for the first token, once per decode step: not per row
    assert m.cache_len() == 0
    for bad in ([[1, 2], []], [[1, 2], [3, 5000]]):
        with pytest.raises(AhaHipError):
            m.generate_batch_sampled(bad, SamplingParams(**QWEN3_DEFAULT), 4)
        assert m.cache_len() == 0
    with pytest.raises(AhaHipError):
        m.generate_batch_sampled([[1, 2]], [SamplingParams(0.7, top_k=0, seed=1)], 4)
    assert m.cache_len() == 0
    assert m.generate_batch_sampled(prompts[:2], SamplingParams(**QWEN3_DEFAULT), 4) == [[p[-1] ^ 1, p[-1]] * 2 for p in prompts[:2]]
