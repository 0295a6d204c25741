"""-m gpu: per-token log-probabilities (aha_hip_logprob_rows, aha_hip_generate_batch_logprobs, aha_hip_engine_*_logprobs).

The reference is numpy in f64 on the very logits the library reports: lp = (x - max x) - log sum exp(x - max x), the top-N ids in numpy's
stable descending order (value descending, index ascending).  Ids must match exactly.  Values must be within 2^-14 (6.1e-5) absolute of
the f64 value: for |lp| <= 128 the f32 chain contributes half an ulp at 32 for x - M (2e-6), about 2e-6 for the tree sum of <= 151 936
terms in [0, 1], half an ulp at 64 for the last subtraction (4e-6); a CPU emulation of the two-stage sum on these input classes gave at
most 3.7e-6, so the bound leaves about 16x for the hardware exp / log.  The measured maximum is printed (run with -s).

  1. op level: V from 1 to the real vocabulary around every boundary of the pass (fewer entries than N, N itself, one stage-1 wave and
     its boundary, many waves), R = 1 / 7 / 33 / 64, a row pitch above V, per-row n_top 0 / 1 / 5 / 20, tokens at the arg-max, the
     arg-min and at random, rows of bf16-rounded normals of four widths, all-equal rows, small-integer rows (order by index alone), rows
     with -inf entries; the logits are only read;
  2. generation on the three tiny random-weight models of test_generate_sampled_gpu.py with its MIXED samplers: tokens and step logits
     are generate_batch_mm's bit for bit, every entry follows the f64 reference of its own step logits (rows with a repeat penalty and
     rows that fall back to the full vector included), one launch of each stage per step with a logprob row, none otherwise;
  3. a sequence's entries do not depend on the batch; 4. an image request; 5. the engine; 6. argument errors.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from aha_amd import _lib
from aha_amd._lib import AhaHipError
from aha_amd.configs import tiny_qwen3, tiny_qwen3vl
from aha_amd.sampling import SamplingParams
from aha_amd.weights import qwen3_text_weights, qwen3vl_weights

pytestmark = pytest.mark.gpu

TOL = 2.0 ** -14
NO_ID = 0xFFFFFFFF
WORST = {"err": 0.0}
QWEN3_DEFAULT = dict(temperature=0.6, top_p=0.95, top_k=20)
# the sampler list and prompt lengths of tests/test_generate_sampled_gpu.py
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
TOPS = [None, 0, 1, 5, 20]
MAX_NEW = 12


def bits(x):
    return np.asarray(x, dtype=np.float32).view(np.uint32)


def prompts_for(n, seed, vocab, lens):
    g = np.random.default_rng(seed)
    return [[int(x) for x in g.integers(0, vocab, size=lens[i % len(lens)])] for i in range(n)]


def reference(x):
    """f64 log-softmax of one row of f32 logits and its ids in (value descending, index ascending) order."""
    x64 = np.asarray(x, dtype=np.float32).astype(np.float64)
    m = x64.max()
    with np.errstate(divide="ignore"):
        lp = (x64 - m) - np.log(np.exp(x64 - m).sum())
    return lp, np.argsort(-x64, kind="stable")


def check_values(got, want, what):
    got, want = np.asarray(got, dtype=np.float64).reshape(-1), np.asarray(want, dtype=np.float64).reshape(-1)
    inf = np.isneginf(want)
    assert np.array_equal(np.isneginf(got), inf), (what, got, want)
    assert np.isfinite(got[~inf]).all(), (what, got)
    if (~inf).any():
        err = float(np.abs(got[~inf] - want[~inf]).max())
        WORST["err"] = max(WORST["err"], err)
        assert err <= TOL, (what, err, got, want)


def check_entry(x, tok, n, logprob, ids, lps, what):
    """One aha_token_logprobs (logprob, the first n ids / lps) against the f64 reference of its logits row x."""
    lp, order = reference(x)
    V = len(lp)
    k = min(n, V)
    assert [int(i) for i in ids[:k]] == [int(i) for i in order[:k]], (what, list(ids[:n]), list(order[:k]))
    assert all(int(i) == NO_ID for i in ids[k:n]), (what, list(ids[:n]))
    check_values(lps[:k], lp[order[:k]], what)
    assert all(np.isneginf(v) for v in lps[k:n]), (what, list(lps[:n]))
    check_values([logprob], [lp[tok]], what)


# ---- 1. the op ------------------------------------------------------------------------------------------------------------------------
def make_rows(R, V, seed):
    g = torch.Generator().manual_seed(seed)
    rows = []
    for r in range(R):
        kind = r % 7
        if kind < 4:
            x = (torch.randn(V, generator=g) * (0.02, 1.0, 4.0, 12.0)[kind]).bfloat16().float()
        elif kind == 4:
            x = torch.full((V,), (-1.5, 0.0, 7.25)[(r // 7) % 3])
        elif kind == 5:
            x = torch.randint(-3, 4, (V,), generator=g).float()
        else:   # a few -inf entries, a finite maximum
            x = torch.randn(V, generator=g).bfloat16().float()
            n_inf = min(max(V - 1, 0), 3)
            if n_inf:
                x[torch.randperm(V, generator=g)[:n_inf]] = float("-inf")
        rows.append(x)
    return torch.stack(rows)


@pytest.mark.parametrize("V", [1, 19, 20, 21, 300, 511, 512, 513, 4096, 151936])
def test_logprob_rows_against_f64(gpu, V):
    from aha_amd import ops
    R_ALL, PAD = 64, 5
    host = make_rows(R_ALL, V, 100 + V % 97)
    g = np.random.default_rng(V)
    n_top = np.asarray([(0, 1, 5, 20)[(r // 2) % 4] for r in range(R_ALL)], dtype=np.int32)
    refs = [reference(host[r].numpy()) for r in range(R_ALL)]
    tokens = np.zeros(R_ALL, dtype=np.int64)
    for r in range(R_ALL):
        x = host[r].numpy()
        tokens[r] = (int(np.argmax(x)), int(np.argmin(x)), int(g.integers(0, V)))[r % 3]
    # a row pitch above V; the padding holds huge values a read past V would pick up
    dev = torch.full((R_ALL, V + PAD), 3.0e38, dtype=torch.float32)
    dev[:, :V] = host
    dev = dev.cuda()
    before = dev.clone()
    for R in (1, 7, 33, 64):
        sel = list(range(R)) if R != 7 else [6, 13, 4, 5, 27, 62, 0]   # (a -inf row, an all-equal row and an integer row among the 7)
        lg = dev[sel][:, :V] if R != 64 else dev[:, :V]
        assert lg.stride(0) == V + PAD
        keep = lg.clone()
        lp, nt, ids, lps = ops.logprob_rows(lg, tokens[sel], n_top[sel])
        torch.cuda.synchronize()
        assert torch.equal(lg.view(torch.int32), keep.view(torch.int32)), "logprob_rows wrote its input logits"
        assert np.array_equal(nt, n_top[sel])
        for s, r in enumerate(sel):
            what = (V, R, r)
            want_lp, order = refs[r]
            n, k = int(n_top[r]), min(int(n_top[r]), V)
            assert np.array_equal(ids[s, :k], order[:k].astype(np.uint32)), (what, ids[s, :n], order[:k])
            assert (ids[s, k:n] == NO_ID).all(), what
            check_values(lps[s, :k], want_lp[order[:k]], what)
            assert np.isneginf(lps[s, k:n]).all(), what
            check_values([lp[s]], [want_lp[tokens[r]]], what)
    assert torch.equal(dev.view(torch.int32), before.view(torch.int32))
    print(f"\nlogprob_rows V={V}: max |error| so far {WORST['err']:.3e} (bound {TOL:.3e})")


def test_logprob_rows_inf_entries_reach_the_list_in_index_order(gpu):
    """V = 21, N = 20: the -inf entries are part of the top 20, in index order, with logprob -inf; as the token too."""
    from aha_amd import ops
    x = torch.arange(21, dtype=torch.float32) * 0.25
    x[[3, 11, 12]] = float("-inf")
    lp, nt, ids, lps = ops.logprob_rows(x.reshape(1, 21).cuda(), [11], 20)
    want = [i for i in range(20, -1, -1) if i not in (3, 11, 12)] + [3, 11]
    assert ids[0].tolist() == want
    assert np.isneginf(lps[0, 18:]).all() and np.isfinite(lps[0, :18]).all() and np.isneginf(lp[0])
    check_entry(x.numpy(), 11, 20, lp[0], ids[0], lps[0], "inf")


# ---- 2. generation --------------------------------------------------------------------------------------------------------------------
class Models:
    """The three tiny random-weight models of tests/test_generate_sampled_gpu.py's rand_model, each built when first asked for."""

    def __init__(self):
        self.built = {}

    def get(self, name):
        from aha_amd.model import HipInferenceModel
        if name not in self.built:
            if name == "narrow":
                cfg = tiny_qwen3(layers=3, hidden=512, heads=4, kv_heads=2, inter=1024, vocab=4096)
                m = HipInferenceModel(cfg, qwen3_text_weights(cfg, seed=0))
            elif name == "wide":
                cfg = tiny_qwen3(layers=2, hidden=1024, heads=16, kv_heads=8, inter=3072, vocab=4096)
                m = HipInferenceModel(cfg, qwen3_text_weights(cfg, seed=0))
                m.debug_scramble_pages(True)
            else:
                cfg = tiny_qwen3vl()
                m = HipInferenceModel(cfg, qwen3vl_weights(cfg, seed=0))
            self.built[name] = m
        return name, self.built[name].text_cfg, self.built[name]


@pytest.fixture(scope="module")
def models(gpu):
    ms = Models()
    yield ms
    for m in ms.built.values():
        m.close()


ALL_MODELS = pytest.mark.parametrize("which", ["narrow", "wide", "vl"])


STAGES = ("sample_rows_stage1", "sample_rows_stage2a", "sample_rows_stage2b", "logprob_rows_stage1", "logprob_rows_stage2")


def profiled(m, call):
    m.set_profiling(False)
    m.set_profiling(True)
    res = call()
    launches = {s: m.get_profile(s)["launches"] for s in STAGES}
    m.set_profiling(False)
    return res, launches


def check_sequences(toks, lps, step, tops, what):
    for j, top in enumerate(tops):
        if top is None:
            assert lps[j] is None, (what, j)
            continue
        assert len(lps[j]) == len(toks[j]), (what, j)
        for t, tok in enumerate(toks[j]):
            logprob, alts = lps[j][t]
            assert len(alts) == top, (what, j, t)
            check_entry(step[j, t], tok, top, logprob, [a[0] for a in alts], [a[1] for a in alts], (what, j, t))


@ALL_MODELS
def test_generate_batch_logprobs_matches_mm_and_f64(models, which):
    name, cfg, m = models.get(which)
    V = cfg.vocab_size
    prompts = prompts_for(len(MIXED), 51, V, LENS)
    tops = [TOPS[j % len(TOPS)] for j in range(len(prompts))]
    (want, wstep), base = profiled(m, lambda: m.generate_batch_mm(prompts, None, MAX_NEW, params=MIXED, want_step_logits=True))
    (toks, lps, step), prof = profiled(m, lambda: m.generate_batch_logprobs(prompts, MAX_NEW, tops, params=MIXED, want_step_logits=True))
    assert m.cache_len() == 0
    assert toks == want
    assert np.array_equal(bits(step), bits(wstep))
    check_sequences(toks, lps, step, tops, name)
    steps = sum(1 for t in range(MAX_NEW) if any(top is not None and len(toks[j]) > t for j, top in enumerate(tops)))
    assert prof["logprob_rows_stage1"] == steps and prof["logprob_rows_stage2"] == steps, (prof, steps)
    assert base["logprob_rows_stage1"] == 0 and base["logprob_rows_stage2"] == 0, base
    for s in STAGES[:3]:
        assert prof[s] == base[s], (s, prof, base)
    # no sequence asks: neither stage runs, every entry says so, the tokens stay
    (toks0, lps0), prof0 = profiled(m, lambda: m.generate_batch_logprobs(prompts, MAX_NEW, None, params=MIXED))
    assert toks0 == want and lps0 == [None] * len(prompts)
    assert prof0["logprob_rows_stage1"] == 0 and prof0["logprob_rows_stage2"] == 0, prof0
    for s in STAGES[:3]:
        assert prof0[s] == base[s], (s, prof0, base)
    # greedy (params None) with one top_logprobs for all
    gw, gstep_w = m.generate_batch_mm(prompts[:5], None, 6, want_step_logits=True)
    gt, glp, gstep = m.generate_batch_logprobs(prompts[:5], 6, 20, want_step_logits=True)
    assert gt == gw and np.array_equal(bits(gstep), bits(gstep_w))
    check_sequences(gt, glp, gstep, [20] * 5, name + " greedy")
    print(f"\ngenerate_batch_logprobs {name}: max |error| so far {WORST['err']:.3e} (bound {TOL:.3e})")


def test_none_entries_carry_n_top_minus_one(models):
    """Through the C ABI: a sequence with -1 gets n_top = -1 in its n_out entries and nothing else; entries past n_out[j] are untouched."""
    name, cfg, m = models.get("narrow")
    prompts = prompts_for(3, 57, cfg.vocab_size, [5, 70, 9])
    ids = np.ascontiguousarray(np.concatenate([np.asarray(p, dtype=np.uint32) for p in prompts]))
    lens = np.asarray([len(p) for p in prompts], dtype=np.uint64)
    top = np.asarray([-1, 3, -1], dtype=np.int32)
    max_new, fill = 3, 0xABABABAB
    toks, n_out = np.zeros((3, max_new), np.uint32), np.zeros(3, np.uint64)
    lp = (_lib.TokenLogprobs * (3 * max_new + 2))()
    raw = np.frombuffer(lp, dtype=np.uint32).reshape(3 * max_new + 2, 42)
    raw[:] = fill
    _lib.check(_lib.lib().aha_hip_generate_batch_logprobs(m.handle, ids.ctypes.data, lens.ctypes.data, 3, None, None, top.ctypes.data, max_new,
                                                          0, toks.ctypes.data, n_out.ctypes.data, None, lp))
    assert n_out.tolist() == [3, 3, 3]
    for j in range(3):
        for t in range(max_new):
            e = raw[j * max_new + t]
            if top[j] < 0:
                assert int(e[1:2].view(np.int32)[0]) == -1 and (np.delete(e, 1) == fill).all(), (j, t)
            else:
                assert int(e[1:2].view(np.int32)[0]) == 3 and (e[2:5] == fill).sum() == 0, (j, t)
    assert (raw[3 * max_new:] == fill).all()
    # a second call with max_new 1 into the same buffer: entry [j, 0] lives at j, everything behind the three stays untouched
    raw[:] = fill
    _lib.check(_lib.lib().aha_hip_generate_batch_logprobs(m.handle, ids.ctypes.data, lens.ctypes.data, 3, None, None, top.ctypes.data, 1, 0,
                                                          toks.ctypes.data, n_out.ctypes.data, None, lp))
    assert n_out.tolist() == [1, 1, 1] and (raw[3:] == fill).all() and int(raw[1, 1:2].view(np.int32)[0]) == 3


# ---- 3. independence from the batch ---------------------------------------------------------------------------------------------------
@ALL_MODELS
def test_logprobs_do_not_depend_on_the_batch(models, which):
    """One prefill pass per prompt (max_tokens_per_pass=1), as test_generate_sampled_gpu.py's isolation test: the logits are then the same
    bits alone and in the batch, and each row's pass reads its own row only."""
    name, cfg, m = models.get(which)
    prompts = prompts_for(len(MIXED), 53, cfg.vocab_size, LENS)
    tops = [TOPS[(j + 1) % len(TOPS)] for j in range(len(prompts))]
    base, blp = m.generate_batch_logprobs(prompts, MAX_NEW, tops, params=MIXED, max_tokens_per_pass=1)
    for j in range(len(prompts)):
        alone, alp = m.generate_batch_logprobs([prompts[j]], MAX_NEW, [tops[j]], params=[MIXED[j]], max_tokens_per_pass=1)
        assert alone[0] == base[j], j
        if tops[j] is None:
            assert alp[0] is None and blp[j] is None
            continue
        for t in range(len(alone[0])):
            a, b = alp[0][t], blp[j][t]
            assert bits(a[0]) == bits(b[0]), (j, t, a[0], b[0])
            assert [i for i, _ in a[1]] == [i for i, _ in b[1]], (j, t)
            assert np.array_equal(bits([v for _, v in a[1]]), bits([v for _, v in b[1]])), (j, t)


# ---- 4. an image request --------------------------------------------------------------------------------------------------------------
def test_image_request_logprobs(models):
    name, cfg, m = models.get("vl")
    from aha_amd.model import MultiModalData
    from aha_amd.vision_host import image_prompt_ids
    from oracle import qwen3vl as ov
    from oracle.numerics import Numerics
    full = tiny_qwen3vl()
    g = np.random.default_rng(2)
    ids = [int(x) for x in g.integers(0, 1900, size=3)]
    pv, grid = ov.process_images(Numerics("bf16", matmul_f64=True), [g.integers(0, 256, size=(64, 96, 3), dtype=np.uint8)])
    ids = image_prompt_ids(full, grid, ids, [int(x) for x in g.integers(0, 1900, size=2)]) + [int(x) for x in g.integers(0, 1900, size=9)]
    data = [MultiModalData(pv.to(torch.bfloat16), grid)]
    want, wstep = m.generate_batch_mm([ids], data, 8, want_step_logits=True)
    toks, lps, step = m.generate_batch_logprobs([ids], 8, 5, data=data, want_step_logits=True)
    assert toks == want and np.array_equal(bits(step), bits(wstep))
    check_sequences(toks, lps, step, [5], "image")


# ---- 5. the engine --------------------------------------------------------------------------------------------------------------------
def drive_engine(m, reqs, lp_submit, lp_step, cancel=(2, 4), steps_max=64):
    """reqs[i] = (ids, max_new, params, top_logprobs) submitted before step i // 2; request cancel[0] is cancelled before step cancel[1].
    Returns the events per step as tuples, their logits rows and (with lp_step) their logprob entries."""
    from aha_amd.model import HipEngine
    eng = HipEngine(m, max_running=4, kv_pages=64)
    try:
        rid, evs_all, lg_all, lp_all = {}, [], [], []
        for step in range(steps_max):
            for i, (ids, max_new, params, top) in enumerate(reqs):
                if i // 2 == step:
                    rid[i] = eng.submit(ids, max_new, params, top_logprobs=top if lp_submit else None)
            if step == cancel[1]:
                eng.cancel(rid[cancel[0]])
            if lp_step:
                evs, lg, lps = eng.step(want_logits=True, want_logprobs=True)
            else:
                evs, lg = eng.step(want_logits=True)
                lps = [None] * len(evs)
            for k, ev in enumerate(evs):
                evs_all.append((step, ev.req_id, ev.token, ev.first, ev.stop, ev.length, ev.cancelled))
                lg_all.append(None if ev.cancelled else lg[k].copy())
                lp_all.append(lps[k])
            st = eng.stats()
            if step >= len(reqs) // 2 and st["running"] == 0 and st["waiting"] == 0:
                break
        return rid, evs_all, lg_all, lp_all
    finally:
        eng.close()


def test_engine_logprobs(models):
    name, cfg, m = models.get("narrow")
    ps = prompts_for(6, 61, cfg.vocab_size, [70, 9, 33, 64, 5, 20])
    pen = SamplingParams(**QWEN3_DEFAULT, repeat_penalty=1.3, repeat_last_n=6, seed=3)
    reqs = [(ps[0], 9, None, 20), (ps[1], 7, None, None), (ps[2], 12, pen, 0), (ps[3], 8, SamplingParams(1.2, seed=6), None),
            (ps[4], 6, SamplingParams(1.0, top_k=100, seed=7), 20), (ps[5], 5, pen, None)]
    rid, evs, lg, lps = drive_engine(m, reqs, True, True)
    top_of = {rid[i]: reqs[i][3] for i in rid}
    assert any(e[6] for e in evs) and sum(1 for e in evs if e[3]) == 6
    seen = {r: 0 for r in top_of}
    n_tok = {r: sum(1 for e in evs if e[1] == r and not e[6]) for r in top_of}
    for e, row, entry in zip(evs, lg, lps):
        top = top_of[e[1]]
        if e[6] or top is None:
            assert entry is None, e     # n_top = -1: a cancellation, or a request of the plain submit
            continue
        logprob, alts = entry
        assert len(alts) == top, e
        check_entry(row, e[2], top, logprob, [a[0] for a in alts], [a[1] for a in alts], e)
        seen[e[1]] += 1
    assert seen[rid[0]] == n_tok[rid[0]] == 9 and seen[rid[4]] == n_tok[rid[4]] == 6
    assert 0 < seen[rid[2]] == n_tok[rid[2]] < 12   # request 2 was cancelled mid-way
    # the same submissions through aha_hip_engine_step, and the plain submissions: the same events, tokens and logits
    for lp_submit in (True, False):
        _, evs2, lg2, _ = drive_engine(m, reqs, lp_submit, False)
        assert evs2 == evs, lp_submit
        for a, b in zip(lg, lg2):
            assert (a is None and b is None) or np.array_equal(bits(a), bits(b)), lp_submit
    print(f"\nengine: max |error| so far {WORST['err']:.3e} (bound {TOL:.3e})")


# ---- 6. argument errors ---------------------------------------------------------------------------------------------------------------
def test_logprob_argument_errors(models):
    name, cfg, m = models.get("narrow")
    from aha_amd.model import HipEngine
    prompts = prompts_for(3, 58, cfg.vocab_size, [5, 9, 3])
    for bad in (21, -2):
        with pytest.raises(AhaHipError, match=r"top_logprobs of sequence 1 .*%d" % bad) as ei:
            m.generate_batch_logprobs(prompts, 4, [5, bad, None])
        assert ei.value.code == -1
        assert m.cache_len() == 0
    ids = np.ascontiguousarray(np.concatenate([np.asarray(p, dtype=np.uint32) for p in prompts]))
    lens = np.asarray([len(p) for p in prompts], dtype=np.uint64)
    top = np.asarray([5, 5, 5], dtype=np.int32)
    toks, n_out = np.zeros((3, 4), np.uint32), np.zeros(3, np.uint64)
    rc = _lib.lib().aha_hip_generate_batch_logprobs(m.handle, ids.ctypes.data, lens.ctypes.data, 3, None, None, top.ctypes.data, 4, 0,
                                                    toks.ctypes.data, n_out.ctypes.data, None, None)
    assert rc == -1 and b"logprobs_out" in _lib.lib().aha_hip_last_error()
    assert m.cache_len() == 0
    with pytest.raises(AhaHipError):   # generate_batch_mm's own checks still hold
        m.generate_batch_logprobs([[1, 2], []], 4, 5)
    assert m.cache_len() == 0
    eng = HipEngine(m, max_running=2, kv_pages=8)
    try:
        with pytest.raises(AhaHipError, match="top_logprobs must be 0 .. 20, got 21") as ei:
            eng.submit(prompts[0], 4, top_logprobs=21)
        assert ei.value.code == -1
        assert eng.stats()["waiting"] == 0
    finally:
        eng.close()
    assert m.cache_len() == 0
    assert m.generate_batch_logprobs(prompts, 4, 5)[0] == m.generate_batch_mm(prompts, None, 4)
    assert C.sizeof(_lib.TokenLogprobs) == 168
