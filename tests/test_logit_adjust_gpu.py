"""-m gpu: logit_bias, presence_penalty and frequency_penalty (aha_logit_adjust) on the device -- aha_hip_sample_rows_adjusted,
aha_hip_generate_batch_adjusted, aha_hip_engine_submit_adjusted.

The definition (include/aha_hip.h), restated in numpy wherever a reference is needed: y = the step's f32 logits after the repeat penalty;
for every id with a non-zero bias b_i or a count c_i > 0 over ALL generated tokens a_i = f32(f64(b_i) - f64(frequency) * c_i -
f64(presence)); z_i = y_i + a_i, one f32 add; the request's sampler runs on z; logprobs stay those of the raw logits.

  1. the op against numpy: z built in f32, a stable descending sort; idx and the bits of vals and max equal, sumexp within 2e-5 relative
     of the f64 sum over z (the bound of tests/test_sampling_gpu.py::check_candidates) and finite; rows without addends bit-identical to
     ops.sample_rows; the logits only read;
  2. generation: every token equals the oracle replay of steps 1-4 on the reported step logits, and every sequence with an active adjust
     differs from the same call without it;
  3. properties that need no replay; 4. logprobs with an adjust; 5. isolation from the batch; 6. the engine; 7. argument errors.
"""
import numpy as np
import pytest
import torch

from aha_amd._lib import AhaHipError
from aha_amd.sampling import SamplingParams
from oracle import rand_stdrng as ornd
from oracle import sampling as osamp

from test_generate_sampled_gpu import LENS, MIXED, QWEN3_DEFAULT
from test_logit_adjust_cpu import addends
from test_logprobs_gpu import STAGES, Models, bits, check_sequences, make_rows, profiled, prompts_for

pytestmark = pytest.mark.gpu
NINF = float("-inf")
MAX_NEW = 24


# ---- 1. the op ------------------------------------------------------------------------------------------------------------------------
N_FORMS = 9


def make_adjust_list(form, y, V, k, ctx, g):
    """One row's (ids, addends) of form `form`; y: the row's penalised logits."""
    finite = np.isfinite(y)
    if form == 0 or not finite.any():
        return [], []
    if form == 1:
        return [int(g.integers(0, V))], [float(g.normal(0, 3))]
    if form == 2:                                                   # exactly at the wave boundaries and the ends
        ids = sorted({i for i in (0, 511, 512, V - 1) if i < V})
        return ids, [float(v) for v in g.normal(0, 4, len(ids))]
    if form == 3:                                                   # a whole stage-1 wave at -inf (V <= 512: the first half of the row)
        ids = list(range(512, min(1024, V))) if V > 512 else list(range(0, V // 2))
        return ids, [NINF] * len(ids)
    if form in (4, 5):                                              # 1024 entries spread over V / 4096 and more (or every id of a small V)
        n = min(V, 1024 if form == 4 else 4096 + 37)
        ids = np.sort(g.choice(V, size=n, replace=False))
        return [int(i) for i in ids][::-1], [float(v) for v in g.normal(0, 2, n)]   # (handed over in descending order: any order is allowed)
    if form == 6:                                                   # lifts the arg-min to the top
        lo = int(np.argmin(np.where(finite, y, np.inf)))
        return [lo], [float(y[finite].max() - y[lo]) + 1.0]
    if form == 7:                                                   # on an id that also takes the repeat penalty
        inside = [c for c in ctx if c < V]
        return ([inside[0]], [2.5]) if inside else ([], [])
    top = np.argsort(-y, kind="stable")[:k]                         # -inf on every other one of the would-be top k
    ids = sorted(int(i) for i in top[::2][: max(1, V - 1)]) if V > 1 else []
    return ids, [NINF] * len(ids)


def op_reference(x, k, temp, pen, ctx, ids, vals):
    y = osamp.apply_repeat_penalty(x, pen, ctx) if pen != 1.0 else x.copy()
    z = np.asarray(y, dtype=np.float32).copy()
    if len(ids):
        i = np.asarray(ids, dtype=np.int64)
        z[i] = z[i] + np.asarray(vals, dtype=np.float32)           # one f32 add per listed id
    order = np.argsort(-z, kind="stable")[:k]
    inv_t = np.float32(1.0 / temp) if temp > 0 else np.float32(1.0)
    mx = z.max()
    se = np.exp((z.astype(np.float64) - float(mx)) * float(inv_t)).sum()
    return z[order], order.astype(np.uint32), np.float32(mx), se


@pytest.mark.parametrize("V", [1, 511, 512, 513, 1536, 4096, 151936])
def test_sample_rows_adjusted_against_numpy(gpu, V):
    from aha_amd import ops
    R_ALL, PAD = 64, 5
    host = make_rows(R_ALL, V, 300 + V % 89).numpy()
    g = np.random.default_rng(1000 + V)
    rows = []
    for r in range(R_ALL):
        form = r % N_FORMS
        k = min(V, int(g.choice([1, 2, 20, 63, 64])) if r % 3 else int(g.integers(1, 65)))
        temp = float(g.choice([0.0, 0.6, 1.3, 7.0]))
        pen = 1.3 if form == 7 else float(g.choice([1.0, 1.2, 0.9]))
        ctx = [int(c) for c in g.integers(0, min(V, 64), size=int(g.integers(1 if form == 7 else 0, 30)))]
        if r % 5 == 0:
            ctx += [V + 3]
        y = osamp.apply_repeat_penalty(host[r], pen, ctx) if pen != 1.0 else host[r]
        ids, vals = make_adjust_list(form, y, V, k, ctx, g)
        rows.append((k, temp, pen, ctx, ids, vals, op_reference(host[r], k, temp, pen, ctx, ids, vals)))
    if V == 1536:
        assert any(r[4] == list(range(512, 1024)) for r in rows)
    dev = torch.full((R_ALL, V + PAD), 3.0e38, dtype=torch.float32)   # a row pitch above V; a read past V would pick the padding up
    dev[:, :V] = torch.from_numpy(host)
    dev = dev.cuda()
    before = dev.clone()
    worst = 0.0
    for R in (1, 7, 33, 64):
        sel = list(range(R)) if R != 7 else [6, 13, 3, 5, 26, 62, 0]
        lg = dev[sel][:, :V] if R != 64 else dev[:, :V]
        assert lg.stride(0) == V + PAD
        args = ([rows[i][0] for i in sel], [rows[i][1] for i in sel], [rows[i][2] for i in sel], [rows[i][3] for i in sel])
        vals, idx, ms = ops.sample_rows_adjusted(lg, *args, [(rows[i][4], rows[i][5]) for i in sel])
        pv, pi, pm = ops.sample_rows(lg.contiguous(), *args)
        torch.cuda.synchronize()
        vals, idx, ms = vals.cpu().numpy(), idx.cpu().numpy().view(np.uint32), ms.cpu().numpy()
        pv, pi, pm = pv.cpu().numpy(), pi.cpu().numpy().view(np.uint32), pm.cpu().numpy()
        for s, i in enumerate(sel):
            k, _, _, _, ids, _, (wv, wi, wm, wse) = rows[i]
            what = (V, R, i, i % N_FORMS)
            assert np.array_equal(idx[s, :k], wi), (what, idx[s, :k], wi)
            assert np.array_equal(bits(vals[s, :k]), bits(wv)), what
            assert bits(ms[s, 0]) == bits(wm), (what, ms[s, 0], wm)
            assert np.isfinite(ms[s, 1]), (what, ms[s])
            rel = abs(float(ms[s, 1]) - wse) / wse
            worst = max(worst, rel)
            assert rel <= 2e-5, (what, ms[s, 1], wse)
            if not ids:   # no addends: what sample_rows gives, bit for bit
                assert np.array_equal(bits(vals[s, :k]), bits(pv[s, :k])) and np.array_equal(idx[s, :k], pi[s, :k]), what
                assert np.array_equal(bits(ms[s]), bits(pm[s])), what
    assert torch.equal(dev.view(torch.int32), before.view(torch.int32)), "sample_rows_adjusted wrote its input logits"
    print(f"\nsample_rows_adjusted V={V}: max relative sumexp error {worst:.3e} (bound 2e-5)")


def test_sample_rows_adjusted_argument_errors(gpu):
    from aha_amd import ops
    lg = torch.zeros(2, 600, device="cuda")   # (a device pointer only: the checks come before any launch)
    for bad in ([([600], [1.0]), ([], [])], [([3, 3], [1.0, 2.0]), ([], [])], [([], []), ([5], [float("nan")])], [([5], [float("inf")]), ([], [])]):
        with pytest.raises(AhaHipError, match="sample_rows_adjusted: row"):
            ops.sample_rows_adjusted(lg, [1, 1], [0.0, 0.0], [1.0, 1.0], [[], []], bad)


# ---- 2. generation replay -------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def models(gpu):
    ms = Models()
    yield ms
    for m in ms.built.values():
        m.close()


ALL_MODELS = pytest.mark.parametrize("which", ["narrow", "wide", "vl"])

INACTIVE = dict()
BIAS = dict(logit_bias={17: 100.0, 23: NINF, 900: 1.5, 5: -2.0})
# presence and frequency reach a sequence only through tokens it has already generated: the presence-only adjust rewards them (negative),
# the frequency-only one is the issue's 2.0, and both sit on the rows that run on few leaders
PRESENCE = dict(presence_penalty=-4.0)
FREQUENCY = dict(frequency_penalty=2.0)
ALL3 = dict(presence_penalty=0.5, frequency_penalty=2.0, logit_bias={40: 9.0, 41: 9.0, 42: 8.5, 43: 8.0, 44: NINF, 1000: 9.0})
# one adjust per sampler of MIXED
PAIRS = [FREQUENCY, PRESENCE, BIAS, ALL3, PRESENCE, ALL3, INACTIVE, BIAS, ALL3, PRESENCE, FREQUENCY, INACTIVE]


def with_adjust(p, adj):
    return SamplingParams(p.temperature, p.top_p, p.top_k, p.repeat_penalty, p.repeat_last_n, p.seed, **adj)


def adjusted_params():
    return [with_adjust(p, PAIRS[j]) for j, p in enumerate(MIXED)]


def replay(params, toks, step_logits, V):
    """tests/test_generate_sampled_gpu.py's replay with steps 2-3 between the penalty and the sampler."""
    s = osamp.get_logit_processor(params.temperature, params.top_p, params.top_k)
    rng = ornd.StdRng.seed_from_u64(params.seed)
    pen_v = 1.0 if params.repeat_penalty is None else params.repeat_penalty
    bias = list((params.logit_bias or {}).items())
    out = []
    for t in range(len(toks)):
        z = np.asarray(osamp.use_repeat_penalty(pen_v, params.repeat_last_n, step_logits[t], out), dtype=np.float32).copy()
        if params.adjust_active:
            ids, a = addends(params.presence_penalty, params.frequency_penalty, bias, out, V)
            z[ids] = z[ids] + a
        if s.kind == "ArgMax":
            tok = int(np.argmax(z))
        else:
            w = osamp.final_weights(z, s)
            if s.kind in ("TopK", "TopKThenTopP") and s.k < V:
                prs = osamp.softmax_last_dim(z * np.float32(1.0 / s.temperature))
                keep = osamp.topk_order(prs, z)[: s.k]
                tok = int(keep[ornd.sample_multinomial(rng, w[keep])])
            else:
                tok = ornd.sample_multinomial(rng, w)
        out.append(tok)
    return out


RUNS = {}


def adjusted_run(models, which):
    """One adjusted call per model, with logprobs, shared by the replay and the logprob tests."""
    if which not in RUNS:
        name, cfg, m = models.get(which)
        prompts = prompts_for(len(MIXED), 51, cfg.vocab_size, LENS)
        tops = [(None, 0, 1, 5, 20)[(j + 2) % 5] for j in range(len(prompts))]
        params = adjusted_params()
        toks, lps, step = m.generate_batch_adjusted(prompts, MAX_NEW, params, tops, want_step_logits=True)
        assert m.cache_len() == 0
        RUNS[which] = (prompts, params, tops, toks, lps, step)
    return RUNS[which]


@ALL_MODELS
def test_generate_batch_adjusted_exact_replay(models, which):
    name, cfg, m = models.get(which)
    V = cfg.vocab_size
    prompts, params, tops, toks, lps, step = adjusted_run(models, which)
    plain = m.generate_batch_sampled(prompts, MIXED, MAX_NEW)
    differ = [toks[j] != plain[j] for j in range(len(prompts))]
    print(f"\n{name}: sequences that differ from the unadjusted call: {differ}")
    for j, p in enumerate(params):
        assert len(toks[j]) == MAX_NEW, j
        assert replay(p, toks[j], step[j], V) == toks[j], f"sequence {j} ({p}) differs from the oracle replay"
    for j, p in enumerate(params):
        assert differ[j] == p.adjust_active, (j, p, toks[j], plain[j])
    assert 23 not in toks[2] and 44 not in toks[3] and set(toks[2]) == {17}    # the banned ids; +100 wins every step


# ---- 3. properties that need no replay ------------------------------------------------------------------------------------------------
@ALL_MODELS
def test_greedy_bans_and_a_dominant_bias(models, which):
    name, cfg, m = models.get(which)
    V = cfg.vocab_size
    prompts = prompts_for(4, 71, V, [9, 64, 33, 130])
    base, step = m.generate_batch_mm(prompts, None, MAX_NEW, want_step_logits=True)
    banned = [sorted(set(t)) for t in base]
    params = [SamplingParams(logit_bias={i: NINF for i in b}) for b in banned]
    toks, _ = m.generate_batch_adjusted(prompts, MAX_NEW, params)
    for j in range(len(prompts)):
        assert len(toks[j]) == MAX_NEW and not set(toks[j]) & set(banned[j]), (j, toks[j], banned[j])
    stop = set(m.stop_token_ids())
    lucky = next(i for i in range(100, V) if i not in stop)
    toks, _, step2 = m.generate_batch_adjusted(prompts, MAX_NEW, SamplingParams(logit_bias={lucky: 100.0}), want_step_logits=True)
    for j in range(len(prompts)):
        assert np.abs(step[j, :len(base[j])]).max() < 50 and np.abs(step2[j, :len(toks[j])]).max() < 50   # +100 beats any logit
        assert toks[j] == [lucky] * MAX_NEW, (j, toks[j])
    assert m.cache_len() == 0


@ALL_MODELS
def test_inactive_adjusts_change_nothing(models, which):
    name, cfg, m = models.get(which)
    prompts = prompts_for(len(MIXED), 51, cfg.vocab_size, LENS)
    tops = [(None, 0, 1, 5, 20)[j % 5] for j in range(len(prompts))]
    (want, wlp, wstep), base = profiled(m, lambda: m.generate_batch_logprobs(prompts, 12, tops, params=MIXED, want_step_logits=True))
    inactive = [with_adjust(p, dict(logit_bias={})) for p in MIXED]
    (toks, lps, step), prof = profiled(m, lambda: m.generate_batch_adjusted(prompts, 12, inactive, tops, want_step_logits=True))
    assert toks == want and np.array_equal(bits(step), bits(wstep))
    for j in range(len(prompts)):
        if tops[j] is None:
            assert lps[j] is None and wlp[j] is None
            continue
        for a, b in zip(lps[j], wlp[j]):
            assert bits(a[0]) == bits(b[0]) and [i for i, _ in a[1]] == [i for i, _ in b[1]]
            assert np.array_equal(bits([v for _, v in a[1]]), bits([v for _, v in b[1]]))
    assert prof == base, (prof, base)
    # greedy (params None), no logprobs: generate_batch's tokens, and no candidate step at all
    (gt, glp), gprof = profiled(m, lambda: m.generate_batch_adjusted(prompts[:5], 6))
    assert gt == m.generate_batch(prompts[:5], 6) and glp is None and all(v == 0 for v in gprof.values()), gprof


# ---- 4. logprobs with an adjust ---------------------------------------------------------------------------------------------------------
@ALL_MODELS
def test_logprobs_with_an_adjust_follow_the_raw_logits(models, which):
    prompts, params, tops, toks, lps, step = adjusted_run(models, which)
    check_sequences(toks, lps, step, tops, which)
    # a sampled row whose picked token only became likely through its bias: still the raw distribution's (low) log-probability
    j = 7                                                           # Sampling::All with +100 on id 17
    assert tops[j] is not None and set(toks[j]) == {17}
    assert all(lp[0] < -2.0 for lp in lps[j]), [lp[0] for lp in lps[j]]


# ---- 5. isolation ---------------------------------------------------------------------------------------------------------------------
@ALL_MODELS
def test_adjusted_sequences_do_not_depend_on_the_batch(models, which):
    """One prefill pass per prompt (max_tokens_per_pass=1), as tests/test_generate_sampled_gpu.py's isolation test."""
    name, cfg, m = models.get(which)
    prompts = prompts_for(len(MIXED), 53, cfg.vocab_size, LENS)
    params = adjusted_params()
    base, _, bl = m.generate_batch_adjusted(prompts, 16, params, max_tokens_per_pass=1, want_step_logits=True)
    for j in range(len(prompts)):
        alone, _, al = m.generate_batch_adjusted([prompts[j]], 16, [params[j]], max_tokens_per_pass=1, want_step_logits=True)
        assert alone[0] == base[j], j
        assert np.array_equal(bits(al[0]), bits(bl[j])), j


# ---- 6. the engine --------------------------------------------------------------------------------------------------------------------
def run_engine(m, reqs, cancel=None, max_running=4, steps_max=200):
    """reqs[i] = (ids, max_new, params, top_logprobs) submitted before step i (one prompt per prefill pass); cancel = (request, step)."""
    from aha_amd.model import HipEngine
    eng = HipEngine(m, max_running=max_running, kv_pages=64)
    try:
        rid, toks, cancelled = {}, {}, set()
        for step in range(steps_max):
            if step < len(reqs):
                ids, max_new, params, top = reqs[step]
                rid[eng.submit(ids, max_new, params, top_logprobs=top)] = step
                toks[step] = []
            if cancel and step == cancel[1]:
                eng.cancel([r for r, i in rid.items() if i == cancel[0]][0])
            evs, _, _ = eng.step(want_logits=True, want_logprobs=True)
            for ev in evs:
                if ev.cancelled:
                    cancelled.add(rid[ev.req_id])
                else:
                    toks[rid[ev.req_id]].append(ev.token)
            st = eng.stats()
            if step >= len(reqs) and st["running"] == 0 and st["waiting"] == 0:
                break
        assert st["free_pages"] == st["total_pages"], st
        return toks, cancelled
    finally:
        eng.close()


def test_engine_adjusted_requests(models):
    name, cfg, m = models.get("narrow")
    ps = prompts_for(7, 61, cfg.vocab_size, [70, 9, 33, 64, 5, 20, 41])
    sampled = SamplingParams(**QWEN3_DEFAULT, repeat_penalty=1.3, repeat_last_n=6, seed=3)
    reqs = [(ps[0], 14, with_adjust(SamplingParams(), FREQUENCY), None), (ps[1], 9, None, 5),
            (ps[2], 16, with_adjust(sampled, ALL3), 20), (ps[3], 8, SamplingParams(1.2, seed=6), None),
            (ps[4], 12, with_adjust(SamplingParams(1.0, top_k=100, seed=7), BIAS), None), (ps[5], 10, with_adjust(SamplingParams(), PRESENCE), 0),
            (ps[6], 11, with_adjust(SamplingParams(0.9, top_k=20, seed=1), dict(presence_penalty=1.0, frequency_penalty=0.5)), None)]
    toks, cancelled = run_engine(m, reqs)
    assert not cancelled
    for i, (ids, max_new, params, top) in enumerate(reqs):
        want, _ = m.generate_batch_adjusted([ids], max_new, None if params is None else [params])
        assert toks[i] == want[0], (i, toks[i], want[0])
    assert m.cache_len() == 0


def test_engine_cancelled_adjusted_request_leaves_nothing_behind(models):
    name, cfg, m = models.get("narrow")
    ps = prompts_for(2, 62, cfg.vocab_size, [33, 20])
    reqs = [(ps[0], 40, with_adjust(SamplingParams(), dict(frequency_penalty=2.0, presence_penalty=1.0, logit_bias={7: 50.0})), None),
            (ps[1], 12, with_adjust(SamplingParams(), PRESENCE), None)]
    toks, cancelled = run_engine(m, reqs, cancel=(0, 6), max_running=1)       # one slot: request 1 takes request 0's
    assert cancelled == {0} and 0 < len(toks[0]) < 40
    want, _ = m.generate_batch_adjusted([ps[1]], 12, [reqs[1][2]])
    assert toks[1] == want[0], (toks[1], want[0])
    assert m.cache_len() == 0


# ---- 7. argument errors ---------------------------------------------------------------------------------------------------------------
def test_adjust_argument_errors(models):
    import ctypes as C
    from aha_amd import _lib
    from aha_amd.model import HipEngine
    name, cfg, m = models.get("narrow")
    V = cfg.vocab_size
    prompts = prompts_for(3, 58, V, [5, 9, 3])
    ok = SamplingParams()
    bad = [dict(presence_penalty=float("nan")), dict(frequency_penalty=float("inf")), dict(logit_bias={i: 1.0 for i in range(1025)}),
           dict(logit_bias={V: 1.0}), dict(logit_bias={3: float("nan")}), dict(logit_bias={3: float("inf")})]
    for kw in bad:
        with pytest.raises(AhaHipError, match="adjust of sequence 1") as ei:
            m.generate_batch_adjusted(prompts, 4, [ok, SamplingParams(**kw), ok])
        assert ei.value.code == -1 and m.cache_len() == 0, kw
    # through the C ABI: a duplicate id, a null array with n_bias > 0
    ids = np.ascontiguousarray(np.concatenate([np.asarray(p, dtype=np.uint32) for p in prompts]))
    lens = np.asarray([len(p) for p in prompts], dtype=np.uint64)
    toks, n_out = np.zeros((3, 4), np.uint32), np.zeros(3, np.uint64)
    dup_i, dup_v = np.asarray([4, 9, 4], np.uint32), np.asarray([1, 2, 3], np.float32)
    for fill in ((0.0, 0.0, dup_i.ctypes.data_as(C.POINTER(C.c_uint32)), dup_v.ctypes.data_as(C.POINTER(C.c_float)), 3), (0.0, 0.0, None, None, 2)):
        adj = (_lib.LogitAdjust * 3)()
        adj[2] = _lib.LogitAdjust(*fill)
        rc = _lib.lib().aha_hip_generate_batch_adjusted(m.handle, ids.ctypes.data, lens.ctypes.data, 3, None, None, adj, None, 4, 0,
                                                        toks.ctypes.data, n_out.ctypes.data, None, None)
        assert rc == -1 and b"adjust of sequence 2" in _lib.lib().aha_hip_last_error() and m.cache_len() == 0
    # -inf on every id of the vocabulary needs V <= 1024 ids
    from aha_amd.configs import tiny_qwen3
    from aha_amd.model import HipInferenceModel
    from aha_amd.weights import qwen3_text_weights
    cfg2 = tiny_qwen3(layers=1, hidden=256, heads=2, kv_heads=1, inter=512, vocab=300)
    m2 = HipInferenceModel(cfg2, qwen3_text_weights(cfg2, seed=3))
    try:
        with pytest.raises(AhaHipError, match="adjust of sequence 0: -inf bias on every id"):
            m2.generate_batch_adjusted([[1, 2, 3]], 4, [SamplingParams(logit_bias={i: NINF for i in range(300)})])
        assert m2.cache_len() == 0
        toks2, _ = m2.generate_batch_adjusted([[1, 2, 3]], 4, [SamplingParams(logit_bias={i: NINF for i in range(299)})])
        assert toks2 == [[299] * 4]                                 # one id left: it is the token
    finally:
        m2.close()
    # top_logprobs without logprobs_out; the other entries' own checks still hold
    top = np.asarray([5, 5, 5], dtype=np.int32)
    rc = _lib.lib().aha_hip_generate_batch_adjusted(m.handle, ids.ctypes.data, lens.ctypes.data, 3, None, None, None, top.ctypes.data, 4, 0,
                                                    toks.ctypes.data, n_out.ctypes.data, None, None)
    assert rc == -1 and b"logprobs_out" in _lib.lib().aha_hip_last_error() and m.cache_len() == 0
    with pytest.raises(AhaHipError):
        m.generate_batch_adjusted([[1, 2], []], 4, SamplingParams(logit_bias={1: 1.0}))
    assert m.cache_len() == 0
    eng = HipEngine(m, max_running=2, kv_pages=8)
    try:
        for kw in bad:
            with pytest.raises(AhaHipError, match="engine_submit_adjusted: adjust") as ei:
                eng.submit(prompts[0], 4, SamplingParams(**kw))
            assert ei.value.code == -1 and eng.stats()["waiting"] == 0, kw
        with pytest.raises(AhaHipError, match="top_logprobs must be -1"):
            eng.submit(prompts[0], 4, SamplingParams(logit_bias={1: 1.0}), top_logprobs=21)
    finally:
        eng.close()
    assert m.cache_len() == 0
    assert m.generate_batch_adjusted(prompts, 4, ok)[0] == m.generate_batch(prompts, 4)
