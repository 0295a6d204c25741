"""-m gpu: the continuous batching engine (aha_hip_engine_* / HipEngine) on tiny models with the real head_dim.

Every comparison rebuilds the engine's prefill pass composition with generate_batch_mm: requests whose first-token events come out of
the same step were packed into one pass, in submission order.  A request's streamed tokens and per-event logits must then be bit-identical
to that pass's generate_batch_mm row (the decode rows are row-isolated), through staggered arrivals, cancellation, page reuse under
pressure with scrambled pages, split counters near their wrap point and a Qwen3-VL image request admitted mid-stream.  A long prompt's
chunked prefill (the packed attention over a cache prefix per segment) is held to the parity bound of the same prompt prefilled whole and
to exact greedy tokens on a decisive checkpoint.  Launches without a cache prefix reproduce the digests recorded before the change.
"""
import json
import os
import sys

import numpy as np
import pytest

from aha_amd._lib import AhaHipError
from aha_amd.configs import tiny_qwen3, tiny_qwen3vl
from aha_amd.sampling import SamplingParams
from aha_amd.weights import qwen3_text_weights, qwen3vl_weights

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import decisive  # noqa: E402
import engine_digests  # noqa: E402

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "engine_parent_digests.json")
LOGIT_TOL_STD, LOGIT_RMS_STD = 0.05, 0.02   # tests/test_model_gpu.py check_logits


def bits(x):
    return np.asarray(x, dtype=np.float32).view(np.uint32)


def prompts(seed, lens, vocab=1000):
    g = np.random.default_rng(seed)
    return [[int(x) for x in g.integers(0, vocab, size=n)] for n in lens]


@pytest.fixture(scope="module")
def text(gpu):
    from aha_amd.model import HipInferenceModel
    cfg = tiny_qwen3(layers=2, hidden=256, heads=4, kv_heads=2, inter=512, vocab=1024)
    m = HipInferenceModel(cfg, qwen3_text_weights(cfg, seed=21))
    yield cfg, m
    m.close()


def drive(m, reqs, arrivals, cancel_at=None, steps_max=400, ctr_base=None, **cfg):
    """Run an engine: reqs[i] = (ids, max_new, params, data) submitted before step arrivals[i].  Returns per request (tokens, logits rows,
    step of its first token, cancelled?) and the engine's events per step."""
    from aha_amd.model import HipEngine
    eng = HipEngine(m, **cfg)
    try:
        if ctr_base is not None:
            eng.debug_ctr_base(ctr_base)
        start_free = eng.stats()["free_pages"]
        rid, out, per_step = {}, {}, []
        for step in range(steps_max):
            for i, a in enumerate(arrivals):
                if a == step:
                    ids, max_new, params, data = reqs[i]
                    rid[eng.submit(ids, max_new, params, data)] = i
                    out[i] = {"toks": [], "lg": [], "first_step": None, "cancelled": False}
            if cancel_at and step == cancel_at[1]:
                eng.cancel([r for r, i in rid.items() if i == cancel_at[0]][0])
            evs, lg = eng.step(want_logits=True)
            per_step.append(evs)
            for k, ev in enumerate(evs):
                o = out[rid[ev.req_id]]
                if ev.cancelled:
                    o["cancelled"] = True
                    continue
                if ev.first:
                    o["first_step"] = step
                o["toks"].append(ev.token)
                o["lg"].append(lg[k].copy())
            if step > max(arrivals) and eng.stats()["running"] == 0 and eng.stats()["waiting"] == 0:
                break
        assert eng.stats()["free_pages"] == start_free
        return out, per_step
    finally:
        eng.close()


def check_against_batches(m, reqs, out, ignore=()):
    """Requests whose first tokens came out of one step shared one prefill pass: rebuild it with generate_batch_mm."""
    groups = {}
    for i in sorted(out):
        groups.setdefault(out[i]["first_step"], []).append(i)
    for step, idx in groups.items():
        max_new = max(reqs[i][1] for i in idx)
        params = None if all(reqs[i][2] is None for i in idx) else [reqs[i][2] or SamplingParams() for i in idx]
        data = None if all(reqs[i][3] is None for i in idx) else [reqs[i][3] for i in idx]
        toks, lg = m.generate_batch_mm([reqs[i][0] for i in idx], data, max_new, params=params, want_step_logits=True)
        for j, i in enumerate(idx):
            got = out[i]["toks"]
            if i in ignore:
                assert got == toks[j][:len(got)], i
            else:
                assert got == toks[j][:reqs[i][1]], (i, step)
            for t in range(len(got)):
                assert np.array_equal(bits(out[i]["lg"][t]), bits(lg[j, t])), (i, t)


def staggered(cfg, sampled):
    ps = prompts(31, (70, 130, 40, 100))
    params = [None] * 4
    if sampled:
        params = [SamplingParams(0.7, 0.9, 20, repeat_penalty=1.1, seed=5), None, SamplingParams(1.0, top_p=0.8, seed=6),
                  SamplingParams(0.5, top_k=8, seed=7)]
    return [(ps[0], 14, params[0], None), (ps[1], 30, params[1], None), (ps[2], 10, params[2], None), (ps[3], 12, params[3], None)]


@pytest.mark.parametrize("sampled", [False, True])
def test_staggered_arrivals_equal_generate_batch(text, sampled):
    cfg, m = text
    reqs = staggered(cfg, sampled)
    out, _ = drive(m, reqs, [0, 0, 5, 9], max_running=8, kv_pages=64)
    assert out[0]["first_step"] == out[1]["first_step"] == 0 and out[2]["first_step"] == 5 and out[3]["first_step"] == 9
    for i, r in enumerate(reqs):
        assert len(out[i]["toks"]) == r[1]
    check_against_batches(m, reqs, out)
    assert m.cache_len() == 0


def test_cancellation(text):
    cfg, m = text
    reqs = staggered(cfg, False)
    full, _ = drive(m, reqs, [0, 0, 5, 9], max_running=8, kv_pages=64)
    out, per_step = drive(m, reqs, [0, 0, 5, 9], cancel_at=(1, 12), max_running=8, kv_pages=64)
    assert out[1]["cancelled"] and len(out[1]["toks"]) < reqs[1][1]
    assert out[1]["toks"] == full[1]["toks"][:len(out[1]["toks"])]
    b_events = [ev for evs in per_step for ev in evs if ev.req_id == 2]
    assert b_events[-1].cancelled and not any(ev.cancelled for ev in b_events[:-1])
    for i in (0, 2, 3):
        assert out[i]["toks"] == full[i]["toks"]
        for a, b in zip(out[i]["lg"], full[i]["lg"]):
            assert np.array_equal(bits(a), bits(b))
    check_against_batches(m, reqs, out, ignore=(1,))


def test_page_reuse_under_pressure_with_scrambled_pages(gpu):
    from aha_amd.model import HipInferenceModel
    cfg = tiny_qwen3(layers=2, hidden=256, heads=4, kv_heads=2, inter=512, vocab=1024)
    m = HipInferenceModel(cfg, qwen3_text_weights(cfg, seed=21))
    try:
        m.debug_scramble_pages(True)
        # prompts over 256 tokens: two KV splits, so the reused slots' split counters move too
        ps = prompts(41, (300, 260, 320, 280, 290))
        reqs = [(p, 40, None, None) for p in ps]
        # 5 or 6 pages per request: 12 pages hold two at a time, the rest queue and reuse pages with stale K / V
        out, per_step = drive(m, reqs, [0, 0, 0, 0, 0], max_running=8, kv_pages=12)
        firsts = sorted(o["first_step"] for o in out.values())
        assert firsts[2] > firsts[0] and firsts[4] > firsts[2]
        for evs in per_step:
            assert len({ev.req_id for ev in evs}) <= 2
        check_against_batches(m, reqs, out)
    finally:
        m.close()


def test_split_counters_near_the_wrap_point(text):
    cfg, m = text
    ps = prompts(51, (300, 420, 270))   # > 256 tokens: two or more KV splits, the counters move
    reqs = [(p, 40, None, None) for p in ps] + [(ps[0][:280], 30, None, None)]
    # two slots for four requests: slots are reused while their counters run through the wrap point
    base, _ = drive(m, reqs, [0, 0, 3, 3], max_running=2, kv_pages=64)
    wrap, _ = drive(m, reqs, [0, 0, 3, 3], max_running=2, kv_pages=64, ctr_base=2 ** 32 - 37)
    assert sorted(o["first_step"] for o in base.values())[2] > 0
    check_against_batches(m, reqs, wrap)
    for i in base:
        assert wrap[i]["toks"] == base[i]["toks"]
        for a, b in zip(wrap[i]["lg"], base[i]["lg"]):
            assert np.array_equal(bits(a), bits(b))


@pytest.fixture(scope="module")
def decisive_text(gpu):
    from aha_amd.model import HipInferenceModel
    cfg = tiny_qwen3(layers=3, hidden=512, heads=4, kv_heads=2, inter=1024, vocab=2048, tie=True)
    w = qwen3_text_weights(cfg, seed=0)
    decisive.make_tied_decisive(w, "model.embed_tokens.weight", "model.norm.weight", scale=32.0, seed=7, n_text=2000)
    m = HipInferenceModel(cfg, w)
    yield cfg, m
    m.close()


def test_chunked_prefill_of_a_long_prompt(decisive_text):
    cfg, m = decisive_text
    shorts = prompts(61, (40, 55, 70, 33, 90, 64, 20, 100), vocab=2000)
    long = prompts(62, (3000,), vocab=2000)[0]
    reqs = [(p, 24, None, None) for p in shorts] + [(long, 6, None, None)]
    out, per_step = drive(m, reqs, [0] * 8 + [3], max_running=12, kv_pages=160, max_tokens_per_step=1024)
    f = out[8]["first_step"]
    assert f == 3 + 2, "3000 tokens in chunks of 1024: the first token comes with the third chunk"
    # every running stream gets exactly one event per step while the long prompt is prefilled
    for step in range(1, f + 1):
        ids = [ev.req_id for ev in per_step[step] if ev.req_id <= 8]
        assert sorted(ids) == list(range(1, 9)), step
    whole, wl = m.generate_batch_mm([long], None, 6, want_step_logits=True)
    ref = wl[0, 0]
    got = out[8]["lg"][0]
    err = float(np.abs(got - ref).max()) / float(ref.std())
    rms = float(np.sqrt(((got - ref) ** 2).mean())) / float(ref.std())
    assert err <= LOGIT_TOL_STD and rms <= LOGIT_RMS_STD, (err, rms)
    assert decisive.margin_std(ref) >= 0.5
    assert out[8]["toks"] == whole[0]
    check_against_batches(m, reqs[:8], {i: out[i] for i in range(8)})


def test_image_request_admitted_mid_stream(gpu):
    from aha_amd.model import HipInferenceModel
    from test_generate_batch_mm_gpu import make_request
    cfg = tiny_qwen3vl()
    m = HipInferenceModel(cfg, qwen3vl_weights(cfg, seed=0))
    try:
        ids, data, _ = make_request(cfg, 2, [(64, 96)], n_text=9)
        texts = prompts(71, (30, 50), vocab=1900)
        reqs = [(texts[0], 16, None, None), (texts[1], 16, None, None), (ids, 8, None, data)]
        out, _ = drive(m, reqs, [0, 0, 4], max_running=4, kv_pages=32)
        assert out[2]["first_step"] == 4
        check_against_batches(m, reqs, out)
    finally:
        m.close()


def test_engine_owns_the_cache(text):
    from aha_amd.model import HipEngine
    cfg, m = text
    eng = HipEngine(m, max_running=2, kv_pages=8)
    try:
        with pytest.raises(AhaHipError) as ei:
            m.generate_batch([[1, 2, 3]], 2)
        assert ei.value.code == -7
        with pytest.raises(AhaHipError) as ei:
            m.forward_initial([1, 2, 3], 0)
        assert ei.value.code == -7
        with pytest.raises(AhaHipError) as ei:
            HipEngine(m, max_running=2, kv_pages=8)
        assert ei.value.code == -7
        with pytest.raises(AhaHipError) as ei:
            eng.submit([1] * 600, 10)   # 10 pages > 8
        assert ei.value.code == -3
        with pytest.raises(AhaHipError) as ei:
            eng.submit([5000], 4)
        assert ei.value.code == -1 and "out of range" in str(ei.value)
        with pytest.raises(AhaHipError):
            eng.cancel(99)
        r = eng.submit([1, 2, 3], 3)
        assert len(list(eng.stream(r))) == 3
        with pytest.raises(KeyError):   # an exhausted stream's record is dropped
            eng.tokens(r)
        for bad in (dict(max_running=0), dict(max_running=65), dict(kv_pages=0), dict(max_tokens_per_step=63),
                    dict(prefill_chunk=100), dict(max_tokens_per_step=512, prefill_chunk=1024)):
            with pytest.raises(AhaHipError) as ei:
                HipEngine(m, **{"max_running": 2, "kv_pages": 8, **bad})
            assert ei.value.code == -1 and "bad config" in str(ei.value), bad
    finally:
        eng.close()
    assert m.cache_len() == 0
    m.generate_batch([[1, 2, 3]], 2)


def test_launches_without_a_cache_prefix_match_the_parent_digests(gpu):
    with open(GOLDEN) as f:
        want = json.load(f)
    assert engine_digests.compute() == want


def test_audio_request_admitted_mid_stream(gpu):
    from aha_amd.configs import tiny_qwen3_asr
    from aha_amd.model import HipInferenceModel
    from aha_amd.weights import qwen3_asr_weights
    from test_generate_batch_asr_gpu import audio_request
    cfg = tiny_qwen3_asr()
    m = HipInferenceModel(cfg, qwen3_asr_weights(cfg, seed=0))
    try:
        ids, data, _ = audio_request(cfg, 40000, 12)
        ids2, data2, _ = audio_request(cfg, 9600, 11, True, n_post=3)
        texts = prompts(81, (30, 50), vocab=1900)
        reqs = [(texts[0], 20, None, None), (texts[1], 20, None, None), (ids, 8, None, data),
                (ids2, 6, SamplingParams(0.7, 0.9, 20, seed=3), data2)]
        out, _ = drive(m, reqs, [0, 0, 4, 7], max_running=4, kv_pages=32)
        assert out[2]["first_step"] == 4 and out[3]["first_step"] == 7
        check_against_batches(m, reqs, out)
    finally:
        m.close()


def test_model_close_takes_an_open_engine_along(gpu):
    from aha_amd.model import HipEngine, HipInferenceModel
    cfg = tiny_qwen3(layers=1, hidden=256, heads=4, kv_heads=2, inter=512, vocab=1024)
    m = HipInferenceModel(cfg, qwen3_text_weights(cfg, seed=3))
    eng = HipEngine(m, max_running=2, kv_pages=4)
    eng.submit([1, 2, 3], 2)
    eng.step()
    m.close()
    assert not eng.handle
    eng.close()   # a no-op


# ---- op level: the packed attention with a cache prefix per segment (AttnPrefillArgs::seg_kv0) ----------------------------------
def _segs_case(segs, nh, kvh, seed):
    import torch
    from test_ops_gpu import rnd
    d = 128
    S = sum(n for n, _ in segs)
    L = sum(n + k0 for n, k0 in segs)
    return rnd((S, nh * d), seed), rnd((L, kvh * d), seed + 1), rnd((L, kvh * d), seed + 2)


@pytest.mark.parametrize("segs", [
    [(100, 64)],                                   # a prefix of one page, a chunk over two pages
    [(300, 1024)],                                 # a long prefix, a chunk spanning five pages
    [(64, 64), (37, 0), (130, 1024), (1, 128)],    # mixed: with and without a prefix, a one-row chunk
    [(200, 0), (65, 192), (64, 0)],
])
@pytest.mark.parametrize("nh,kvh", [(4, 2), (8, 2)])
def test_attn_prefill_segments_with_a_cache_prefix(gpu, segs, nh, kvh):
    """Every segment's rows against the oracle (the f32 score chain's rounding points at 3 bf16 ulp of the row scale, the eager oracle at
    4: tests/test_ops_gpu.py's bounds) and against the single-sequence launch with kv_offset = kv0 over the same cache."""
    import torch
    from aha_amd import ops
    from test_ops_gpu import NM_F32SCORES, _attn_ref, assert_close_ulps
    d = 128
    q, k, v = _segs_case(segs, nh, kvh, 90 + len(segs))
    got = ops.attn_prefill_segs(q.to(gpu), k.to(gpu), v.to(gpu), nh, kvh, segs, True).cpu()
    r0 = c0 = 0
    for j, (n, k0) in enumerate(segs):
        qs, ks, vs = q[r0:r0 + n], k[c0:c0 + k0 + n], v[c0:c0 + k0 + n]
        g = got[r0:r0 + n]
        what = f"segment {j} (len {n}, kv0 {k0})"
        assert_close_ulps(g, _attn_ref(qs, ks, vs, nh, kvh, d, True, k0, NM_F32SCORES), 3, None, what + " vs f32-score oracle", row_scale=True)
        assert_close_ulps(g, _attn_ref(qs, ks, vs, nh, kvh, d, True, k0), 4, None, what + " vs eager oracle", row_scale=True)
        single = ops.attn_prefill(qs.to(gpu), ks.to(gpu), vs.to(gpu), nh, kvh, d, k0, True).cpu()
        assert_close_ulps(g, single.float(), 3, None, what + " vs the kv_offset launch", row_scale=True)
        r0 += n
        c0 += k0 + n


def test_attn_prefill_segments_without_a_prefix_are_the_plain_launch(gpu):
    """kv0 all 0: the launch with seg_kv0 and the one without it give the same bits."""
    import torch
    from aha_amd import ops
    segs = [(200, 0), (65, 0), (1, 0), (130, 0)]
    q, k, v = _segs_case(segs, 8, 2, 77)
    a = ops.attn_prefill_segs(q.to(gpu), k.to(gpu), v.to(gpu), 8, 2, segs, True)
    b = ops.attn_prefill_segs(q.to(gpu), k.to(gpu), v.to(gpu), 8, 2, segs, False)
    assert torch.equal(a, b)
