"""-m gpu: draft-and-verify requests in the continuous batching engine (aha_hip_engine_submit_spec / HipEngine.submit(spec=...)).

The contract is equality, not closeness.  For the same submission history an engine whose requests came through submit_spec gives
every request the tokens, event flags and per-event logits (np.array_equal on bit patterns) of the engine whose requests came through
submit, whatever the predictions are -- true, wrong, corrupted, absent.  On top of that the per-request and engine-wide counters must
equal a host simulation of the documented scheduler (aha_amd/speculative.py engine_step_drafts), which also checks, step by step, that
the rows never pass the row budget and that a request's events of a step are consecutive with STOP / LENGTH on the last only.

Models: those of tests/test_generate_spec_gpu.py."""
import os
import sys

import numpy as np
import pytest

from aha_amd._lib import AhaHipError
from aha_amd.sampling import SamplingParams
from aha_amd.speculative import EngineRow, SpecConfig, engine_step_drafts, row_budget

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_generate_spec_gpu import prompts_for, rand_model, tied, tied_weights, untied_vl, wide_model  # noqa: E402,F401

pytestmark = pytest.mark.gpu

AHA_ERR_INVALID, AHA_ERR_OOM = -1, -3


def bits(x):
    return np.asarray(x, dtype=np.float32).view(np.uint32)


class Req:
    """One request of a run: spec None = HipEngine.submit (plain greedy, or `params`), else submit(spec=..., prediction=...)."""

    def __init__(self, ids, max_new, spec=None, prediction=None, params=None, arrival=0):
        self.ids, self.max_new, self.spec, self.prediction, self.params, self.arrival = list(ids), max_new, spec, prediction, params, arrival


def drive(m, reqs, want_logits=True, cancel=None, ctr_base=None, late=None, steps_max=400, **cfg):
    """Run an engine over reqs (submitted before step req.arrival).  cancel = (request index, step): cancelled before that step;
    late = (step, Req): one more request submitted before that step.  Returns per request its tokens, flags, logits rows and
    (proposed, accepted) -- read through request_spec after the step that ended it -- and per step the engine's events and the rows the
    step ran; and the engine's SpecStats.  Checks the event contract and the event cap in every step."""
    from aha_amd.model import HipEngine
    reqs = list(reqs)
    eng = HipEngine(m, **cfg)
    try:
        if ctr_base is not None:
            eng.debug_ctr_base(ctr_base)
        total = eng.stats()["total_pages"]
        assert eng.stats()["free_pages"] == total
        rid, out, steps = {}, {}, []
        rows_before = 0
        last_arrival = max([r.arrival for r in reqs] + ([late[0]] if late else []))
        for step in range(steps_max):
            if late and late[0] == step:
                reqs.append(late[1])
                late[1].arrival = step
            for i, r in enumerate(reqs):
                if r.arrival == step and i not in out:
                    if r.spec is None:
                        rid[eng.submit(r.ids, r.max_new, r.params)] = i
                    else:
                        rid[eng.submit(r.ids, r.max_new, spec=r.spec, prediction=r.prediction)] = i
                    out[i] = {"toks": [], "flags": [], "lg": [], "spec": None, "cancelled": False}
            if cancel and cancel[1] == step:
                eng.cancel([k for k, i in rid.items() if i == cancel[0]][0])
            cap = eng.max_events()
            res = eng.step(want_logits=want_logits)
            evs, lg = res if want_logits else (res, None)
            assert len(evs) <= cap
            st = eng.spec_stats()
            steps.append({"events": evs, "rows": st.rows - rows_before})
            rows_before = st.rows
            seen_done = set()
            for k, ev in enumerate(evs):
                i = rid[ev.req_id]
                o = out[i]
                assert ev.req_id not in seen_done, "STOP / LENGTH / CANCELLED only on a request's last event of the step"
                if k and evs[k - 1].req_id != ev.req_id:
                    assert ev.req_id not in {e.req_id for e in evs[:k]}, "a request's events of a step are consecutive"
                if ev.finished:
                    seen_done.add(ev.req_id)
                if ev.cancelled:
                    o["cancelled"] = True
                else:
                    o["toks"].append(ev.token)
                    o["flags"].append((ev.first, ev.stop, ev.length))
                    if lg is not None:
                        o["lg"].append(lg[k].copy())
                if ev.finished:
                    o["spec"] = eng.request_spec(ev.req_id)   # the step that ended it has just returned
            if step >= last_arrival and eng.stats()["running"] == 0 and eng.stats()["waiting"] == 0:
                break
        assert eng.stats()["free_pages"] == total, "every request's pages came back"
        return out, steps, eng.spec_stats()
    finally:
        eng.close()


def simulate(reqs, outs, stop=(), max_running=0):
    """The documented scheduler on the host for requests all admitted in the first step, given their greedy outputs: per-request
    (proposed, accepted), the decode steps and the rows of each."""
    gen = [o[:1] for o in outs]
    active = [j for j, r in enumerate(reqs) if r.max_new > 1]
    counts = [[0, 0] for _ in reqs]
    step_rows = []
    while active:
        rows = [EngineRow(reqs[j].ids + gen[j], len(reqs[j].ids), reqs[j].max_new, reqs[j].spec, reqs[j].prediction) for j in active]
        drafts = engine_step_drafts(rows, max_running)
        n_rows = len(active) + sum(len(d) for d in drafts)
        assert n_rows <= row_budget(len(active)), "the row budget"
        nxt = []
        for j, d in zip(active, drafts):
            left = outs[j][len(gen[j]):]
            a = 0
            while a < len(d) and a < len(left) and d[a] == left[a]:
                a += 1
            kept = left[:a + 1]
            if any(t in stop for t in kept):
                kept = kept[:min(i for i, t in enumerate(kept) if t in stop) + 1]
            counts[j][0] += len(d)
            counts[j][1] += min(a, len(kept))
            gen[j] = gen[j] + kept
            if not (kept[-1] in stop or len(gen[j]) == reqs[j].max_new):
                nxt.append(j)
        step_rows.append(n_rows)
        active = nxt
    assert gen == outs
    return [tuple(c) for c in counts], step_rows


def same_bits(a, b, what=""):
    assert a["toks"] == b["toks"], what
    assert a["flags"] == b["flags"], what
    assert len(a["lg"]) == len(b["lg"])
    for t, (x, y) in enumerate(zip(a["lg"], b["lg"])):
        assert np.array_equal(bits(x), bits(y)), (what, t)


def check_same_composition(m, prompts, max_new, spec, preds, stop=(), max_running=8, kv_pages=64, plain=None):
    """Requests all submitted before the first step and admitted whole in it: submit_spec against submit, and the counters against the
    simulation.  Returns (plain run, spec run's per-request counts, its stats)."""
    if plain is None:
        plain, _, _ = drive(m, [Req(p, max_new) for p in prompts], max_running=max_running, kv_pages=kv_pages)
    reqs = [Req(p, max_new, spec, None if preds is None else preds[j]) for j, p in enumerate(prompts)]
    got, steps, st = drive(m, reqs, max_running=max_running, kv_pages=kv_pages)
    for j in range(len(prompts)):
        same_bits(got[j], plain[j], j)
    counts, step_rows = simulate(reqs, [plain[j]["toks"] for j in range(len(prompts))], stop, max_running)
    assert [got[j]["spec"] for j in range(len(prompts))] == counts, (counts, [got[j]["spec"] for j in range(len(prompts))])
    assert [s["rows"] for s in steps[1:]] == step_rows and steps[0]["rows"] == 0, "rows of every step (the first step is the prefill)"
    assert (st.decode_steps, st.rows, st.proposed, st.accepted) == (len(step_rows), sum(step_rows), sum(c[0] for c in counts),
                                                                    sum(c[1] for c in counts)), st
    return plain, counts, st


# ---- 1. same composition, same bits (acceptance) -----------------------------------------------------------------------------------
def test_same_composition_same_bits(rand_model, tied, untied_vl):
    for cfg, m in (rand_model, tied, untied_vl):
        vocab = min(cfg.vocab_size, 2000)
        prompts = prompts_for([5, 64, 130, 33], 201, vocab)
        max_new = 40
        plain, _, st0 = drive(m, [Req(p, max_new) for p in prompts], max_running=8, kv_pages=64)
        truth = [plain[j]["toks"] for j in range(4)]
        assert (st0.decode_steps, st0.rows, st0.proposed, st0.accepted) == (max(len(o) for o in truth) - 1, sum(len(o) - 1 for o in truth), 0, 0)
        # the tokens and the last logits are generate_batch's on the same prompts (one prefill pass there as here)
        base, lb = m.generate_batch(prompts, max_new, want_logits=True)
        assert truth == base
        for j in range(4):
            assert np.array_equal(bits(plain[j]["lg"][-1]), bits(lb[j]))
        g = np.random.default_rng(202)
        wrong = [[(t + 1) % cfg.vocab_size for t in o] for o in truth]
        corrupted = [[(t + 1) % cfg.vocab_size if g.random() < 0.25 else t for t in o] for o in truth]
        for D in (1, 7, 15):
            spec = SpecConfig(D, 1, 3)
            _, counts, st = check_same_composition(m, prompts, max_new, spec, truth, plain=plain)
            # a true prediction: everything proposed is accepted, and the engine needs fewer decode steps than tokens
            assert all(p == a and a > 0 for p, a in counts) and st.decode_steps < max_new - 1, (D, counts)
            _, counts_w, _ = check_same_composition(m, prompts, max_new, spec, wrong, plain=plain)
            _, counts_c, st_c = check_same_composition(m, prompts, max_new, spec, corrupted, plain=plain)
            assert st_c.accepted < st_c.proposed
            check_same_composition(m, prompts, max_new, spec, None, plain=plain)
        # a true prediction for one request only, its neighbours plain: with max_draft 15 it emits up to 16 tokens per step
        reqs = [Req(prompts[0], max_new), Req(prompts[1], max_new, SpecConfig(15, 1, 3), truth[1]), Req(prompts[2], max_new)]
        ref, _, _ = drive(m, [Req(p, max_new) for p in prompts[:3]], max_running=8, kv_pages=64)
        got, steps, _ = drive(m, reqs, max_running=8, kv_pages=64)
        for j in range(3):
            same_bits(got[j], ref[j], j)
        n1 = len(truth[1])
        per_step = [len([e for e in s["events"] if e.req_id == 2]) for s in steps]
        want = [1] + [16] * ((n1 - 1) // 16) + ([(n1 - 1) % 16] if (n1 - 1) % 16 else [])
        assert per_step[:len(want)] == want and sum(per_step) == n1, per_step
        assert got[1]["spec"] == (n1 - len(want), n1 - len(want)) and got[0]["spec"] == (0, 0)
    # the untied model walks a permutation: with every prediction token wrong and n-grams of length >= 2 nothing is ever accepted
    cfg, m = untied_vl
    prompts = prompts_for([7, 63, 100], 203, 2000)
    plain, _, _ = drive(m, [Req(p, 30) for p in prompts], max_running=8, kv_pages=64)
    wrong = [[(t + 1) % cfg.vocab_size for t in plain[j]["toks"]] for j in range(3)]
    _, counts, st = check_same_composition(m, prompts, 30, SpecConfig(7, 2, 3), wrong, plain=plain)
    assert st.accepted == 0 and st.decode_steps == 29


# ---- 2. page and split boundaries ---------------------------------------------------------------------------------------------------
def test_page_and_split_boundaries(wide_model):
    """Drafts that cross a 64-token page (prompts of 60 .. 66 tokens) and runs inside which the cache length crosses 256 and 512, where
    the attention's split count changes: every row splits by its own length, with counters of its own."""
    cfg, m = wide_model
    for lens, max_new in (([60, 61, 62, 63], 24), ([64, 65, 66], 24), ([250, 254, 505, 509], 20), ([241, 497], 40)):
        prompts = prompts_for(lens, 81, cfg.vocab_size)
        plain, _, _ = drive(m, [Req(p, max_new) for p in prompts], max_running=4, kv_pages=40)
        truth = [plain[j]["toks"] for j in range(len(prompts))]
        for D in (7, 15):
            _, counts, st = check_same_composition(m, prompts, max_new, SpecConfig(D, 1, 3), truth, max_running=4, kv_pages=40, plain=plain)
            assert all(p == a for p, a in counts)
            if len(prompts) * (D + 1) <= 32:   # every request gets its whole draft: the closed form
                assert st.decode_steps == -(-(max_new - 1) // (D + 1))
        # corrupted predictions at the same boundaries: rejected rows leave K/V behind that the next steps overwrite
        g = np.random.default_rng(82)
        preds = [[(t + 1) % cfg.vocab_size if g.random() < 0.3 else t for t in o] for o in truth]
        check_same_composition(m, prompts, max_new, SpecConfig(7, 1, 3), preds, max_running=4, kv_pages=40, plain=plain)


# ---- 3. stop token and max_new inside an accepted run -------------------------------------------------------------------------------
def test_stop_token_and_max_new_inside_an_accepted_run(tied):
    from aha_amd.model import HipInferenceModel
    a = 600
    cfg2, w = tied_weights()
    cfg2.eos_token_ids = [a]
    m = HipInferenceModel(cfg2, w)
    try:
        prompts = [[5, 9, a], [11, a ^ 1], [40, 41, 42, 43], [100] * 70, [7, a ^ 1, a ^ 1]]
        plain, _, _ = drive(m, [Req(p, 9) for p in prompts], max_running=8, kv_pages=16)
        assert plain[0]["toks"] == [a ^ 1, a] and plain[1]["toks"] == [a, a ^ 1, a]
        # what the model would go on to say: the accepted run reaches past the stop token, the events are cut at it and keep it
        preds = [[a ^ 1, a] * 5, [a, a ^ 1] * 5, [42, 43] * 5, [101, 100] * 5, [a, a ^ 1] * 5]
        for D in (1, 3, 7, 15):
            for pr in (preds, None):
                reqs = [Req(p, 9, SpecConfig(D, 1, 3), None if pr is None else pr[j]) for j, p in enumerate(prompts)]
                got, steps, st = drive(m, reqs, max_running=8, kv_pages=16)   # (drive: every page is back at the end)
                for j in range(5):
                    same_bits(got[j], plain[j], (D, j))
                    assert got[j]["flags"][-1][1] or got[j]["flags"][-1][2]
                    assert not any(f[1] or f[2] for f in got[j]["flags"][:-1]), "the flag is on the last event"
                assert got[0]["toks"] == [a ^ 1, a] and got[0]["flags"][-1] == (False, True, False)
                counts, step_rows = simulate(reqs, [plain[j]["toks"] for j in range(5)], stop=(a,))
                assert [got[j]["spec"] for j in range(5)] == counts
                assert (st.decode_steps, st.rows) == (len(step_rows), sum(step_rows))
                if D >= 3 and pr is preds:   # request 1: [a, a^1, a] in one run whose prediction goes on: 2 drafts kept of the 3 or more that ran
                    assert got[1]["spec"][1] == 2 and got[1]["spec"][0] >= 3
    finally:
        m.close()
    # max_new inside a run the prediction would carry further; max_new == 1: no decode step at all
    cfg, m = tied
    prompts = prompts_for([5, 64, 130], 91, 2000)
    long_pred = [[p[-1] ^ 1, p[-1]] * 20 for p in prompts]
    for max_new in (2, 3, 6, 9, 17):
        for D in (3, 7, 15):
            _, counts, st = check_same_composition(m, prompts[:2], max_new, SpecConfig(D, 1, 3), long_pred[:2])
            assert st.decode_steps == -(-(max_new - 1) // (D + 1))
    reqs = [Req(p, 1, SpecConfig(7, 1, 3), long_pred[j]) for j, p in enumerate(prompts)]
    got, steps, st = drive(m, reqs, max_running=8, kv_pages=16)
    assert all(got[j]["flags"] == [(True, False, True)] for j in range(3)) and (st.decode_steps, st.rows) == (0, 0)


# ---- 4. mixed engine ----------------------------------------------------------------------------------------------------------------
def test_sampled_and_plain_neighbours_keep_their_bits(rand_model):
    """A sampled and a plain greedy request beside requests that draft: their tokens and logits are those of a run in which the
    neighbours came through submit, and those of a run without the neighbours at all.  Everything is submitted up front.  A prefill
    pass is bit-identical only for the same pass composition (include/aha_hip.h, aha_hip_engine_step), which draft-and-verify does not
    touch: the step budget of 160 rows holds the two requests' prompts (40 + 97) and not the first neighbour's 130 behind them, so
    their prefill pass is the same in all three runs and the neighbours are admitted in the next steps, beside their decode rows."""
    cfg, m = rand_model
    prompts = prompts_for([40, 97, 130, 64, 5], 211, 2000)
    sampler = SamplingParams(0.7, 0.8, 20, seed=1234)   # Qwen3's generation_config defaults, a fixed seed
    head = [Req(prompts[0], 32, params=sampler), Req(prompts[1], 32)]
    kw = dict(max_running=8, kv_pages=64, max_tokens_per_step=160)
    alone, _, _ = drive(m, head, **kw)
    ref, ref_steps, _ = drive(m, head + [Req(p, 32) for p in prompts[2:]], **kw)
    assert [e.req_id for e in ref_steps[0]["events"]] == [1, 2] and [e.req_id for e in ref_steps[1]["events"] if e.first] == [3]
    truth = [ref[j]["toks"] for j in range(5)]
    g = np.random.default_rng(212)
    preds = [None, None, truth[2], [(t + 1) % cfg.vocab_size if g.random() < 0.3 else t for t in truth[3]], None]
    mixed = head + [Req(prompts[j], 32, SpecConfig(7, 1, 3), preds[j]) for j in (2, 3, 4)]
    got, steps, st = drive(m, mixed, **kw)
    assert 0 < st.accepted < st.proposed
    for j in range(5):
        same_bits(got[j], ref[j], j)
    for j in range(2):
        same_bits(got[j], alone[j], j)
    assert len(set(got[0]["toks"])) > 4   # (the sampler did sample)
    # the head requests decoded beside rows that drafted: some step gave request 3 more than one event next to theirs
    assert any(len([e for e in s["events"] if e.req_id == 3]) > 1 and {1, 2} <= {e.req_id for e in s["events"]} for s in steps)


def test_step_logprobs_beside_requests_that_draft(rand_model):
    """aha_hip_engine_step_logprobs on steps with drafts: the entries of a top_logprobs request (greedy and sampled) equal those of a
    run whose neighbours came through submit, float for float; every event of a request that drafts has no entry (n_top = -1), and so
    has a plain neighbour's."""
    from aha_amd.model import HipEngine
    cfg, m = rand_model
    prompts = prompts_for([40, 97, 33, 64, 5], 213, 2000)
    sampler = SamplingParams(0.7, 0.8, 20, seed=77)
    truth = m.generate_batch(prompts, 24)

    def run(spec):
        out = {}
        with HipEngine(m, max_running=8, kv_pages=64) as eng:
            ids = [eng.submit(prompts[0], 24, top_logprobs=5), eng.submit(prompts[1], 24, sampler, top_logprobs=3), eng.submit(prompts[2], 24)]
            ids += [eng.submit(prompts[j], 24, spec=spec, prediction=truth[j]) if spec else eng.submit(prompts[j], 24) for j in (3, 4)]
            multi = 0
            while eng.stats()["running"] or eng.stats()["waiting"]:
                evs, lg, lps = eng.step(want_logits=True, want_logprobs=True)
                assert len(evs) == len(lps) == len(lg)
                multi += len([e for e in evs if e.req_id == ids[3]]) > 1
                for ev, row, lp in zip(evs, lg, lps):
                    out.setdefault(ids.index(ev.req_id), []).append((ev.token, bits(row).tobytes(), lp))
        return out, multi

    ref, _ = run(None)
    got, multi = run(SpecConfig(7, 1, 3))
    assert multi >= 2, "request 3 drafted, beside the logprob requests"
    for j in range(5):   # tokens and logits, bit for bit
        assert [(t, b) for t, b, _ in got[j]] == [(t, b) for t, b, _ in ref[j]], j
    for j in (0, 1):
        assert [lp for _, _, lp in got[j]] == [lp for _, _, lp in ref[j]], j
        assert all(lp is not None and len(lp[1]) == (5, 3)[j] for _, _, lp in got[j])
    for j in (2, 3, 4):
        assert all(lp is None for _, _, lp in got[j]), j
    assert [t for t, _, _ in got[3]] == truth[3]


# ---- 5. staggered arrivals and a chunked long prompt beside running spec requests ---------------------------------------------------
def test_staggered_arrivals_and_a_chunked_prompt(tied, untied_vl):
    """Tokens only: the pass composition differs between the runs.  The models are decisive, so the tokens do not depend on it."""
    for cfg, m in (tied, untied_vl):
        prompts = prompts_for([30, 64, 130, 9, 50], 221, 2000)
        max_new = [40, 33, 12, 48, 25]
        truth = [m.generate_batch([p], n)[0] for p, n in zip(prompts, max_new)]
        g = np.random.default_rng(222)
        preds = [truth[0], None, truth[2], [(t + 1) % cfg.vocab_size if g.random() < 0.2 else t for t in truth[3]], truth[4]]
        arrivals = [0, 0, 2, 3, 6]
        reqs = [Req(p, n, SpecConfig(7, 1, 3), pr, arrival=a) for p, n, pr, a in zip(prompts, max_new, preds, arrivals)]
        # 64 rows per step, chunks of 64: the 130-token prompt is prefilled in three chunks beside the running requests
        got, steps, st = drive(m, reqs, want_logits=False, max_running=4, kv_pages=32, max_tokens_per_step=64, prefill_chunk=64)
        for j in range(5):
            assert got[j]["toks"] == truth[j], j
        assert st.accepted > 0
        first_step = {j: next(s for s, x in enumerate(steps) if any(e.first and e.req_id == j + 1 for e in x["events"])) for j in range(5)}
        assert first_step[2] >= arrivals[2] + 2, "the long prompt took three steps"


# ---- 6. more requests than 32 rows allow drafts for ----------------------------------------------------------------------------------
def test_33_running_requests(rand_model):
    cfg, m = rand_model
    lens = [5, 63, 64, 65, 130, 7, 129, 64, 33, 90, 17] * 3
    prompts = prompts_for(lens, 231, 2000)
    assert len(prompts) == 33
    plain, _, _ = drive(m, [Req(p, 16) for p in prompts], max_running=64, kv_pages=33 * 3)
    truth = [plain[j]["toks"] for j in range(33)]
    g = np.random.default_rng(232)
    preds = [None if j % 3 == 2 else [(t + 1) % cfg.vocab_size if g.random() < 0.1 else t for t in o] for j, o in enumerate(truth)]
    for D in (7, 15):
        _, counts, st = check_same_composition(m, prompts, 16, SpecConfig(D, 1, 3), preds, max_running=64, kv_pages=33 * 3, plain=plain)
        assert st.proposed > 0 and st.rows <= st.decode_steps * 64


# ---- 7. cancelling a spec request mid-run --------------------------------------------------------------------------------------------
def test_cancel_after_a_partly_rejected_draft_and_slot_reuse_near_the_counter_wrap(rand_model):
    """Prompts over 256 tokens, so that the rows have two KV splits and the split-arrival counters move (draft rows' blocks included);
    the base sits a few arrivals below 2^32.  Request 0 is cancelled after the step in which 5 of its 7 drafts were kept: the K/V of the
    rejected rows stay above its cache length, in pages the late request then takes."""
    cfg, m = rand_model
    prompts = prompts_for([300, 270, 290], 241, 2000)
    max_new = 30
    kw = dict(max_running=2, kv_pages=12, ctr_base=2 ** 32 - 37)
    plain, _, _ = drive(m, [Req(p, max_new) for p in prompts[:2]], late=(4, Req(prompts[2], max_new)), cancel=(0, 2), **kw)
    full, _, _ = drive(m, [Req(p, max_new) for p in prompts[:2]], max_running=2, kv_pages=12)
    truth0 = full[0]["toks"]
    pred0 = list(truth0)
    pred0[6] = (pred0[6] + 1) % cfg.vocab_size     # drafts of the first decode step: tokens 1 .. 7, of which 1 .. 5 are right
    spec = SpecConfig(7, 1, 3)
    reqs = [Req(prompts[0], max_new, spec, pred0), Req(prompts[1], max_new, spec, full[1]["toks"])]
    late = Req(prompts[2], max_new, spec, None)
    got, steps, st = drive(m, reqs, late=(4, late), cancel=(0, 2), **kw)
    assert got[0]["cancelled"] and got[0]["toks"] == truth0[:7] and got[0]["spec"] == (7, 5)
    assert plain[0]["cancelled"] and plain[0]["toks"] == truth0[:2]
    same_bits(got[1], full[1], "the neighbour")
    same_bits(got[1], plain[1], "the neighbour")
    # the late request runs in the cancelled request's slot and pages (2 slots, 12 pages, 6 each): its bits are those of the plain run
    same_bits(got[2], plain[2], "the request that reused the slot")
    assert len(got[2]["toks"]) == max_new
    # the same without moving the counter base
    got0, _, _ = drive(m, reqs[:2] + [], late=(4, Req(prompts[2], max_new, spec, None)), cancel=(0, 2), max_running=2, kv_pages=12)
    for j in (1, 2):
        same_bits(got[j], got0[j], j)


# ---- 8. a step without drafts launches what it did before (acceptance) ---------------------------------------------------------------
def test_a_step_without_drafts_launches_what_it_did_before(tied, untied_vl):
    def launches(m, reqs):
        m.set_profiling(False)
        m.set_profiling(True)
        out, steps, st = drive(m, reqs, want_logits=False, max_running=8, kv_pages=32)
        prof = {k: m.get_profile(k)["launches"] for k in ("kv_append_rows", "spec_accept_split", "spec_accept_rows", "attn_decode_batch")}
        m.set_profiling(False)
        return out, prof, st

    cfg, m = tied
    L = cfg.num_hidden_layers
    prompts = prompts_for([90, 5, 64], 251, 2000)
    base, prof0, _ = launches(m, [Req(p, 12) for p in prompts])
    assert prof0 == {"kv_append_rows": 0, "spec_accept_split": 0, "spec_accept_rows": 0, "attn_decode_batch": L * 11}, prof0
    truth = [base[j]["toks"] for j in range(3)]
    # max_draft == 0: ordinary greedy requests, whatever the prediction
    out, prof, st = launches(m, [Req(p, 12, SpecConfig(0, 1, 3), truth[j]) for j, p in enumerate(prompts)])
    assert prof == prof0 and [out[j]["toks"] for j in range(3)] == truth and (st.proposed, st.rows) == (0, 33)
    # and with drafts the new launches are there (the test that fails without the feature)
    out, prof, st = launches(m, [Req(p, 12, SpecConfig(3, 1, 3), truth[j]) for j, p in enumerate(prompts)])
    assert [out[j]["toks"] for j in range(3)] == truth
    assert prof["spec_accept_split"] == st.decode_steps == 3 and prof["kv_append_rows"] == 3 * L and prof["attn_decode_batch"] == 3 * L
    assert prof["spec_accept_rows"] == 0
    # a silent proposer: the untied model walks a permutation, no prediction, nothing repeats
    cfg, m = untied_vl
    L = cfg.num_hidden_layers
    prompts = [[int(x) for x in np.random.default_rng(252).permutation(2000)[:n]] for n in (40, 7)]
    base, prof0, _ = launches(m, [Req(p, 12) for p in prompts])
    for j in range(2):
        assert len(set(prompts[j] + base[j]["toks"])) == len(prompts[j]) + 12, "nothing repeats"
    out, prof, st = launches(m, [Req(p, 12, SpecConfig(7, 1, 3), None) for p in prompts])
    assert prof == prof0 and prof["kv_append_rows"] == 0 and prof["attn_decode_batch"] == L * 11
    assert [out[j]["toks"] for j in range(2)] == [base[j]["toks"] for j in range(2)] and st.proposed == 0


# ---- 9. errors -----------------------------------------------------------------------------------------------------------------------
def test_errors(tied):
    import ctypes as C
    from aha_amd import _lib
    from aha_amd.model import HipEngine
    cfg, m = tied
    lib = _lib.lib()
    with HipEngine(m, max_running=4, kv_pages=8) as eng:
        def submit(ids, max_new, spec, pred=None):
            arr = None if ids is None else np.asarray(ids, dtype=np.uint32)
            p = None if pred is None else np.asarray(pred, dtype=np.uint32)
            rid = C.c_uint64()
            rc = lib.aha_hip_engine_submit_spec(eng.handle, None if arr is None else arr.ctypes.data, 0 if arr is None else arr.size, None,
                                                max_new, None if spec is None else C.byref(spec), None if p is None else p.ctypes.data,
                                                0 if p is None else p.size, C.byref(rid))
            return rc, lib.aha_hip_last_error().decode()

        good = _lib.SpecConfig(7, 1, 3)
        for args, code, message in (
                (([1, 2], 4, None), AHA_ERR_INVALID, "engine_submit_spec: null spec"),
                (([1, 2], 4, _lib.SpecConfig(16, 1, 3)), AHA_ERR_INVALID, "engine_submit_spec: max_draft must be in 0..15"),
                (([1, 2], 4, _lib.SpecConfig(-1, 1, 3)), AHA_ERR_INVALID, "engine_submit_spec: max_draft must be in 0..15"),
                (([1, 2], 4, _lib.SpecConfig(7, 0, 3)), AHA_ERR_INVALID, "n-gram bounds must satisfy 1 <= ngram_min <= ngram_max <= 8"),
                (([1, 2], 4, _lib.SpecConfig(7, 3, 2)), AHA_ERR_INVALID, "n-gram bounds must satisfy 1 <= ngram_min <= ngram_max <= 8"),
                (([1, 2], 4, _lib.SpecConfig(7, 1, 9)), AHA_ERR_INVALID, "n-gram bounds must satisfy 1 <= ngram_min <= ngram_max <= 8"),
                (([1, 2], 4, good, [3, cfg.vocab_size]), AHA_ERR_INVALID, "engine_submit_spec: prediction id out of range at position 1"),
                (([1, 2], 4, good, [0xFFFFFFFF]), AHA_ERR_INVALID, "engine_submit_spec: prediction id out of range at position 0"),
                # aha_hip_engine_submit's own
                ((None, 4, good), AHA_ERR_INVALID, "engine_submit: null input_ids / req_id"),
                (([1, 2], 0, good), AHA_ERR_INVALID, "engine_submit: max_new must be at least 1"),
                (([1, 2], (1 << 20) + 1, good), AHA_ERR_INVALID, "engine_submit: at most 2^20 new tokens"),
                (([1, cfg.vocab_size], 4, good), AHA_ERR_INVALID, "out of range"),
                (([1] * 500, 100, good), AHA_ERR_OOM, "engine_submit: the request needs 10 pages, the engine has 8")):
            rc, msg = submit(*args)
            assert rc == code and message in msg, (args[1:], rc, msg)
        st = eng.stats()
        assert st["waiting"] == 0 and st["running"] == 0 and st["free_pages"] == 8, "nothing was queued"
        with pytest.raises(ValueError):
            eng.submit([1, 2], 4, params=SamplingParams(0.7, 0.8, 20), spec=SpecConfig(3, 1, 3))
        # the cap: max_running without a request that may draft, the row budget with one, pending cancellations on top
        assert eng.max_events() == 4
        r0 = eng.submit([1, 2, 3], 4, spec=SpecConfig(0, 1, 3))
        assert eng.max_events() == 4, "max_draft 0 is an ordinary request"
        r1 = eng.submit([1, 2, 3], 6, spec=SpecConfig(3, 1, 3), prediction=[5, 6])
        assert eng.max_events() == 32
        r2 = eng.submit([9], 3)
        eng.cancel(r2)
        assert eng.max_events() == 33
        evs = (_lib.EngineEvent * 33)()
        n = C.c_size_t()
        assert lib.aha_hip_engine_step(eng.handle, evs, 32, C.byref(n), None) == AHA_ERR_INVALID
        assert "engine_step: room for 32 events, a step may emit 33" in lib.aha_hip_last_error().decode()
        # request_spec: a waiting request is not running; a running one answers; one that ended answers until the next step begins
        with pytest.raises(AhaHipError, match="engine_request_spec"):
            eng.request_spec(r1)
        # masks on a request that drafts are out of scope: set_mask refuses it, waiting or running, to set and to clear
        from aha_amd.guided import pack_mask
        words = pack_mask([5, 6, 7], cfg.vocab_size)
        for mask in (words, None):
            with pytest.raises(AhaHipError, match="engine_set_mask: request %d was submitted through engine_submit_spec" % r1) as ei:
                eng.set_mask(r1, mask)
            assert ei.value.code == AHA_ERR_INVALID
        evs = eng.step()
        assert [e.cancelled for e in evs] == [True, False, False]
        with pytest.raises(AhaHipError, match="engine_set_mask: request %d was submitted through engine_submit_spec" % r1):
            eng.set_mask(r1, words)
        eng.set_mask(r0, None)   # max_draft 0: an ordinary request
        assert eng.request_spec(r1) == (0, 0) and eng.request_spec(r0) == (0, 0)
        with pytest.raises(AhaHipError, match="engine_request_spec") as ei:
            eng.request_spec(12345)
        assert ei.value.code == AHA_ERR_INVALID
        assert eng.request_spec(r2) == (0, 0), "the cancelled request ended in the most recent step"
        ended, counts = {}, {}
        for step in range(1, 10):
            for e in eng.step():
                if e.finished:
                    ended[e.req_id] = step
                    counts[e.req_id] = eng.request_spec(e.req_id)   # it ended in the step that has just returned
            if len(ended) == 2:
                break
        assert ended[r0] == 3 and counts[r0] == (0, 0) and eng.max_events() == 4, "no request that may draft is left"
        assert counts[r1][0] >= counts[r1][1] > 0, "the prompt lookup drafted [3, 2] behind [1, 2, 3, 2], and was right"
        assert ended[r1] < ended[r0]
        with pytest.raises(AhaHipError, match="engine_request_spec"):   # it ended a step before the most recent one
            eng.request_spec(r1)
        assert eng.request_spec(r0) == (0, 0)
        eng.step()
        for r in (r0, r1, r2):   # ended two steps ago, or more
            with pytest.raises(AhaHipError, match="engine_request_spec"):
                eng.request_spec(r)
        assert eng.stats()["free_pages"] == 8
