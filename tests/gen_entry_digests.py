"""Output digests, launch counts and model-level refusals of every batch generation entry and of the engine's four submit entries, each
through its own Python method.  tests/golden/gen_entries_parent_digests.json holds them as computed by the library before the entries
were folded onto one options struct and one implementation (`python tests/gen_entry_digests.py OUT.json` on an MI355X);
tests/test_gen_entries_gpu.py recomputes them and asserts equality.

Per entry: a sha256 over the tokens, n_out and the returned logits / step logits / logprob structs; with profiling on, the launches of
gemv_rows, argmax, sample_rows_stage1 and logprob_rows_stage1 (no step gained or lost a launch); and the (code, message) of refusals that
need a model (the messages raised inside the shared implementation keep their fixed prefixes whichever entry was called)."""
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

LENS, MAX_NEW = (70, 5, 64, 130), 6     # under a page, a few tokens, exactly a page, over two pages
CLASSES = ("gemv_rows", "argmax", "sample_rows_stage1", "logprob_rows_stage1")


def sha(*arrays) -> str:
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def tok_arrays(toks):
    """Token lists -> (flat tokens, n_out)."""
    return np.asarray([t for row in toks for t in row], np.uint32), np.asarray([len(row) for row in toks], np.uint64)


def lp_arrays(lps):
    """The logprob structs as the wrappers return them -> (float32 values, int64 ids and markers), None entries marked."""
    f, i = [], []
    for seq in lps if lps is not None else [None]:
        if seq is None:
            i.append(-7)
            continue
        for e in seq if isinstance(seq, list) else [seq]:
            if e is None:
                i.append(-9)
                continue
            f.append(e[0])
            i.append(len(e[1]))
            for tid, lp in e[1]:
                i.append(tid)
                f.append(lp)
    return np.asarray(f, np.float32), np.asarray(i, np.int64)


def compute() -> dict:
    from aha_amd._lib import AhaHipError
    from aha_amd.configs import tiny_qwen3
    from aha_amd.guided import ChoiceConstraint, pack_mask
    from aha_amd.model import HipEngine, HipInferenceModel
    from aha_amd.sampling import SamplingParams
    from aha_amd.weights import qwen3_text_weights

    out = {}
    cfg = tiny_qwen3(layers=2, hidden=256, heads=4, kv_heads=2, inter=512, vocab=1024)
    V = cfg.vocab_size
    w = qwen3_text_weights(cfg, seed=11)
    g = np.random.default_rng(12)
    prompts = [[int(x) for x in g.integers(0, V, size=n)] for n in LENS]
    # the stop id: the third token greedy decoding gives the second prompt, so in the greedy entries that sequence ends early, at the
    # id's first occurrence after the first token
    m = HipInferenceModel(cfg, w)
    free = m.generate_batch(prompts, MAX_NEW)
    m.close()
    stop = free[1][2]
    cfg.eos_token_ids = [stop]
    m = HipInferenceModel(cfg, w)
    assert m.stop_token_ids() == [stop]

    def profiled(name, fn):
        m.set_profiling(False)
        m.set_profiling(True)
        res = fn()
        out[name + "/launches"] = {c: int(m.get_profile(c)["launches"]) for c in CLASSES}
        m.set_profiling(False)
        return res

    def refusal(name, fn):
        try:
            fn()
        except AhaHipError as e:
            out["refused/" + name] = [int(e.code), str(e)]
            return
        raise AssertionError(name + ": the call was not refused")

    toks, lg = profiled("generate_batch", lambda: m.generate_batch(prompts, MAX_NEW, want_logits=True))
    assert 1 < len(toks[1]) < MAX_NEW and toks[1][-1] == stop, toks
    out["generate_batch"] = sha(*tok_arrays(toks), lg)

    mixed = [SamplingParams(seed=21), SamplingParams(0.8, None, 12, 1.15, 32, seed=22), SamplingParams(0.9, 0.85, None, None, 64, seed=23),
             SamplingParams(1.3, None, None, None, 64, seed=24)]   # argmax; top-k + repeat penalty; top-p; temperature over all candidates
    toks, lg = profiled("generate_batch_sampled", lambda: m.generate_batch_sampled(prompts, mixed, MAX_NEW, want_step_logits=True))
    out["generate_batch_sampled"] = sha(*tok_arrays(toks), lg)

    toks, lg = profiled("generate_batch_mm", lambda: m.generate_batch_mm(prompts, None, MAX_NEW, None, want_step_logits=True))
    out["generate_batch_mm"] = sha(*tok_arrays(toks), lg)

    toks, lps, lg = profiled("generate_batch_logprobs",
                             lambda: m.generate_batch_logprobs(prompts, MAX_NEW, [0, 3, None, 20], want_step_logits=True))
    assert lps[2] is None and len(lps[3][0][1]) == 20
    out["generate_batch_logprobs"] = sha(*tok_arrays(toks), lg, *lp_arrays(lps))

    adjusted = [SamplingParams(seed=31, logit_bias={7: 4.0, 900: -3.0, stop: float("-inf")}, presence_penalty=0.6, frequency_penalty=0.4),
                SamplingParams(seed=32),
                SamplingParams(0.8, None, 12, 1.1, 64, seed=33, logit_bias={5: 2.5, 6: 2.5}, presence_penalty=0.3, frequency_penalty=0.7),
                SamplingParams(0.9, 0.9, None, None, 64, seed=34)]
    toks, lps, lg = profiled("generate_batch_adjusted",
                             lambda: m.generate_batch_adjusted(prompts, MAX_NEW, adjusted, [None, None, 5, None], want_step_logits=True))
    out["generate_batch_adjusted"] = sha(*tok_arrays(toks), lg, *lp_arrays(lps))

    choices = [[900, 901, 902], [900, 901], [900, 950, 951, 952, 953, 954], [1000], [333, 901, 17, 23]]
    con = ChoiceConstraint(choices, [stop], V)
    masked = [SamplingParams(seed=40), SamplingParams(seed=41), SamplingParams(0.8, None, 12, seed=42), SamplingParams(seed=43)]
    toks, lps, lg = profiled("generate_batch_masked", lambda: m.generate_batch_masked(
        prompts, MAX_NEW, lambda seq, gen: con(seq, gen) if seq in (0, 2) else None, masked, [2, None, None, None], want_step_logits=True))
    assert all(toks[j][0] in (900, 1000, 333) for j in (0, 2)), toks
    out["generate_batch_masked"] = sha(*tok_arrays(toks), lg, *lp_arrays(lps))

    pred = [None, list(free[1]), None, None]
    toks, lg, info = profiled("generate_batch_spec", lambda: m.generate_batch_spec(prompts, MAX_NEW, None, pred, want_logits=True, want_stats=True))
    st = info["stats"]
    out["generate_batch_spec"] = sha(*tok_arrays(toks), lg, np.asarray(info["proposed"] + info["accepted"] +
                                                                      [st.decode_steps, st.rows, st.proposed, st.accepted], np.uint64))

    # ---- refusals that need a model, through the entries that share the implementation ----
    one = SamplingParams(seed=1)
    entries = {
        "generate_batch": lambda ps, n: m.generate_batch(ps, n),
        "generate_batch_sampled": lambda ps, n: m.generate_batch_sampled(ps, one, n),
        "generate_batch_mm": lambda ps, n: m.generate_batch_mm(ps, None, n),
        "generate_batch_logprobs": lambda ps, n: m.generate_batch_logprobs(ps, n, 2),
        "generate_batch_adjusted": lambda ps, n: m.generate_batch_adjusted(ps, n, one),
        "generate_batch_masked": lambda ps, n: m.generate_batch_masked(ps, n, lambda seq, gen: None),
        "generate_batch_spec": lambda ps, n: m.generate_batch_spec(ps, n),
    }
    for name, call in entries.items():
        refusal(name + "/n_seqs_0", lambda: call([], 4))
        refusal(name + "/max_new_0", lambda: call(prompts[:2], 0))
        refusal(name + "/id_at_vocab", lambda: call([prompts[1], [1, 2, V]], 4))
    bad_bias = [one, SamplingParams(seed=2, logit_bias={V: 1.0})]
    refusal("generate_batch_adjusted/bias_id_at_vocab", lambda: m.generate_batch_adjusted(prompts[:2], 4, bad_bias))
    refusal("generate_batch_masked/bias_id_at_vocab", lambda: m.generate_batch_masked(prompts[:2], 4, lambda seq, gen: None, bad_bias))
    refusal("generate_batch_masked/callback_returns_minus_3", lambda: m.generate_batch_masked(prompts[:2], 4, lambda seq, gen: -3 if seq else None))
    assert m.cache_len() == 0

    # ---- the engine: one request through each submit entry, run to completion with step logits and logprobs ----
    eng = HipEngine(m, max_running=4, kv_pages=16)
    try:
        W = (V + 31) // 32
        refusal("engine_submit_adjusted/bias_id_at_vocab", lambda: eng.submit(prompts[0], 4, bad_bias[1]))
        refusal("engine_submit_masked/bias_id_at_vocab", lambda: eng.submit(prompts[0], 4, bad_bias[1], mask=np.ones(W, np.uint32)))
        refusal("engine_submit_masked/wrong_word_count", lambda: eng.submit(prompts[0], 4, mask=np.ones(W - 1, np.uint32)))
        refusal("engine_submit/max_new_0", lambda: eng.submit(prompts[0], 0))
        refusal("engine_submit_logprobs/id_at_vocab", lambda: eng.submit([1, V], 4, top_logprobs=2))
        refusal("generate_batch/engine_owns_the_cache", lambda: m.generate_batch(prompts[:1], 2))
        refusal("generate_batch_masked/engine_owns_the_cache", lambda: m.generate_batch_masked(prompts[:1], 2, lambda seq, gen: None))
        assert eng.stats()["waiting"] == 0

        def run():
            rids = [eng.submit(prompts[0], MAX_NEW),                                               # aha_hip_engine_submit
                    eng.submit(prompts[1], MAX_NEW, SamplingParams(0.8, None, 12, seed=51), top_logprobs=3),   # _logprobs
                    eng.submit(prompts[2], MAX_NEW, adjusted[2], top_logprobs=2),                      # _adjusted
                    eng.submit(prompts[3], MAX_NEW, adjusted[0], top_logprobs=0,                       # _masked
                               mask=pack_mask(list(range(100, 400)) + [7, 900], V))]
            evs, lgs, lps = [], [], []
            for _ in range(4 * MAX_NEW + 8):
                if all(eng.finished(r) for r in rids):
                    break
                e, lg_, lp_ = eng.step(want_logits=True, want_logprobs=True)
                evs += [(ev.req_id - rids[0], ev.token, ev.first, ev.stop, ev.length, ev.cancelled) for ev in e]
                lgs.append(lg_)
                lps += lp_
            assert all(eng.finished(r) for r in rids)
            return evs, np.concatenate(lgs), lps, [eng.tokens(r) for r in rids]
        evs, lgs, lps, toks = profiled("engine", run)
        assert all(100 <= t < 400 or t in (7, 900) for t in toks[3]) and lps[0] is None
        out["engine"] = sha(np.asarray(evs, np.int64), lgs, *lp_arrays(lps), *tok_arrays(toks))
    finally:
        eng.close()
    m.close()
    return out


if __name__ == "__main__":
    res = compute()
    print(json.dumps(res, indent=1))
    if len(sys.argv) > 1:
        os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
        with open(sys.argv[1], "w") as f:
            json.dump(res, f, indent=1, sort_keys=True)
