"""Continuous batching (aha_hip_engine_* / HipEngine) under seeded Poisson arrivals, on the Qwen3-0.6B and Qwen3-VL-8B text shapes with
seeded random weights (no stop tokens: every request runs to its max_new).

Workload per model: --requests requests, prompt lengths drawn from --lens (seeded), one of them --long tokens long, arrivals a Poisson
process of --rate requests per engine step (seeded), every request --max-new tokens.  Reported (JSON, one line per model and mode):
  engine   aggregate generated tok/s over the wall time of the run, time to first token (submit -> FIRST event; mean / p99 ms), inter-token
           latency (gap between a request's consecutive events; mean / p99 ms) and the worst gap of a running stream during the long
           prompt's admission;
  serial   the same requests one after the other through generate_batch with one prompt each (no overlap: arrivals ignored);
  waves    generate_batch over waves of --max-running requests in arrival order (a wave starts when the previous one ends);
  steady   decode at a fixed number of rows (--max-running requests of --steady-len tokens, all admitted at once): the engine's step time
           once every request has its first token, against generate_batch's per-step time at the same rows ((t(1 + N new) - t(1 new)) / N);
  long     the --long prompt's whole prefill alone (generate_batch with max_new 1), the figure a chunked admission is to stay below.
Writes the lines to --out (default: stdout only).

--spec: draft-and-verify requests instead (HipEngine.submit(spec=...), aha_hip_engine_submit_spec).  Per model, for 1 / 4 / 16 concurrent
requests of --steady-len tokens (all admitted in the first step), predictions = the greedy output with 0 / 50 / 100 % of its tokens
corrupted (seeded) and max_draft 7 / 15: engines with predictions and engines without, alternated, --spec-repeats runs each, and
generate_batch_spec against generate_batch on the same prompts.  Reported per case (one JSON line): the decode phase's aggregate tok/s
(tokens after the first ones over the time from the end of the prefill step to the last event; min / median / max over the runs), the
mean inter-token gap of a request (that time over its tokens), the engine's decode steps and accepted / proposed draft tokens.
--repeat N runs the Poisson workload N times and reports every run (for a comparison of two trees, alternated from outside).
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def model_for(name):
    from aha_amd.configs import qwen3_0_6b, qwen3vl_8b_text
    from aha_amd.model import HipInferenceModel
    from aha_amd.weights import qwen3_text_weights
    cfg = qwen3_0_6b() if name == "0.6b" else qwen3vl_8b_text()
    cfg.eos_token_ids = []
    return cfg, HipInferenceModel(cfg, qwen3_text_weights(cfg, seed=0, device="cuda"))


def workload(a, vocab):
    g = np.random.default_rng(a.seed)
    lens = [int(x) for x in g.choice(a.lens, size=a.requests)]
    lens[a.requests // 2] = a.long
    prompts = [[int(x) for x in g.integers(0, min(vocab, 150000), size=n)] for n in lens]
    gaps = g.exponential(1.0 / a.rate, size=a.requests)
    arrive = np.floor(np.cumsum(gaps) - gaps[0]).astype(int).tolist()
    return prompts, arrive


def pct(x, q):
    return float(np.percentile(np.asarray(x), q)) * 1e3 if len(x) else 0.0


def run_engine(m, prompts, arrive, a):
    from aha_amd.model import HipEngine
    pages = sum((len(p) + a.max_new + 63) // 64 for p in prompts) + 8
    eng = HipEngine(m, max_running=a.max_running, kv_pages=pages, max_tokens_per_step=a.budget, prefill_chunk=a.chunk)
    t_sub, last, ttft, itl, long_gap = {}, {}, [], [], 0.0
    n_tok, step, long_id, long_live = 0, 0, None, False
    t0 = time.perf_counter()
    try:
        nxt = 0
        while nxt < len(prompts) or eng.stats()["running"] or eng.stats()["waiting"]:
            while nxt < len(prompts) and arrive[nxt] <= step:
                r = eng.submit(prompts[nxt], a.max_new)
                t_sub[r] = time.perf_counter()
                if len(prompts[nxt]) == a.long:
                    long_id, long_live = r, True
                nxt += 1
            evs = eng.step()
            now = time.perf_counter()
            for ev in evs:
                n_tok += 1
                if ev.first:
                    ttft.append(now - t_sub[ev.req_id])
                    if ev.req_id == long_id:
                        long_live = False
                else:
                    gap = now - last[ev.req_id]
                    itl.append(gap)
                    if long_live:
                        long_gap = max(long_gap, gap)
                last[ev.req_id] = now
            step += 1
    finally:
        eng.close()
    wall = time.perf_counter() - t0
    return {"mode": "engine", "tok_s": n_tok / wall, "wall_s": wall, "steps": step, "ttft_mean_ms": float(np.mean(ttft)) * 1e3,
            "ttft_p99_ms": pct(ttft, 99), "itl_mean_ms": float(np.mean(itl)) * 1e3, "itl_p99_ms": pct(itl, 99),
            "itl_max_during_long_admission_ms": long_gap * 1e3}


def run_serial(m, prompts, a):
    t0 = time.perf_counter()
    n = 0
    for p in prompts:
        n += len(m.generate_batch([p], a.max_new)[0])
    wall = time.perf_counter() - t0
    return {"mode": "serial", "tok_s": n / wall, "wall_s": wall}


def run_waves(m, prompts, a):
    t0 = time.perf_counter()
    n = 0
    for w0 in range(0, len(prompts), a.max_running):
        n += sum(len(t) for t in m.generate_batch(prompts[w0:w0 + a.max_running], a.max_new, a.budget))
    wall = time.perf_counter() - t0
    return {"mode": "waves", "tok_s": n / wall, "wall_s": wall}


def run_steady(m, a, vocab):
    from aha_amd.model import HipEngine
    g = np.random.default_rng(a.seed + 1)
    R, n = a.max_running, a.steady_steps
    ps = [[int(x) for x in g.integers(0, min(vocab, 150000), size=a.steady_len)] for _ in range(R)]
    eng = HipEngine(m, max_running=R, kv_pages=R * ((a.steady_len + n + 80) // 64 + 1), max_tokens_per_step=max(a.budget, R * a.steady_len))
    try:
        for p in ps:
            eng.submit(p, n + 4)
        eng.step()   # every prefill, the first tokens
        eng.step()
        t0 = time.perf_counter()
        for _ in range(n):
            assert len(eng.step()) == R
        t_eng = (time.perf_counter() - t0) / n
    finally:
        eng.close()
    t1 = min(timed_call(lambda: m.generate_batch(ps, 1, a.budget)) for _ in range(3))
    tn = min(timed_call(lambda: m.generate_batch(ps, n + 1, a.budget)) for _ in range(3))
    t_gb = (tn - t1) / n
    return {"mode": "steady", "rows": R, "kv_len": a.steady_len, "engine_step_ms": t_eng * 1e3, "generate_batch_step_ms": t_gb * 1e3,
            "engine_tok_s": R / t_eng, "generate_batch_tok_s": R / t_gb}


def timed_call(fn):
    t0 = time.perf_counter()
    fn()
    return time.perf_counter() - t0


def run_long(m, a, vocab):
    g = np.random.default_rng(a.seed + 2)
    p = [int(x) for x in g.integers(0, min(vocab, 150000), size=a.long)]
    t = min(timed_call(lambda: m.generate_batch([p], 1)) for _ in range(3))
    return {"mode": "long", "whole_prefill_ms": t * 1e3, "tokens": a.long}


def run_spec_engine(m, prompts, a, spec, preds):
    """One engine run over prompts all submitted up front; spec None: plain requests.  -> (tokens per request, decode seconds, stats)"""
    from aha_amd.model import HipEngine
    R = len(prompts)
    eng = HipEngine(m, max_running=R, kv_pages=R * ((a.steady_len + a.max_new + 63) // 64 + 1), max_tokens_per_step=max(a.budget, R * a.steady_len))
    try:
        ids = [eng.submit(p, a.max_new) if spec is None else eng.submit(p, a.max_new, spec=spec, prediction=preds[j])
               for j, p in enumerate(prompts)]
        eng.step()   # every prefill, the first tokens
        t0 = time.perf_counter()
        while eng.stats()["running"]:
            eng.step()
        secs = time.perf_counter() - t0
        st = eng.spec_stats()
        return [eng.tokens(r) for r in ids], secs, st
    finally:
        eng.close()


def run_spec(m, a, vocab, name):
    from aha_amd.speculative import SpecConfig
    g = np.random.default_rng(a.seed + 3)
    out = []
    for R in (1, 4, 16):
        prompts = [[int(x) for x in g.integers(0, min(vocab, 150000), size=a.steady_len)] for _ in range(R)]
        truth, _, _ = run_spec_engine(m, prompts, a, None, None)
        n_dec = sum(len(t) - 1 for t in truth)
        t1 = min(timed_call(lambda: m.generate_batch(prompts, 1, a.budget)) for _ in range(3))
        for corrupt in (0.0, 0.5, 1.0):
            preds = [[(t + 1) % vocab if g.random() < corrupt else t for t in o] for o in truth]
            for D in (7, 15):
                spec = SpecConfig(D, 1, 3)
                plain, drafted, st = [], [], None
                for _ in range(a.spec_repeats):   # alternated: the two see the same clocks and the same neighbours on the machine
                    plain.append(run_spec_engine(m, prompts, a, None, None)[1])
                    toks, secs, st = run_spec_engine(m, prompts, a, spec, preds)
                    assert toks == truth, "draft-and-verify changed the tokens"
                    drafted.append(secs)
                gb = min(timed_call(lambda: m.generate_batch(prompts, a.max_new, a.budget)) for _ in range(a.spec_repeats)) - t1
                gbs = min(timed_call(lambda: m.generate_batch_spec(prompts, a.max_new, spec, preds, max_tokens_per_pass=a.budget))
                          for _ in range(a.spec_repeats)) - t1

                def rate(ts):
                    return {"min": n_dec / max(ts), "median": n_dec / float(np.median(ts)), "max": n_dec / min(ts)}
                r = {"mode": "spec", "model": name, "requests": R, "kv_len": a.steady_len, "max_new": a.max_new, "corrupt": corrupt, "max_draft": D,
                     "engine_plain_tok_s": rate(plain), "engine_spec_tok_s": rate(drafted),
                     "engine_plain_gap_ms": float(np.median(plain)) * R / n_dec * 1e3, "engine_spec_gap_ms": float(np.median(drafted)) * R / n_dec * 1e3,
                     "generate_batch_tok_s": n_dec / gb, "generate_batch_spec_tok_s": n_dec / gbs,
                     "decode_steps": st.decode_steps, "proposed": st.proposed, "accepted": st.accepted, "runs": a.spec_repeats}
                print(json.dumps(r), flush=True)
                out.append(r)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--models", default="0.6b,8b")
    ap.add_argument("--requests", type=int, default=24)
    ap.add_argument("--lens", type=lambda s: [int(x) for x in s.split(",")], default=[64, 200, 512, 1000])
    ap.add_argument("--long", type=int, default=8192)
    ap.add_argument("--rate", type=float, default=0.25, help="mean arrivals per engine step")
    ap.add_argument("--max-new", type=int, default=64)
    ap.add_argument("--max-running", type=int, default=16)
    ap.add_argument("--budget", type=int, default=2048)
    ap.add_argument("--chunk", type=int, default=1024)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--skip-baselines", action="store_true")
    ap.add_argument("--steady-len", type=int, default=512)
    ap.add_argument("--steady-steps", type=int, default=32)
    ap.add_argument("--out", default="")
    ap.add_argument("--spec", action="store_true", help="measure draft-and-verify requests instead of the Poisson workload")
    ap.add_argument("--spec-repeats", type=int, default=3)
    ap.add_argument("--repeat", type=int, default=1, help="runs of the Poisson workload")
    a = ap.parse_args()
    lines = []
    for name in a.models.split(","):
        cfg, m = model_for(name)
        prompts, arrive = workload(a, cfg.vocab_size)
        m.generate_batch([prompts[0][:64]], 4)   # warm-up: code objects, scratch
        if a.spec:
            lines += run_spec(m, a, cfg.vocab_size, name)
            m.close()
            continue
        res = [run_engine(m, prompts, arrive, a) for _ in range(a.repeat)]
        if not a.skip_baselines:
            res += [run_serial(m, prompts, a), run_waves(m, prompts, a), run_steady(m, a, cfg.vocab_size), run_long(m, a, cfg.vocab_size)]
        for r in res:
            r.update(model=name, requests=a.requests, max_new=a.max_new, max_running=a.max_running, budget=a.budget, chunk=a.chunk,
                     long=a.long)
            print(json.dumps(r), flush=True)
            lines.append(r)
        m.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for r in lines:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
