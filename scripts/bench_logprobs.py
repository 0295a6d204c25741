"""What per-token log-probabilities cost (aha_hip_generate_batch_logprobs against aha_hip_generate_batch_mm on the same build), at the
Qwen3-0.6B and Qwen3-VL-8B text dimensions of scripts/bench_generate_batch.py (seeded random weights generated on the GPU, no stop tokens
so every sequence runs to max_new).  Per model, sequence count B (1 / 16 / 64) and sampler (greedy; the Qwen3 default request: T 0.6 /
top_p 0.95 / top_k 20), one line per top_logprobs setting:
  mm     aha_hip_generate_batch_mm: the baseline;
  none   generate_batch_logprobs with every entry -1 (the pass never runs);
  0 / 5 / 20   every sequence asks for that many alternatives.
Each line: the decode step time, taken as (t(max_new) - t(1)) / (max_new - 1) with the best of --reps runs of each -- the C entry point
alone is timed, on arrays packed beforehand, so that the Python wrapper's per-token tuples do not count -- decode tok/s, the step over the
baseline's, and -- from one more run with profiling on -- the microseconds per step of the two profile classes of the pass
(logprob_rows_stage1 / logprob_rows_stage2; event-timed, so each includes its launch).  One JSON object per line.
    python scripts/bench_logprobs.py [--only 0.6b,8b] [--batches 1,16,64] [--prompt 128] [--max-new 64] [--reps 3]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np


def model_for(name):
    import torch
    from aha_amd.configs import qwen3_0_6b, qwen3vl_8b_text
    from aha_amd.model import HipInferenceModel
    from aha_amd.weights import qwen3_text_weights
    cfg = qwen3_0_6b() if name == "0.6b" else qwen3vl_8b_text()
    cfg.eos_token_ids = []
    w = qwen3_text_weights(cfg, seed=0, device="cuda")
    m = HipInferenceModel(cfg, w)
    del w
    torch.cuda.empty_cache()
    return cfg, m


def prompts(n, L, vocab, seed=0):
    g = np.random.default_rng(seed)
    return [g.integers(0, min(vocab, 150000), size=L).astype(np.uint32).tolist() for _ in range(n)]


def best(fn, reps):
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        ts.append(time.perf_counter() - t0)
    return min(ts), out


class Call:
    """One batch packed for the C ABI: run(setting, max_new) calls aha_hip_generate_batch_mm ("mm") or aha_hip_generate_batch_logprobs
    (top_logprobs -1 for "none", else the setting for every sequence) and returns n_out."""

    def __init__(self, m, ps, params, max_new):
        import ctypes as C
        from aha_amd import _lib
        from aha_amd.model import _pack_batch, _sampling_array
        self.m, self.n = m, len(ps)
        self.ids, self.lens = _pack_batch(ps)
        self.cp = None if params is None else _sampling_array(params, self.n)
        self.toks = np.zeros((self.n, max_new), np.uint32)
        self.n_out = np.zeros(self.n, np.uint64)
        self.lp = (_lib.TokenLogprobs * (self.n * max_new))()
        self.lib, self.check = _lib.lib(), _lib.check

    def run(self, setting, max_new):
        a = (self.m.handle, self.ids.ctypes.data, self.lens.ctypes.data, self.n, None, self.cp)
        b = (max_new, 0, self.toks.ctypes.data, self.n_out.ctypes.data, None)
        if setting == "mm":
            self.check(self.lib.aha_hip_generate_batch_mm(*a, *b))
        else:
            top = np.full(self.n, -1 if setting == "none" else setting, dtype=np.int32)
            self.check(self.lib.aha_hip_generate_batch_logprobs(*a, top.ctypes.data, *b, self.lp))
        return self.n_out.copy()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default="0.6b,8b")
    ap.add_argument("--batches", default="1,16,64")
    ap.add_argument("--prompt", type=int, default=128)
    ap.add_argument("--max-new", type=int, default=64)
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    from aha_amd import build
    build.build()
    from aha_amd.sampling import SamplingParams
    for name in a.only.split(","):
        cfg, m = model_for(name)
        batches = [int(b) for b in a.batches.split(",")]
        ps_all = prompts(max(batches), a.prompt, cfg.vocab_size)
        m.generate_batch_logprobs(ps_all[:2], 4, 20, params=SamplingParams(0.6, 0.95, 20))   # warm-up
        for B in batches:
            ps = ps_all[:B]
            for sname, params in (("greedy", None), ("qwen3_default", SamplingParams(0.6, 0.95, 20))):
                base_step = None
                call = Call(m, ps, params, a.max_new)
                for setting in ("mm", "none", 0, 5, 20):
                    def run(n):
                        return call.run(setting, n)
                    t1, _ = best(lambda: run(1), a.reps)
                    tn, out = best(lambda: run(a.max_new), a.reps)
                    assert all(int(o) == a.max_new for o in out)
                    step = (tn - t1) / (a.max_new - 1)
                    base_step = step if setting == "mm" else base_step
                    m.set_profiling(False)
                    m.set_profiling(True)
                    run(a.max_new)
                    prof = {s: m.get_profile(f"logprob_rows_stage{s}") for s in ("1", "2")}
                    m.set_profiling(False)
                    rec = {"model": name, "B": B, "sampler": sname, "top_logprobs": setting, "prompt": a.prompt, "max_new": a.max_new,
                           "step_ms": round(step * 1e3, 4), "decode_tok_s": round(B / step, 1), "step_vs_mm": round(step / base_step, 4)}
                    for s, p in prof.items():
                        rec[f"stage{s}_launches"] = int(p["launches"])
                        rec[f"stage{s}_us_per_step"] = round(p["ms"] * 1e3 / p["launches"], 2) if p["launches"] else 0.0
                    print(json.dumps(rec), flush=True)
        m.close()
        import torch
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
