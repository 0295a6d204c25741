"""What logit_bias and the presence / frequency penalties (aha_hip_generate_batch_adjusted) cost per decode step, against
generate_batch_mm on the same prompts and sampler, at the Qwen3-0.6B and Qwen3-VL-8B text dimensions of bench_generate_batch.py (seeded
random weights, no stop tokens: every sequence runs to max_new).

Per model, sequence count (--batches), sampler (greedy / the Qwen3 default request) and variant:
    none      no adjust (the entry itself: must cost nothing)
    bias16 / bias300 / bias1024   a logit_bias of that many random ids, values N(0, 2)
    pen       presence 0.5 + frequency 0.5 (the list grows with every distinct generated token)
    all       bias300 + pen
the decode step time (t(max_new) - t(1)) / (max_new - 1) and tok/s of the adjusted call and of generate_batch_mm, measured alternately
--repeats times in this one process (the spread is reported), then one profiled call: us per sample_rows_stage1 launch, the addend list's
length at the last step (largest over the sequences) and the bytes of the lists uploaded per step.  One JSON object per line.
    python scripts/bench_logit_adjust.py [--only 0.6b,8b] [--batches 1,16,64] [--max-new 512] [--long 4096] [--repeats 2]
--long N: the pen and all variants are also run at max_new N (0: skip)."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from bench_generate_batch import model_for, prompts, timed

VARIANTS = ("none", "bias16", "bias300", "bias1024", "pen", "all")


def variant_params(name, base, j, vocab):
    """The SamplingParams of sequence j: `base` plus the variant's adjust (every sequence has its own bias ids)."""
    from aha_amd.sampling import SamplingParams
    g = np.random.default_rng(1000 + j)
    kw = {}
    n_bias = {"bias16": 16, "bias300": 300, "bias1024": 1024, "all": 300}.get(name, 0)
    if n_bias:
        ids = g.choice(min(vocab, 150000), size=n_bias, replace=False)
        kw["logit_bias"] = {int(i): float(v) for i, v in zip(ids, g.normal(0, 2, n_bias))}
    if name in ("pen", "all"):
        kw.update(presence_penalty=0.5, frequency_penalty=0.5)
    return SamplingParams(base.temperature, base.top_p, base.top_k, base.repeat_penalty, base.repeat_last_n, base.seed + j, **kw)


def step_time(call, max_new):
    t1, _ = timed(lambda: call(1))
    tn, out = timed(lambda: call(max_new))
    return (tn - t1) / (max_new - 1), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default="0.6b,8b")
    ap.add_argument("--batches", default="1,16,64")
    ap.add_argument("--samplers", default="greedy,qwen3")
    ap.add_argument("--variants", default=",".join(VARIANTS))
    ap.add_argument("--prompt", type=int, default=128)
    ap.add_argument("--max-new", type=int, default=512)
    ap.add_argument("--long", type=int, default=4096)
    ap.add_argument("--repeats", type=int, default=2)
    a = ap.parse_args()
    from aha_amd import build
    from aha_amd.sampling import SamplingParams
    build.build()
    samplers = {"greedy": SamplingParams(), "qwen3": SamplingParams(0.6, 0.95, 20, 1.1, 64)}
    for name in a.only.split(","):
        cfg, m = model_for(name)
        V = cfg.vocab_size
        ps_all = prompts(max(int(b) for b in a.batches.split(",")), a.prompt, V)
        m.generate_batch_adjusted(ps_all[:2], 4, variant_params("all", samplers["qwen3"], 0, V))   # warm-up
        for B in (int(b) for b in a.batches.split(",")):
            ps = ps_all[:B]
            for sname in a.samplers.split(","):
                base = samplers[sname]
                plain = [variant_params("none", base, j, V) for j in range(B)]
                for vname in a.variants.split(","):
                    for max_new in [a.max_new] + ([a.long] if a.long and vname in ("pen", "all") else []):
                        params = [variant_params(vname, base, j, V) for j in range(B)]
                        adj, ref = [], []
                        for _ in range(a.repeats):   # alternated: drift hits both alike
                            ref.append(step_time(lambda n: m.generate_batch_mm(ps, None, n, params=plain), max_new)[0])
                            s, (toks, _) = step_time(lambda n: m.generate_batch_adjusted(ps, n, params), max_new)
                            adj.append(s)
                        assert all(len(t) == max_new for t in toks)
                        m.set_profiling(False)
                        m.set_profiling(True)
                        m.generate_batch_adjusted(ps, max_new, params)
                        prof = m.get_profile("sample_rows_stage1")
                        m.set_profiling(False)
                        n_l = max(int(prof["launches"]), 1)
                        list_len = max(len(set(t[:-1]) | {i for i, b in (p.logit_bias or {}).items() if b != 0}) if p.adjust_active else 0
                                       for t, p in zip(toks, params))
                        rows_cand = B if (vname != "none" or sname != "greedy") else 0
                        rec = {"model": name, "B": B, "sampler": sname, "variant": vname, "max_new": max_new,
                               "step_ms": round(min(adj) * 1e3, 4), "step_ms_runs": [round(x * 1e3, 4) for x in adj],
                               "ref_step_ms": round(min(ref) * 1e3, 4), "ref_step_ms_runs": [round(x * 1e3, 4) for x in ref],
                               "decode_tok_s": round(B / min(adj), 1), "ref_decode_tok_s": round(B / min(ref), 1),
                               "step_vs_ref": round(min(adj) / min(ref), 4),
                               "stage1_us": round(prof["ms"] * 1e3 / n_l, 2) if prof["launches"] else None,
                               "stage1_launches": int(prof["launches"]), "list_len_last": list_len,
                               "adj_upload_bytes_per_step": round(max(prof["bytes"] / n_l - rows_cand * V * 4, 0), 1) if prof["launches"] else 0}
                        print(json.dumps(rec), flush=True)
        m.close()
        import torch
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
