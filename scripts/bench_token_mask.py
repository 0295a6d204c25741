"""What a per-step allowed-token mask (aha_hip_generate_batch_masked) costs per decode step, against generate_batch_mm on the same
prompts and sampler, at the Qwen3-0.6B and Qwen3-VL-8B text dimensions of bench_generate_batch.py (seeded random weights, no stop tokens:
every sequence runs to max_new).

Per model, sequence count (--batches), sampler (greedy / the Qwen3 default request) and variant:
    none      no constraint (the entry itself: must cost nothing)
    zero      a constraint that answers "no mask" every step (the callback alone)
    static    one mask per sequence, about 40 % allowed, handed over again every step
    changing  a different mask per sequence and step (8 precomputed masks per sequence taken in turn, so no mask-building time is measured)
the decode step time (t(max_new) - t(1)) / (max_new - 1) and tok/s of the masked call and of generate_batch_mm, measured alternately
--repeats times in this one process (the spread is reported), then one profiled call: us per sample_rows_stage1 launch and the mask bytes
uploaded per step (callback answers that carried a mask x ceil(V / 32) x 4).  One JSON object per line.  The `none` rows against the same
rows of an earlier commit are the check that nothing existing slowed down.
    python scripts/bench_token_mask.py [--only 0.6b,8b] [--batches 1,16,64] [--max-new 512] [--repeats 2]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from bench_generate_batch import model_for, prompts, timed

VARIANTS = ("none", "zero", "static", "changing")


class Constraint:
    def __init__(self, name, n_seqs, vocab):
        from aha_amd.guided import pack_mask
        self.name, self.answers = name, 0
        n = {"static": 1, "changing": 8}.get(name, 0)
        g = np.random.default_rng(7)
        self.masks = [[pack_mask(np.flatnonzero(g.random(vocab) < 0.4).tolist(), vocab) for _ in range(n)] for _ in range(n_seqs if n else 0)]

    def __call__(self, seq, generated):
        if self.name == "zero":
            return None
        self.answers += 1
        ms = self.masks[seq]
        return ms[len(generated) % len(ms)]


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
    ap.add_argument("--repeats", type=int, default=2)
    a = ap.parse_args()
    from aha_amd import build
    from aha_amd.sampling import SamplingParams
    build.build()
    samplers = {"greedy": None, "qwen3": SamplingParams(0.6, 0.95, 20, 1.1, 64)}
    for name in a.only.split(","):
        cfg, m = model_for(name)
        V = cfg.vocab_size
        W = (V + 31) // 32
        ps_all = prompts(max(int(b) for b in a.batches.split(",")), a.prompt, V)
        m.generate_batch_masked(ps_all[:2], 4, Constraint("static", 2, V), samplers["qwen3"])   # warm-up
        for B in (int(b) for b in a.batches.split(",")):
            ps = ps_all[:B]
            for sname in a.samplers.split(","):
                base = samplers[sname]
                params = None if base is None else [SamplingParams(base.temperature, base.top_p, base.top_k, base.repeat_penalty,
                                                                   base.repeat_last_n, base.seed + j) for j in range(B)]
                for vname in a.variants.split(","):
                    con = None if vname == "none" else Constraint(vname, B, V)
                    msk, ref = [], []
                    for _ in range(a.repeats):   # alternated: drift hits both alike
                        ref.append(step_time(lambda n: m.generate_batch_mm(ps, None, n, params=params), a.max_new)[0])
                        s, (toks, _) = step_time(lambda n: m.generate_batch_masked(ps, n, con, params), a.max_new)
                        msk.append(s)
                    assert all(len(t) == a.max_new for t in toks)
                    if con is not None:
                        con.answers = 0
                    m.set_profiling(False)
                    m.set_profiling(True)
                    m.generate_batch_masked(ps, a.max_new, con, params)
                    prof = m.get_profile("sample_rows_stage1")
                    m.set_profiling(False)
                    n_l = max(int(prof["launches"]), 1)
                    rec = {"model": name, "B": B, "sampler": sname, "variant": vname, "max_new": a.max_new,
                           "step_ms": round(min(msk) * 1e3, 4), "step_ms_runs": [round(x * 1e3, 4) for x in msk],
                           "ref_step_ms": round(min(ref) * 1e3, 4), "ref_step_ms_runs": [round(x * 1e3, 4) for x in ref],
                           "decode_tok_s": round(B / min(msk), 1), "ref_decode_tok_s": round(B / min(ref), 1),
                           "step_vs_ref": round(min(msk) / min(ref), 4),
                           "stage1_us": round(prof["ms"] * 1e3 / n_l, 2) if prof["launches"] else None,
                           "stage1_launches": int(prof["launches"]),
                           "mask_upload_bytes_per_step": round((con.answers if con is not None else 0) * W * 4 / a.max_new, 1)}
                    print(json.dumps(rec), flush=True)
        m.close()
        import torch
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
