"""Serial embed_one against packed embed_batch at Qwen3-Embedding-0.6B dimensions (configs.qwen3_0_6b, seeded random weights).
Per workload: median of --reps timed repeats after one warm-up, as texts/s and tokens/s, and the speed-up; every timed output of the two
paths is checked against each other: cosine >= 0.9995 per row (the oracle bound of tests/test_embed_batch_gpu.py), unit norm to 1e-5.
At 28 layers the two paths differ by more than the tiny test models' 0.9999: a GEMM of M = 8192 packed rows runs another tile plan (another
k order) than one of M = 32.  The 256x32 workload therefore also runs embed_batch with one text per pass (M = 32, the serial plans) and
reports its largest difference to the serial outputs, which isolates that effect.
    python scripts/bench_embed.py [--reps 5] [--only 256x32,mixed] [--json out.jsonl]
    python scripts/bench_embed.py --once 256x32     # one embed_batch call and nothing else (under rocprofv3 --kernel-trace --stats)"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

WORKLOADS = {"256x32": (256, 32), "64x128": (64, 128), "32x512": (32, 512), "8x2048": (8, 2048), "mixed": (128, None)}


def texts(name, vocab, seed=0):
    n, L = WORKLOADS[name]
    g = np.random.default_rng(seed)
    lens = [L] * n if L else [int(x) for x in g.integers(1, 1001, size=n)]   # mixed: lengths uniform in 1 .. 1000
    return [g.integers(0, vocab, size=k).astype(np.uint32).tolist() for k in lens]


def check(serial, batched, name):
    cos = (serial * batched).sum(-1) / (np.linalg.norm(serial, axis=-1) * np.linalg.norm(batched, axis=-1))
    nrm = np.abs(np.linalg.norm(batched, axis=-1) - 1.0)
    if not (cos.min() >= 0.9995 and nrm.max() < 1e-5):
        FAILED.append(f"{name}: batched and serial disagree (min cosine {cos.min():.6f}, max |norm - 1| {nrm.max():.2e})")
        print(FAILED[-1], flush=True)
    return float(cos.min())


FAILED = []


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--only", default="")
    ap.add_argument("--once", default="")
    ap.add_argument("--json", default="")
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "bench_embed.py needs a GPU"
    from aha_amd.configs import qwen3_0_6b
    from aha_amd.model import HipInferenceModel
    from aha_amd.weights import qwen3_text_weights
    cfg = qwen3_0_6b()
    m = HipInferenceModel(cfg, qwen3_text_weights(cfg, seed=0))
    if args.once:
        m.embed_batch(texts(args.once, cfg.vocab_size))
        m.close()
        return
    names = [x for x in args.only.split(",") if x] or list(WORKLOADS)
    rows = []
    for name in names:
        seqs = texts(name, cfg.vocab_size)
        ntok = sum(len(s) for s in seqs)
        check(np.stack([m.embed_one(s) for s in seqs]), m.embed_batch(seqs), name)   # warm-up of both paths
        same_plan = None
        if name == "256x32":   # one text per pass: the serial GEMM plans
            same_plan = float(np.abs(m.embed_batch(seqs, max_tokens_per_pass=32) - np.stack([m.embed_one(s) for s in seqs])).max())
        ts, tb, worst = [], [], 1.0
        for _ in range(args.reps):   # alternate the two paths so that drift of the box shows in both
            t0 = time.perf_counter()
            serial = np.stack([m.embed_one(s) for s in seqs])
            t1 = time.perf_counter()
            batched = m.embed_batch(seqs)
            t2 = time.perf_counter()
            ts.append(t1 - t0)
            tb.append(t2 - t1)
            worst = min(worst, check(serial, batched, name))
        s_med, b_med = float(np.median(ts)), float(np.median(tb))
        r = {"workload": name, "texts": len(seqs), "tokens": ntok, "serial_ms": s_med * 1e3, "batched_ms": b_med * 1e3,
             "serial_texts_s": len(seqs) / s_med, "batched_texts_s": len(seqs) / b_med, "serial_tokens_s": ntok / s_med,
             "batched_tokens_s": ntok / b_med, "speedup": s_med / b_med, "min_cosine": worst, "reps": args.reps}
        if same_plan is not None:
            r["one_text_per_pass_max_abs_diff"] = same_plan
        rows.append(r)
        print(json.dumps(r), flush=True)
    m.close()
    print("| workload | texts | tokens | serial ms | batched ms | serial texts/s | batched texts/s | batched tokens/s | speed-up |")
    print("|---|---:|---:|---:|---:|---:|---:|---:|---:|")
    for r in rows:
        print(f"| {r['workload']} | {r['texts']} | {r['tokens']} | {r['serial_ms']:.2f} | {r['batched_ms']:.2f} | {r['serial_texts_s']:.0f} | "
              f"{r['batched_texts_s']:.0f} | {r['batched_tokens_s']:.0f} | {r['speedup']:.2f}x |")
    if args.json:
        with open(args.json, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")
    if FAILED:
        raise SystemExit("; ".join(FAILED[:3]))


if __name__ == "__main__":
    main()
