"""aha_hip_score_batch (HipInferenceModel.score_batch) at Qwen3-0.6B and Qwen3-VL-8B text dimensions (seeded random weights): scored
tokens/s end to end -- host clock around the call, which ends in a synchronise, after a warm-up call -- for 16 sequences of 2048 tokens and
1 sequence of 128 tokens, and the fused kernel (ops.score_rows) against the only route the parent commit has, ops.gemm + ops.logprob_rows,
on a 2048-row chunk whose logits fit in memory, alternated three times in one process.  One JSON object per line.
    python scripts/bench_score.py [--model 0.6b|8b] [--layers N] [--reps 5]
    python scripts/bench_score.py --model 0.6b --once 16x2048   # a warm-up and one call (under rocprofv3 --kernel-trace --stats:
                                                                # score_rows_kernel's time, 2 R V K / time over the bf16 MFMA peak)
--layers: decoder layers of the model (default: the real depth); the kernel's time does not depend on it, its share of the call does."""
import argparse
import dataclasses
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

WORKLOADS = {"16x2048": (16, 2048), "1x128": (1, 128)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="0.6b", choices=["0.6b", "8b"])
    ap.add_argument("--layers", type=int, default=0)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--once", default="")
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "bench_score.py needs a GPU"
    from aha_amd import ops
    from aha_amd.configs import qwen3_0_6b, qwen3vl_8b_text
    from aha_amd.model import HipInferenceModel
    from aha_amd.weights import qwen3_text_weights
    cfg = qwen3_0_6b() if args.model == "0.6b" else dataclasses.replace(qwen3vl_8b_text(), mrope_section=None)
    if args.layers:
        cfg = dataclasses.replace(cfg, num_hidden_layers=args.layers)
    m = HipInferenceModel(cfg, qwen3_text_weights(cfg, seed=0))
    g = np.random.default_rng(0)

    def prompts(name):
        n, L = WORKLOADS[name]
        return [g.integers(0, cfg.vocab_size, size=L).astype(np.uint32).tolist() for _ in range(n)]

    if args.once:
        p = prompts(args.once)
        m.score_batch(p)
        m.score_batch(p)
        m.close()
        return
    for name in WORKLOADS:
        p = prompts(name)
        m.score_batch(p)
        ts = []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            m.score_batch(p)
            ts.append(time.perf_counter() - t0)
        n = sum(len(x) - 1 for x in p)
        print(json.dumps({"model": args.model, "layers": cfg.num_hidden_layers, "workload": name, "scored_tokens": n,
                          "ms_median": 1e3 * float(np.median(ts)), "ms_min": 1e3 * min(ts), "ms_max": 1e3 * max(ts),
                          "tokens_per_s": n / float(np.median(ts))}), flush=True)
    m.close()
    # the fused kernel against gemm + logprob_rows on 2048 rows (device tensors in, results on the host out, both ways)
    R, V, K = 2048, cfg.vocab_size, cfg.hidden_size
    tg = torch.Generator().manual_seed(0)
    h = torch.randn(R, K, generator=tg).bfloat16().cuda()
    W = (torch.randn(V, K, generator=tg) / K ** 0.5).bfloat16().cuda()
    t = np.random.default_rng(1).integers(0, V, size=R)

    def fused():
        return ops.score_rows(h, W, t)

    def unfused():
        return ops.logprob_rows(ops.gemm(h, W).float(), t, 0)

    def timed(f):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        f()
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0)

    a, b = fused(), unfused()
    dev = float(np.abs(a[0] - b[0]).max())
    rounds = [(timed(fused), timed(unfused)) for _ in range(3)]
    print(json.dumps({"model": args.model, "rows": R, "V": V, "K": K, "fused_ms": [r[0] for r in rounds], "gemm_logprob_rows_ms": [r[1] for r in rounds],
                      "max_abs_logprob_difference": dev, "fused_tflops": [2e-9 * R * V * K / r[0] for r in rounds]}), flush=True)


if __name__ == "__main__":
    main()
