"""The wide batched matvec (gemv_rows_wide_kernel: 33 .. 128 rows in one pass over the weights) against the groups of 32 it replaces.

Per matrix (the five projection shapes of Qwen3-0.6B and Qwen3-VL-8B text, the three weight forms, R in 48 / 64 / 96 / 128, the model's
epilogue for each matrix): one op-level call with R rows against the same rows in calls of at most 32.  Host timers see the entries'
per-call allocation and synchronise, so kernel time comes from a rocprofv3 kernel trace of --once:
    rocprofv3 --kernel-trace --output-format csv -d DIR -- python scripts/bench_gemv_rows_wide.py --once --plan-out DIR/plan.json
    python scripts/bench_gemv_rows_wide.py --trace-csv DIR --plan DIR/plan.json          # no GPU: one JSON line per (model, matrix, form, R)
--once walks (repeat, R, path, matrix) with the matrix innermost, so two calls on one matrix have every other matrix of the model (the
lm_head among them) streamed in between, and writes the call sequence; --trace-csv sums the matvec and merge kernels of each call in that
order (argmax excluded) and applies the project's rule: wide wins iff its p90 is below the groups' p10, or its max below their min.

End to end, one fresh process per figure (alternate the switch from a shell loop):
    python scripts/bench_gemv_rows_wide.py --e2e 8b:64 --switch 0|1|2 [--format mxfp8|mxfp4] [--draft 7]
prints the decode step ms of generate_batch (or, with --draft, generate_batch_spec fed its own output as the prediction), taken as
(t(max_new) - t(1)) / (max_new - 1), the median of --reps calls."""
import argparse
import csv
import glob
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

ROWS = (48, 64, 96, 128)
FORMS = ("bf16", "mxfp8", "mxfp4")
EPI = {"qkv": 0, "o_proj": 1, "gate_up": 2, "down": 1, "lm_head": 3}


def shapes_of(name):
    from aha_amd.configs import qwen3_0_6b, qwen3vl_8b_text
    cfg = qwen3_0_6b() if name == "0.6b" else qwen3vl_8b_text()
    H, I, V = cfg.hidden_size, cfg.intermediate_size, cfg.vocab_size
    q, kv = cfg.num_attention_heads * 128, cfg.num_key_value_heads * 128
    return {"qkv": (q + 2 * kv, H), "o_proj": (H, q), "gate_up": (2 * I, H), "down": (H, I), "lm_head": (V, H)}


def sequence(models, reps):
    """The calls of --once in launch order: (model, matrix, form, R, path, kernels of the call that the trace sums)."""
    return [(mo, s, f, R, path, 2 if path == "wide" else 2 * ((R + 31) // 32))
            for mo in models for f in FORMS for _ in range(reps) for R in ROWS for path in ("wide", "groups") for s in EPI]


def run_once(models, reps, plan_out):
    import torch
    from aha_amd import ops
    for mo in models:
        shp = shapes_of(mo)
        W = {s: torch.empty(N, K, device="cuda", dtype=torch.bfloat16).normal_(0, 0.02) for s, (N, K) in shp.items()}
        x = {s: torch.randn(128, K, device="cuda", dtype=torch.bfloat16) for s, (N, K) in shp.items()}
        res = {s: torch.randn(128, N, device="cuda", dtype=torch.bfloat16) for s, (N, K) in shp.items() if EPI[s] == 1}
        for f in FORMS:
            if f == "bf16":
                call = {s: (lambda xs, e, r, w=W[s]: ops.gemv_rows(w, xs, e, r)) for s in shp}
            else:
                quant, run = (ops.quantize_mxfp8, ops.gemv_rows_mxfp8) if f == "mxfp8" else (ops.quantize_mxfp4, ops.gemv_rows_mxfp4)
                qs = {s: quant(W[s])[:2] for s in shp}
                call = {s: (lambda xs, e, r, q=qs[s], run=run: run(q[0], q[1], xs, e, r)) for s in shp}
            for _ in range(reps):
                for R in ROWS:
                    for path in ("wide", "groups"):
                        for s in EPI:
                            for r0 in range(0, R, R if path == "wide" else 32):
                                r1 = min(R, r0 + (R if path == "wide" else 32))
                                call[s](x[s][r0:r1], EPI[s], res[s][r0:r1] if EPI[s] == 1 else None)
            del call
        torch.cuda.synchronize()
        del W, x, res
        torch.cuda.empty_cache()
    if plan_out:
        json.dump({"models": models, "reps": reps}, open(plan_out, "w"))


def from_trace(trace_dir, plan):
    p = json.load(open(plan))
    files = sorted(glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True))
    assert files, f"no *kernel_trace.csv under {trace_dir}"
    rows = [r for r in csv.DictReader(open(files[0])) if "gemv_rows" in r["Kernel_Name"]]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    seq = sequence(p["models"], p["reps"])
    assert len(rows) == sum(c[5] for c in seq), (len(rows), sum(c[5] for c in seq))
    acc, i = {}, 0
    for mo, s, f, R, path, n in seq:
        ks = rows[i:i + n]
        i += n
        assert all(("wide" in r["Kernel_Name"]) == (path == "wide") for r in ks if "merge" not in r["Kernel_Name"]), (mo, s, f, R, path)
        acc.setdefault((mo, s, f, R), {}).setdefault(path, []).append(sum(int(r["End_Timestamp"]) - int(r["Start_Timestamp"]) for r in ks) / 1e3)
    for (mo, s, f, R), d in acc.items():
        w, g = np.asarray(d["wide"][1:]), np.asarray(d["groups"][1:])          # the first repeat warms up
        win = bool(np.percentile(w, 90) < np.percentile(g, 10) or w.max() < g.min())
        N, K = shapes_of(mo)[s]
        print(json.dumps({"model": mo, "shape": s, "N": N, "K": K, "form": f, "R": R, "wide_us": round(float(np.median(w)), 1),
                          "wide_min_max_us": [round(float(w.min()), 1), round(float(w.max()), 1)], "groups_us": round(float(np.median(g)), 1),
                          "groups_min_max_us": [round(float(g.min()), 1), round(float(g.max()), 1)],
                          "speedup": round(float(np.median(g) / np.median(w)), 3), "win": win}))


def e2e(a):
    import torch
    from aha_amd.speculative import SpecConfig
    from bench_generate_batch import model_for, prompts, timed
    name, B = a.e2e.split(":")
    cfg, m = model_for(name)
    if a.format:
        m.quantize_weights(a.format, lm_head=True)
    m.debug_rows_wide(a.switch)
    ps = prompts(int(B), a.prompt, cfg.vocab_size)
    if a.draft:
        pred = m.generate_batch(ps, a.max_new)
        gen = lambda n: m.generate_batch_spec(ps, n, spec=SpecConfig(max_draft=a.draft), predictions=pred)
    else:
        gen = lambda n: m.generate_batch(ps, n)
    gen(2)
    steps = []
    for _ in range(a.reps):
        t1, _ = timed(lambda: gen(1))
        tn, _ = timed(lambda: gen(a.max_new))
        steps.append((tn - t1) / (a.max_new - 1) * 1e3)
    torch.cuda.synchronize()
    print(json.dumps({"model": name, "B": int(B), "format": a.format or "bf16", "draft": a.draft, "switch": a.switch, "prompt": a.prompt,
                      "max_new": a.max_new, "step_ms": round(float(np.median(steps)), 3), "step_ms_all": [round(s, 3) for s in steps]}), flush=True)
    m.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--once", action="store_true")
    ap.add_argument("--only", default="0.6b,8b")
    ap.add_argument("--reps", type=int, default=6)
    ap.add_argument("--plan-out", default="")
    ap.add_argument("--trace-csv", default="")
    ap.add_argument("--plan", default="")
    ap.add_argument("--e2e", default="")
    ap.add_argument("--switch", type=int, default=1)
    ap.add_argument("--format", default="")
    ap.add_argument("--draft", type=int, default=0)
    ap.add_argument("--prompt", type=int, default=128)
    ap.add_argument("--max-new", type=int, default=64)
    a = ap.parse_args()
    if a.trace_csv:
        return from_trace(a.trace_csv, a.plan)
    from aha_amd import build
    build.build()
    if a.e2e:
        return e2e(a)
    if a.once:
        return run_once(a.only.split(","), a.reps, a.plan_out)
    ap.error("one of --once, --trace-csv, --e2e")


if __name__ == "__main__":
    main()
