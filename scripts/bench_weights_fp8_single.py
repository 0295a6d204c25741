"""Single-sequence decode from MXFP8 weight copies (gemv_mxfp8_kernel) against the bf16 matvec on the same model's dequantised weights, at
Qwen3-0.6B and Qwen3-VL-8B text dimensions (seeded random weights generated on the GPU, no stop tokens).  One process per model:
    python scripts/bench_weights_fp8_single.py --only 8b [--prompt 128] [--max-new 64]
quantises the model (layer matrices and lm_head) and alternates aha_hip_debug_fp8_single off / on (1: the plan's choice of matrices; --all:
2, every matrix) three times each.  One JSON object per line: decode step ms -- (t(max_new) - t(1)) / (max_new - 1) over forward_initial + decode_greedy calls -- and tok/s of each leg, the spread
of the off runs, whether FP8's slowest run beats bf16's fastest, the HBM fraction of the gemv / gemv_fp8 profile classes (bytes the class
must move over its HIP-event time, against 8 TB/s), and the plan (R, U, grid, form) of every matrix.
    python scripts/bench_weights_fp8_single.py --once 8b            # one decode_greedy call per leg and nothing else (for rocprofv3
                                                                    # --kernel-trace, the program after `--`)
    python scripts/bench_weights_fp8_single.py --trace-csv DIR --once 8b   # no GPU: per-matrix kernel us of both kernels from that trace,
                                                                    # and the decision rule: FP8 wins a shape iff its p90 < bf16's p10"""
import argparse
import json
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from bench_generate_batch import HBM_PEAK, model_for, prompts, timed

EPI = {"qkv": 0, "o_proj": 1, "gate_up": 2, "down": 1, "lm_head": 3}
NORM = {"qkv": True, "o_proj": False, "gate_up": True, "down": False, "lm_head": True}


def shapes_of(cfg):
    H, I, V = cfg.hidden_size, cfg.intermediate_size, cfg.vocab_size
    q, kv = cfg.num_attention_heads * 128, cfg.num_key_value_heads * 128
    return {"qkv": (q + 2 * kv, H), "o_proj": (H, q), "gate_up": (2 * I, H), "down": (H, I), "lm_head": (V, H)}


def cfg_of(name):
    from aha_amd.configs import qwen3_0_6b, qwen3vl_8b_text
    return qwen3_0_6b() if name == "0.6b" else qwen3vl_8b_text()


def run(m, ids, new):
    m.clear_cache()
    _, tok = m.forward_initial(ids, 0, want_logits=False)
    t, out = timed(lambda: m.decode_greedy(tok, len(ids), new))
    assert len(out) == new
    return t


def step_time(m, ids, max_new):
    return (run(m, ids, max_new) - run(m, ids, 1)) / (max_new - 1)


def class_profile(m, ids, max_new):
    m.clear_cache()
    _, tok = m.forward_initial(ids, 0, want_logits=False)
    m.set_profiling(True)
    m.decode_greedy(tok, len(ids), max_new)
    out = {c: m.get_profile(c) for c in ("gemv", "gemv_fp8")}
    m.set_profiling(False)
    return out


def trace_report(path, name):
    """Per matrix, kernel times of gemv_kernel and gemv_mxfp8_kernel launches in a rocprofv3 kernel trace of --once.  A launch is told
    apart by its epilogue (a template argument in the kernel's name) and, for the two residual matvecs, by the dynamic LDS it asks for
    (the activation image: 4 K + 64 bytes; o_proj and down alternate where the trace has no such column)."""
    import csv
    import glob
    shapes = shapes_of(cfg_of(name))
    files = glob.glob(os.path.join(path, "**", "*kernel_trace.csv"), recursive=True)
    assert files, f"no *kernel_trace.csv under {path}"
    acc, flip = {}, {"bf16": 0, "fp8": 0}
    for r in csv.DictReader(open(files[0])):
        kn = r["Kernel_Name"]
        m = re.search(r"gemv_(mxfp8_)?kernel<(\d+), (\d+), (\d+)", kn) or re.search(r"gemv_(mxfp8_)?kernelILi(\d+)ELi(\d+)ELi(\d+)E", kn)
        if not m or "gemv_rows" in kn:
            continue
        leg, epi = "fp8" if m.group(1) else "bf16", int(m.group(4))
        if epi == 1:
            lds = next((int(r[c]) for c in ("LDS_Block_Size", "Group_Segment_Size", "LDS_Block_Size_v") if c in r and r[c]), None)
            if lds:
                sname = min(("o_proj", "down"), key=lambda s: abs(shapes[s][1] * 4 + 64 - lds))
            else:
                sname = ("o_proj", "down")[flip[leg] & 1]
                flip[leg] += 1
        else:
            sname = {0: "qkv", 2: "gate_up", 3: "lm_head"}.get(epi)
        if sname is None:
            continue
        acc.setdefault((sname, leg), []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    for sname, (N, K) in shapes.items():
        b, f = acc.get((sname, "bf16"), []), acc.get((sname, "fp8"), [])
        if not b or not f:
            continue
        mb, mf = float(np.mean(b)), float(np.mean(f))
        print(json.dumps({"trace": "kernel", "model": name, "shape": sname, "N": N, "K": K, "bf16_launches": len(b), "fp8_launches": len(f),
                          "bf16_us": round(mb, 2), "bf16_p10_p90_us": [round(float(np.percentile(b, 10)), 2), round(float(np.percentile(b, 90)), 2)],
                          "fp8_us": round(mf, 2), "fp8_p10_p90_us": [round(float(np.percentile(f, 10)), 2), round(float(np.percentile(f, 90)), 2)],
                          "speedup": round(mb / mf, 3), "win": bool(np.percentile(f, 90) < np.percentile(b, 10)),
                          "bf16_hbm_frac": round(N * K * 2 / (mb * 1e-6) / HBM_PEAK, 3),
                          "fp8_hbm_frac": round(N * K * (1 + 1 / 32) / (mf * 1e-6) / HBM_PEAK, 3)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default="8b")
    ap.add_argument("--prompt", type=int, default=128)
    ap.add_argument("--max-new", type=int, default=64)
    ap.add_argument("--all", action="store_true")
    ap.add_argument("--once", default="")
    ap.add_argument("--trace-csv", default="")
    a = ap.parse_args()
    if a.trace_csv:
        trace_report(a.trace_csv, a.once or "8b")
        return
    import torch
    from aha_amd import build, ops
    build.build()
    if a.once:
        cfg, m = model_for(a.once)
        ids = prompts(1, a.prompt, cfg.vocab_size)[0]
        m.quantize_weights("mxfp8", lm_head=True)
        for on in (0, 2):   # every matrix on the bf16 kernel, then every matrix on the FP8 kernel, whatever the plan says
            m.debug_fp8_single(on)
            run(m, ids, a.max_new)
        torch.cuda.synchronize()
        m.close()
        return
    for name in a.only.split(","):
        cfg, m = model_for(name)
        ids = prompts(1, a.prompt, cfg.vocab_size)[0]
        m.quantize_weights("mxfp8", lm_head=True)
        mode = 2 if a.all else 1
        for on in (0, mode):   # warm-up of both kernels
            m.debug_fp8_single(on)
            run(m, ids, 8)
        off, on_ = [], []
        for _ in range(3):
            m.debug_fp8_single(False)
            off.append(step_time(m, ids, a.max_new))
            m.debug_fp8_single(mode)
            on_.append(step_time(m, ids, a.max_new))
        m.debug_fp8_single(False)
        pb = class_profile(m, ids, a.max_new)["gemv"]
        steps = pb["launches"] / (4 * cfg.num_hidden_layers + 1)   # every matvec of the off leg is a gemv launch
        m.debug_fp8_single(mode)
        both = class_profile(m, ids, a.max_new)
        pf, rest = both["gemv_fp8"], both["gemv"]
        b, f = float(np.median(off)), float(np.median(on_))
        print(json.dumps({"model": name, "fp8_on": "every matrix" if a.all else "by plan", "prompt": a.prompt, "max_new": a.max_new,
                          "bf16_step_ms": round(b * 1e3, 3), "bf16_step_ms_runs": [round(t * 1e3, 3) for t in off],
                          "bf16_spread_ms": round((max(off) - min(off)) * 1e3, 3),
                          "fp8_step_ms": round(f * 1e3, 3), "fp8_step_ms_runs": [round(t * 1e3, 3) for t in on_],
                          "bf16_tok_s": round(1 / b, 1), "fp8_tok_s": round(1 / f, 1), "speedup": round(b / f, 3),
                          "step_drops": bool(max(on_) < min(off)),
                          "gemv_ms_per_step": round(pb["ms"] / steps, 3), "fp8_leg_gemv_fp8_launches_per_step": round(pf["launches"] / steps, 1),
                          "fp8_leg_gemv_launches_per_step": round(rest["launches"] / steps, 1), "fp8_leg_gemv_ms_per_step": round(rest["ms"] / steps, 3),
                          "gemv_hbm_frac": round(pb["bytes"] / (pb["ms"] * 1e-3) / HBM_PEAK, 3),
                          "gemv_fp8_ms_per_step": round(pf["ms"] / steps, 3),
                          "gemv_fp8_hbm_frac": round(pf["bytes"] / (pf["ms"] * 1e-3) / HBM_PEAK, 3)}), flush=True)
        for sname, (N, K) in shapes_of(cfg).items():
            r, u, grid, form = ops.plan_gemv_mxfp8(N, K, EPI[sname], NORM[sname])
            print(json.dumps({"model": name, "shape": sname, "N": N, "K": K, "by_plan": ops.gemv_mxfp8_by_plan(N, K, EPI[sname]), "R": r, "U": u, "grid": grid,
                              "form": ("general", "FAST", "FAST straight-line", "FAST straight-line + norm")[form]}), flush=True)
        m.close()
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
