"""Single-sequence decode from MXFP8 or MXFP4 weight copies (gemv_mxfp8_kernel / gemv_mxfp4_kernel) against the bf16 matvec on the same model's dequantised weights, at
Qwen3-0.6B and Qwen3-VL-8B text dimensions (seeded random weights generated on the GPU, no stop tokens).  One process per model:
    python scripts/bench_weights_fp8_single.py --only 8b [--prompt 128] [--max-new 64]
quantises the model (layer matrices and lm_head) and alternates aha_hip_debug_fp8_single off / on (1: the plan's choice of matrices; --all:
2, every matrix) three times each.  One JSON object per line: decode step ms -- (t(max_new) - t(1)) / (max_new - 1) over forward_initial + decode_greedy calls -- and tok/s of each leg, the spread
of the off runs, whether FP8's slowest run beats bf16's fastest, the HBM fraction of the gemv / gemv_fp8 profile classes (bytes the class
must move over its HIP-event time, against 8 TB/s), and the plan (R, U, grid, form) of every matrix.
    python scripts/bench_weights_fp8_single.py --once 8b            # one decode_greedy call per leg and nothing else (for rocprofv3
                                                                    # --kernel-trace, the program after `--`)
    python scripts/bench_weights_fp8_single.py --trace-csv DIR --once 8b   # no GPU: per-matrix kernel us of both kernels from that trace,
                                                                    # and the decision rule: FP8 wins a shape iff its p90 < bf16's p10
--format mxfp4 (default mxfp8) runs all of the above with MXFP4 copies, gemv_mxfp4_kernel and aha_hip_debug_fp4_single: the keys read
fp4_* and the class is gemv_fp4.  With it, the timed run also reports the step of an MXFP8 model (by its plan) measured in the same
process, for information."""
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
# per --format: key prefix, profile class, kernel name in a trace, bytes per weight, the model's switch, the plan queries
FORMATS = {"mxfp8": {"tag": "fp8", "cls": "gemv_fp8", "kernel": "mxfp8_", "bpw": 1 + 1 / 32, "switch": "debug_fp8_single",
                     "plan": "plan_gemv_mxfp8", "by_plan": "gemv_mxfp8_by_plan"},
           "mxfp4": {"tag": "fp4", "cls": "gemv_fp4", "kernel": "mxfp4_", "bpw": 0.5 + 1 / 32, "switch": "debug_fp4_single",
                     "plan": "plan_gemv_mxfp4", "by_plan": "gemv_mxfp4_by_plan"}}


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


def class_profile(m, ids, max_new, cls):
    m.clear_cache()
    _, tok = m.forward_initial(ids, 0, want_logits=False)
    m.set_profiling(True)
    m.decode_greedy(tok, len(ids), max_new)
    out = {c: m.get_profile(c) for c in ("gemv", cls)}
    m.set_profiling(False)
    return out


def trace_report(path, name, F):
    """Per matrix, kernel times of gemv_kernel and gemv_mxfp8_kernel (--format mxfp4: gemv_mxfp4_kernel) launches in a rocprofv3 kernel trace of --once.  A launch is told
    apart by its epilogue (a template argument in the kernel's name) and, for the two residual matvecs, by the dynamic LDS it asks for
    (the activation image: 4 K + 64 bytes; o_proj and down alternate where the trace has no such column)."""
    import csv
    import glob
    shapes = shapes_of(cfg_of(name))
    files = glob.glob(os.path.join(path, "**", "*kernel_trace.csv"), recursive=True)
    assert files, f"no *kernel_trace.csv under {path}"
    tag = F["tag"]
    acc, flip = {}, {"bf16": 0, tag: 0}
    for r in csv.DictReader(open(files[0])):
        kn = r["Kernel_Name"]
        m = re.search(r"gemv_(%s)?kernel<(\d+), (\d+), (\d+)" % F["kernel"], kn) or re.search(r"gemv_(%s)?kernelILi(\d+)ELi(\d+)ELi(\d+)E" % F["kernel"], kn)
        if not m or "gemv_rows" in kn:
            continue
        leg, epi = tag if m.group(1) else "bf16", int(m.group(4))
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
        b, f = acc.get((sname, "bf16"), []), acc.get((sname, tag), [])
        if not b or not f:
            continue
        mb, mf = float(np.mean(b)), float(np.mean(f))
        print(json.dumps({"trace": "kernel", "model": name, "shape": sname, "N": N, "K": K, "bf16_launches": len(b), tag + "_launches": len(f),
                          "bf16_us": round(mb, 2), "bf16_p10_p90_us": [round(float(np.percentile(b, 10)), 2), round(float(np.percentile(b, 90)), 2)],
                          tag + "_us": round(mf, 2), tag + "_p10_p90_us": [round(float(np.percentile(f, 10)), 2), round(float(np.percentile(f, 90)), 2)],
                          "speedup": round(mb / mf, 3), "win": bool(np.percentile(f, 90) < np.percentile(b, 10)),
                          "bf16_hbm_frac": round(N * K * 2 / (mb * 1e-6) / HBM_PEAK, 3),
                          tag + "_hbm_frac": round(N * K * F["bpw"] / (mf * 1e-6) / HBM_PEAK, 3)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default="8b")
    ap.add_argument("--prompt", type=int, default=128)
    ap.add_argument("--max-new", type=int, default=64)
    ap.add_argument("--all", action="store_true")
    ap.add_argument("--once", default="")
    ap.add_argument("--trace-csv", default="")
    ap.add_argument("--format", default="mxfp8", choices=sorted(FORMATS))
    a = ap.parse_args()
    F = FORMATS[a.format]
    tag = F["tag"]
    if a.trace_csv:
        trace_report(a.trace_csv, a.once or "8b", F)
        return
    import torch
    from aha_amd import build, ops
    build.build()
    if a.once:
        cfg, m = model_for(a.once)
        ids = prompts(1, a.prompt, cfg.vocab_size)[0]
        m.quantize_weights(a.format, lm_head=True)
        for on in (0, 2):   # every matrix on the bf16 kernel, then every matrix on the quantised format's kernel, whatever the plan says
            getattr(m, F["switch"])(on)
            run(m, ids, a.max_new)
        torch.cuda.synchronize()
        m.close()
        return
    for name in a.only.split(","):
        cfg, m = model_for(name)
        ids = prompts(1, a.prompt, cfg.vocab_size)[0]
        m.quantize_weights(a.format, lm_head=True)
        switch = getattr(m, F["switch"])
        mode = 2 if a.all else 1
        for on in (0, mode):   # warm-up of both kernels
            switch(on)
            run(m, ids, 8)
        off, on_ = [], []
        for _ in range(3):
            switch(0)
            off.append(step_time(m, ids, a.max_new))
            switch(mode)
            on_.append(step_time(m, ids, a.max_new))
        switch(0)
        pb = class_profile(m, ids, a.max_new, F["cls"])["gemv"]
        steps = pb["launches"] / (4 * cfg.num_hidden_layers + 1)   # every matvec of the off leg is a gemv launch
        switch(mode)
        both = class_profile(m, ids, a.max_new, F["cls"])
        pf, rest = both[F["cls"]], both["gemv"]
        b, f = float(np.median(off)), float(np.median(on_))
        line = {"model": name, tag + "_on": "every matrix" if a.all else "by plan", "prompt": a.prompt, "max_new": a.max_new,
                "bf16_step_ms": round(b * 1e3, 3), "bf16_step_ms_runs": [round(t * 1e3, 3) for t in off],
                "bf16_spread_ms": round((max(off) - min(off)) * 1e3, 3),
                tag + "_step_ms": round(f * 1e3, 3), tag + "_step_ms_runs": [round(t * 1e3, 3) for t in on_],
                "bf16_tok_s": round(1 / b, 1), tag + "_tok_s": round(1 / f, 1), "speedup": round(b / f, 3),
                "step_drops": bool(max(on_) < min(off)),
                "gemv_ms_per_step": round(pb["ms"] / steps, 3), f"{tag}_leg_{F['cls']}_launches_per_step": round(pf["launches"] / steps, 1),
                tag + "_leg_gemv_launches_per_step": round(rest["launches"] / steps, 1), tag + "_leg_gemv_ms_per_step": round(rest["ms"] / steps, 3),
                "gemv_hbm_frac": round(pb["bytes"] / (pb["ms"] * 1e-3) / HBM_PEAK, 3),
                F["cls"] + "_ms_per_step": round(pf["ms"] / steps, 3),
                F["cls"] + "_hbm_frac": round(pf["bytes"] / (pf["ms"] * 1e-3) / HBM_PEAK, 3) if pf["ms"] else None}
        m.close()
        torch.cuda.empty_cache()
        if a.format == "mxfp4":   # for information: the step of the same weights as an MXFP8 model, by its plan, in the same process
            cfg, m8 = model_for(name)
            m8.quantize_weights("mxfp8", lm_head=True)
            run(m8, ids, 8)
            t8 = [step_time(m8, ids, a.max_new) for _ in range(3)]
            line["mxfp8_model_step_ms"] = round(float(np.median(t8)) * 1e3, 3)
            line["mxfp8_model_step_ms_runs"] = [round(t * 1e3, 3) for t in t8]
            m8.close()
            torch.cuda.empty_cache()
        print(json.dumps(line), flush=True)
        for sname, (N, K) in shapes_of(cfg).items():
            r, u, grid, form = getattr(ops, F["plan"])(N, K, EPI[sname], NORM[sname])
            print(json.dumps({"model": name, "shape": sname, "N": N, "K": K, "by_plan": getattr(ops, F["by_plan"])(N, K, EPI[sname]), "R": r, "U": u, "grid": grid,
                              "form": ("general", "FAST", "FAST straight-line", "FAST straight-line + norm")[form]}), flush=True)


if __name__ == "__main__":
    main()
