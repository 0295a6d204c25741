"""Prefill from the MXFP8 copies (AHA_WQ_PREFILL: mxfp8_quantize_rows_kernel + gemm_mxfp8_kernel) against the bf16 GEMMs on the same model's
dequantised weights, at Qwen3-0.6B and Qwen3-VL-8B text dimensions (seeded random weights generated on the GPU).  One process per leg:
    python scripts/bench_prefill_fp8.py --only 8b --leg fp8 [--rows 1542,2048,8192] [--repeats 5]
builds the model, quantises it ("fp8": with the flag, "bf16": without) and prefills each row count `repeats` times after a warm-up.  One JSON
object per line and row count: prefill ms (host clock around forward_initial, which ends in a synchronise) min / median / max, and -- from a
further profiled prefill -- the HIP-event ms, TFLOP/s and share of the dense peak of the layer GEMMs' profile classes (gemm_fp8 + quant_rows
against gemm; the peak is FP8_PEAK for the fp8 leg, BF16_PEAK for bf16).  Alternate fresh processes of the two legs and compare: a win is
fp8's max below bf16's min, and an end-to-end gain is claimed only at 3 x the bf16 leg's run-to-run spread or more.
    python scripts/bench_prefill_fp8.py --only 8b --leg fp8 --once 2048    # one prefill and nothing else (for rocprofv3 --kernel-trace,
                                                                           # the program after `--`): per-launch kernel times by name
profiles/prefill_fp8.md holds what was measured."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from bench_generate_batch import model_for, prompts, timed

BF16_PEAK, FP8_PEAK = 2.5e15, 5.0e15   # dense MFMA peaks of the MI355X data sheet, FLOP/s


def prefill(m, ids):
    m.clear_cache()
    return timed(lambda: m.forward_initial(ids, 0, want_logits=False))[0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default="0.6b", choices=["0.6b", "8b"])
    ap.add_argument("--leg", default="fp8", choices=["fp8", "bf16"])
    ap.add_argument("--rows", default="1542,2048,8192")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--once", type=int, default=0)
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "bench_prefill_fp8.py needs a GPU"
    cfg, m = model_for(a.only)
    m.quantize_weights_with("mxfp8", prefill=a.leg == "fp8")
    if a.once:
        prefill(m, prompts(1, a.once, cfg.vocab_size)[0])
        return
    classes = ("gemm_fp8", "quant_rows") if a.leg == "fp8" else ("gemm",)
    for S in (int(x) for x in a.rows.split(",")):
        ids = prompts(1, S, cfg.vocab_size)[0]
        prefill(m, ids)
        t = sorted(prefill(m, ids) for _ in range(a.repeats))
        m.set_profiling(True)
        prefill(m, ids)
        prof = {c: m.get_profile(c) for c in classes + ("gemm",)}
        m.set_profiling(False)
        ms = sum(prof[c]["ms"] for c in classes)
        flops = prof[classes[0]]["flops"]
        out = {"size": a.only, "leg": a.leg, "rows": S, "prefill_ms_min": t[0] * 1e3, "prefill_ms_median": float(np.median(t)) * 1e3,
               "prefill_ms_max": t[-1] * 1e3, "layer_gemm_ms": ms, "layer_gemm_launches": prof[classes[0]]["launches"],
               "layer_gemm_tflops": flops / ms / 1e9 if ms else None,
               "share_of_dense_peak": flops / (ms * 1e-3) / (FP8_PEAK if a.leg == "fp8" else BF16_PEAK) if ms else None}
        if a.leg == "fp8":
            out["quant_rows_ms"] = prof["quant_rows"]["ms"]
            out["other_gemm_ms"] = prof["gemm"]["ms"]   # lm_head and whatever else stays on bf16
        print(json.dumps(out), flush=True)
    m.close()


if __name__ == "__main__":
    main()
