"""Batched decode from MXFP8 weight copies (aha_hip_model_quantize_weights) against the bf16 weights, at Qwen3-0.6B and Qwen3-VL-8B text
dimensions (seeded random weights generated on the GPU, no stop tokens).  One model per size, one process: the bf16 legs run first on
the unquantised model (three repeats: the run-to-run spread), then the model is quantised in place (layer matrices and lm_head) and
the FP8 leg alternates with the same model's bf16 kernel on the dequantised weights (aha_hip_debug_fp8_rows: the same bits, the bf16
byte count).  One JSON object per line:
  * per batch size B: decode step ms and tok/s of each leg -- (t(max_new) - t(1)) / (max_new - 1) over generate_batch calls -- the
    bf16 spread, the FP8 speed-up, and from the in-model HIP-event profile of one call the time and HBM fraction of the matvec class
    (gemv_rows / gemv_rows_fp8: bytes the class must move over its time, against the 8 TB/s peak);
  * per projection shape and R = 1, 16, 32: the op-level gemv_rows and gemv_rows_mxfp8 calls, alternating, three blocks of --reps
    calls each.  These entries allocate their scratch and synchronise per call, so "us" is an upper bound of the kernel time and the
    two legs carry the same overhead ("overhead_us": the same call on a 32 x 128 matrix); "win" is true when the FP8 leg's slowest
    block beats the bf16 leg's fastest;
  * records: rms deviation of the quantised model's prefill logits from the unquantised model's (in units of the logits' standard
    deviation), and the extra memory of the copies.
    python scripts/bench_weights_fp8.py [--only 0.6b,8b] [--batches 1,16,32,64] [--prompt 128] [--max-new 64] [--reps 50]
    python scripts/bench_weights_fp8.py --once 8b:16     # one generate_batch call on the bf16 weights, quantise, one on the FP8 copies, and
                                                         # nothing else (for rocprofv3 --kernel-trace)
    python scripts/bench_weights_fp8.py --trace-csv DIR --once 8b:16   # no GPU: per-matrix kernel us of both matvecs from that trace
--format mxfp4 (default mxfp8) runs all of the above with MXFP4 copies: the keys read fp4_* and the class is gemv_rows_fp4.  With it,
--once runs three fresh models (bf16, MXFP8, MXFP4) so that one trace holds all three kernels, and --trace-csv adds the FP8 kernel's
figures and "win_vs_fp8" to every line.
    python scripts/bench_weights_fp8.py --three-way [--only ...] [--batches ...]   # three fresh models per size in one process, three
                                                         # alternated repeats of the bf16 / MXFP8 / MXFP4 decode step, and MXFP4's records"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from bench_generate_batch import HBM_PEAK, model_for, prompts, timed


# per --format: key prefix, profile class, kernel name in a trace, bytes per weight, op-level entries
FORMATS = {"mxfp8": {"tag": "fp8", "cls": "gemv_rows_fp8", "kernel": "gemv_rows_mxfp8_kernel", "bpw": 1 + 1 / 32,
                     "quantize": "quantize_mxfp8", "call": "aha_hip_gemv_rows_mxfp8"},
           "mxfp4": {"tag": "fp4", "cls": "gemv_rows_fp4", "kernel": "gemv_rows_mxfp4_kernel", "bpw": 0.5 + 1 / 32,
                     "quantize": "quantize_mxfp4", "call": "aha_hip_gemv_rows_mxfp4"}}


def step_time(m, ps, max_new):
    t1, _ = timed(lambda: m.generate_batch(ps, 1))
    tn, out = timed(lambda: m.generate_batch(ps, max_new))
    assert all(len(o) == max_new for o in out)
    return (tn - t1) / (max_new - 1)


def matvec_profile(m, ps, max_new):
    """ms, bytes and launches of the matvec classes in one generate_batch call (HIP events around every launch)."""
    m.set_profiling(True)
    m.generate_batch(ps, max_new)
    out = {c: m.get_profile(c) for c in ("gemv_rows", "gemv_rows_fp8", "gemv_rows_fp4")}
    m.set_profiling(False)
    return out


def bench_ops(cfg, name, reps, fmt="mxfp8"):
    import torch
    from aha_amd import ops, quant
    F = FORMATS[fmt]
    tag = F["tag"]
    H, I, V = cfg.hidden_size, cfg.intermediate_size, cfg.vocab_size
    q, kv = cfg.num_attention_heads * 128, cfg.num_key_value_heads * 128
    shapes = {"qkv": (q + 2 * kv, H), "o_proj": (H, q), "gate_up": (2 * I, H), "down": (H, I), "lm_head": (V, H)}

    def block(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(reps):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / reps

    Wt = torch.randn(32, 128, device="cuda", dtype=torch.bfloat16)
    xt = torch.randn(16, 128, device="cuda", dtype=torch.bfloat16)
    ops.gemv_rows(Wt, xt)
    overhead = min(block(lambda: ops.gemv_rows(Wt, xt)) for _ in range(3))
    for sname, (N, K) in shapes.items():
        W = torch.randn(N, K, device="cuda", dtype=torch.bfloat16) * 0.02
        gq, gs, wr = getattr(ops, F["quantize"])(W)
        words = quant.scales_to_kernel(gs).cuda()
        del W
        epi = ops.GEMV_ROWS_LOGITS if sname == "lm_head" else ops.GEMV_ROWS_STORE
        for R in (1, 16, 32):
            x = torch.randn(R, K, device="cuda", dtype=torch.bfloat16)
            y = torch.empty(R, N, device="cuda", dtype=torch.bfloat16)
            lg = torch.empty(R, N, device="cuda", dtype=torch.float32) if epi == ops.GEMV_ROWS_LOGITS else None
            am = torch.empty(R, device="cuda", dtype=torch.int32) if lg is not None else None
            st = torch.cuda.current_stream().cuda_stream
            L = ops.lib()

            def bf():
                ops.check(L.aha_hip_gemv_rows(wr.data_ptr(), x.data_ptr(), y.data_ptr(), R, N, K, epi, None, None if lg is None else lg.data_ptr(),
                                              None if am is None else am.data_ptr(), st))

            def f8():
                ops.check(getattr(L, F["call"])(gq.data_ptr(), words.data_ptr(), x.data_ptr(), y.data_ptr(), R, N, K, epi, None,
                                                None if lg is None else lg.data_ptr(), None if am is None else am.data_ptr(), st))
            bf(), f8()
            tb, tf = [], []
            for _ in range(3):
                tb.append(block(bf))
                tf.append(block(f8))
            b, f = float(np.median(tb)), float(np.median(tf))
            print(json.dumps({"kernel": "gemv_rows", "model": name, "shape": sname, "N": N, "K": K, "R": R, "overhead_us": round(overhead * 1e6, 1),
                              "bf16_us": round(b * 1e6, 1), "bf16_spread_us": round((max(tb) - min(tb)) * 1e6, 1),
                              f"{tag}_us": round(f * 1e6, 1), f"{tag}_spread_us": round((max(tf) - min(tf)) * 1e6, 1),
                              "speedup": round(b / f, 3), "win": bool(max(tf) < min(tb)),
                              "bf16_hbm_frac": round(N * K * 2 / b / HBM_PEAK, 3), f"{tag}_hbm_frac": round(N * K * F["bpw"] / f / HBM_PEAK, 3)}),
                  flush=True)
        del gq, gs, wr, words


def shapes_of(cfg):
    H, I, V = cfg.hidden_size, cfg.intermediate_size, cfg.vocab_size
    q, kv = cfg.num_attention_heads * 128, cfg.num_key_value_heads * 128
    return {"qkv": (q + 2 * kv, H), "o_proj": (H, q), "gate_up": (2 * I, H), "down": (H, I), "lm_head": (V, H)}


def plan(N, K):
    """gemv_rows_plan (csrc/kernels_batch.hip): (blocks along N, K splits) = the launch grid of both matvec kernels."""
    chunks, nb = (K + 127) // 128, (N + 31) // 32
    c = 2 if chunks > 4 else 1
    s = (chunks + 4 * c - 1) // (4 * c)
    if c == 2 and nb * s < 256:
        s = (chunks + 3) // 4
    return nb, s


def trace_report(path, name, fmt="mxfp8"):
    """Per matrix, the mean kernel time of gemv_rows_kernel and gemv_rows_mxfp8_kernel launches in a rocprofv3 kernel trace of --once,
    told apart by their grids; decode launches only (the row count of the prefill's head launch equals the decode's, so it is one more
    lm_head sample).  With fmt "mxfp4" the quantised leg is gemv_rows_mxfp4_kernel and the FP8 kernel's figures are reported beside it."""
    F = FORMATS[fmt]
    tag = F["tag"]
    import csv
    import glob
    from aha_amd.configs import qwen3_0_6b, qwen3vl_8b_text
    cfg = qwen3_0_6b() if name == "0.6b" else qwen3vl_8b_text()
    grids = {plan(N, K): (sname, N, K) for sname, (N, K) in shapes_of(cfg).items()}
    files = glob.glob(os.path.join(path, "**", "*kernel_trace.csv"), recursive=True)
    dbs = glob.glob(os.path.join(path, "**", "*_results.db"), recursive=True)
    assert files or dbs, f"no *kernel_trace.csv and no *_results.db under {path}"
    if files:
        rows = csv.DictReader(open(files[0]))
    else:   # a rocprofv3 that writes its database by default (--output-format csv gives the file above): the same columns from its view
        import sqlite3
        cur = sqlite3.connect(dbs[0]).execute('select name, workgroup_x, grid_x, grid_y, start, "end" from kernels')
        cols = ("Kernel_Name", "Workgroup_Size_X", "Grid_Size_X", "Grid_Size_Y", "Start_Timestamp", "End_Timestamp")
        rows = (dict(zip(cols, r)) for r in cur)
    acc = {}
    for r in rows:
        kn = r["Kernel_Name"]
        leg = "fp8" if "gemv_rows_mxfp8_kernel" in kn else "fp4" if "gemv_rows_mxfp4_kernel" in kn else "bf16" if "gemv_rows_kernel" in kn else None
        if leg is None:
            continue
        wg = int(r["Workgroup_Size_X"])
        gx, gy = int(r["Grid_Size_X"]), int(r["Grid_Size_Y"])
        key = (gx // wg, gy) if (gx // wg, gy) in grids else (gx, gy)   # the trace counts work-items
        if key not in grids:
            continue
        acc.setdefault((grids[key], leg), []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    for sname, N, K in grids.values():
        b, f = acc.get(((sname, N, K), "bf16"), []), acc.get(((sname, N, K), tag), [])
        if not b or not f:
            continue
        mb, mf = float(np.mean(b)), float(np.mean(f))
        line = {"trace": "kernel", "model": name, "shape": sname, "N": N, "K": K, "bf16_launches": len(b), f"{tag}_launches": len(f),
                "bf16_us": round(mb, 2), "bf16_p10_p90_us": [round(float(np.percentile(b, 10)), 2), round(float(np.percentile(b, 90)), 2)],
                f"{tag}_us": round(mf, 2), f"{tag}_p10_p90_us": [round(float(np.percentile(f, 10)), 2), round(float(np.percentile(f, 90)), 2)],
                "speedup": round(mb / mf, 3), "win": bool(np.percentile(f, 90) < np.percentile(b, 10)),
                "bf16_hbm_frac": round(N * K * 2 / (mb * 1e-6) / HBM_PEAK, 3),
                f"{tag}_hbm_frac": round(N * K * F["bpw"] / (mf * 1e-6) / HBM_PEAK, 3)}
        f8 = acc.get(((sname, N, K), "fp8"), [])
        if tag == "fp4" and f8:   # the same trace holds the FP8 kernel: FP4 wins against it when its p90 is below FP8's p10
            m8 = float(np.mean(f8))
            line.update({"fp8_launches": len(f8), "fp8_us": round(m8, 2),
                         "fp8_p10_p90_us": [round(float(np.percentile(f8, 10)), 2), round(float(np.percentile(f8, 90)), 2)],
                         "fp8_hbm_frac": round(N * K * (1 + 1 / 32) / (m8 * 1e-6) / HBM_PEAK, 3), "speedup_vs_fp8": round(m8 / mf, 3),
                         "win_vs_fp8": bool(np.percentile(f, 90) < np.percentile(f8, 10))})
        print(json.dumps(line), flush=True)


def three_way(a):
    """bf16, MXFP8 and MXFP4 decode steps of three fresh models of one size in one process, three alternated repeats per batch size."""
    import torch
    legs = (("bf16", None, "gemv_rows"), ("fp8", "mxfp8", "gemv_rows_fp8"), ("fp4", "mxfp4", "gemv_rows_fp4"))
    batches = [int(b) for b in a.batches.split(",")]
    for name in a.only.split(","):
        ms, cfg = {}, None
        for tag, fmt, _ in legs:
            cfg, m = model_for(name)
            ps_all = prompts(max(batches), a.prompt, cfg.vocab_size)
            if fmt is None:
                ref, _ = m.forward_initial(ps_all[0], 0)
            else:
                t_q, _ = timed(lambda: m.quantize_weights(fmt, lm_head=True))
                got, _ = m.forward_initial(ps_all[0], 0)
                H, I, V, L = cfg.hidden_size, cfg.intermediate_size, cfg.vocab_size, cfg.num_hidden_layers
                q, kv = cfg.num_attention_heads * 128, cfg.num_key_value_heads * 128
                elems = L * ((q + 2 * kv) * H + H * q + 2 * I * H + H * I) + V * H
                bpw = FORMATS[fmt]["bpw"]
                print(json.dumps({"model": name, "format": fmt, "quantize_s": round(t_q, 3), "quantised_GB_bf16": round(elems * 2 / 1e9, 3),
                                  "extra_GB": round(elems * bpw / 1e9, 3), "extra_over_quantised": round(bpw / 2, 4),
                                  "prefill_logits_rms_dev_std": round(float(np.sqrt(((got - ref) ** 2).mean()) / ref.std()), 5),
                                  "prefill_argmax_same": bool(int(np.argmax(got)) == int(np.argmax(ref)))}), flush=True)
            m.clear_cache()
            m.generate_batch(ps_all[:2], 4)   # warm-up
            ms[tag] = m
        for B in batches:
            ps = ps_all[:B]
            t = {tag: [] for tag, _, _ in legs}
            for _ in range(3):
                for tag, _, _ in legs:
                    t[tag].append(step_time(ms[tag], ps, a.max_new))
            line = {"model": name, "B": B, "prompt": a.prompt, "max_new": a.max_new}
            for tag, _, cls in legs:
                pr = matvec_profile(ms[tag], ps, a.max_new)[cls]
                med = float(np.median(t[tag]))
                line.update({f"{tag}_step_ms": round(med * 1e3, 3), f"{tag}_step_ms_runs": [round(x * 1e3, 3) for x in t[tag]],
                             f"{tag}_decode_tok_s": round(B / med, 1), f"{cls}_ms_per_step": round(pr["ms"] / (a.max_new - 1), 3),
                             f"{cls}_hbm_frac": round(pr["bytes"] / (pr["ms"] * 1e-3) / HBM_PEAK, 3)})
            line.update({"bf16_spread_ms": round((max(t["bf16"]) - min(t["bf16"])) * 1e3, 3),
                         "fp4_speedup_vs_bf16": round(line["bf16_step_ms"] / line["fp4_step_ms"], 3),
                         "fp4_speedup_vs_fp8": round(line["fp8_step_ms"] / line["fp4_step_ms"], 3),
                         "fp4_step_drops_vs_bf16": bool(max(t["fp4"]) < min(t["bf16"])),
                         "fp4_step_drops_vs_fp8": bool(max(t["fp4"]) < min(t["fp8"]))})
            print(json.dumps(line), flush=True)
        for m in ms.values():
            m.close()
        ms.clear()
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default="0.6b,8b")
    ap.add_argument("--batches", default="1,16,32,64")
    ap.add_argument("--prompt", type=int, default=128)
    ap.add_argument("--max-new", type=int, default=64)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--no-kernel", action="store_true")
    ap.add_argument("--once", default="")
    ap.add_argument("--trace-csv", default="")
    ap.add_argument("--format", default="mxfp8", choices=sorted(FORMATS))
    ap.add_argument("--three-way", action="store_true")
    a = ap.parse_args()
    F = FORMATS[a.format]
    tag = F["tag"]
    if a.trace_csv:
        trace_report(a.trace_csv, a.once.split(":")[0] if a.once else "8b", a.format)
        return
    import torch
    from aha_amd import build
    build.build()
    if a.once:
        name, B = a.once.split(":")
        cfg, m = model_for(name)
        ps = prompts(int(B), a.prompt, cfg.vocab_size)
        m.generate_batch(ps, a.max_new)
        if a.format == "mxfp4":   # one trace with all three kernels: a fresh model per quantised format
            for fmt in ("mxfp8", "mxfp4"):
                m.close()
                cfg, m = model_for(name)
                m.quantize_weights(fmt, lm_head=True)
                m.generate_batch(ps, a.max_new)
        else:
            m.quantize_weights("mxfp8", lm_head=True)
            m.generate_batch(ps, a.max_new)
        torch.cuda.synchronize()
        m.close()
        return
    if a.three_way:
        three_way(a)
        return
    batches = [int(b) for b in a.batches.split(",")]
    for name in a.only.split(","):
        cfg, m = model_for(name)
        ps_all = prompts(max(batches), a.prompt, cfg.vocab_size)
        m.generate_batch(ps_all[:2], 4)   # warm-up
        bf16 = {B: [step_time(m, ps_all[:B], a.max_new) for _ in range(3)] for B in batches}
        m.clear_cache()
        ref, _ = m.forward_initial(ps_all[0], 0)
        m.clear_cache()
        prof_bf = {B: matvec_profile(m, ps_all[:B], a.max_new) for B in batches}
        H, I, V, L = cfg.hidden_size, cfg.intermediate_size, cfg.vocab_size, cfg.num_hidden_layers
        q, kv = cfg.num_attention_heads * 128, cfg.num_key_value_heads * 128
        elems = L * ((q + 2 * kv) * H + H * q + 2 * I * H + H * I) + V * H
        t_q, _ = timed(lambda: m.quantize_weights(a.format, lm_head=True))
        got, _ = m.forward_initial(ps_all[0], 0)
        m.clear_cache()
        print(json.dumps({"model": name, "quantize_s": round(t_q, 3), "quantised_GB_bf16": round(elems * 2 / 1e9, 3),
                          "extra_GB": round(elems * F["bpw"] / 1e9, 3), "extra_over_quantised": round(F["bpw"] / 2, 4),
                          "prefill_logits_rms_dev_std": round(float(np.sqrt(((got - ref) ** 2).mean()) / ref.std()), 5),
                          "prefill_argmax_same": bool(int(np.argmax(got)) == int(np.argmax(ref)))}), flush=True)
        m.generate_batch(ps_all[:2], 4)   # warm-up of the FP8 kernels
        for B in batches:
            ps = ps_all[:B]
            f8, w16 = [], []
            for _ in range(3):   # alternating: the FP8 kernel, then the bf16 kernel on the dequantised weights of the same model
                m.debug_fp8_rows(True)
                f8.append(step_time(m, ps, a.max_new))
                m.debug_fp8_rows(False)
                w16.append(step_time(m, ps, a.max_new))
            m.debug_fp8_rows(True)
            pf = matvec_profile(m, ps, a.max_new)[F["cls"]]
            pb = prof_bf[B]["gemv_rows"]
            b, f = float(np.median(bf16[B] + w16)), float(np.median(f8))
            allb = bf16[B] + w16
            print(json.dumps({"model": name, "B": B, "prompt": a.prompt, "max_new": a.max_new,
                              "bf16_step_ms": round(b * 1e3, 3), "bf16_step_ms_runs": [round(t * 1e3, 3) for t in allb],
                              "bf16_spread_ms": round((max(allb) - min(allb)) * 1e3, 3),
                              f"{tag}_step_ms": round(f * 1e3, 3), f"{tag}_step_ms_runs": [round(t * 1e3, 3) for t in f8],
                              "bf16_decode_tok_s": round(B / b, 1), f"{tag}_decode_tok_s": round(B / f, 1), "speedup": round(b / f, 3),
                              "step_drops": bool(max(f8) < min(allb)),
                              "gemv_rows_ms_per_step": round(pb["ms"] / (a.max_new - 1), 3), "gemv_rows_hbm_frac": round(pb["bytes"] / (pb["ms"] * 1e-3) / HBM_PEAK, 3),
                              f"{F['cls']}_ms_per_step": round(pf["ms"] / (a.max_new - 1), 3),
                              f"{F['cls']}_hbm_frac": round(pf["bytes"] / (pf["ms"] * 1e-3) / HBM_PEAK, 3)}), flush=True)
        if not a.no_kernel:
            bench_ops(cfg, name, a.reps, a.format)
        m.close()
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
