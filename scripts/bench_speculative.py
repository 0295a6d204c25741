"""Draft-and-verify greedy decoding (aha_hip_generate_batch_spec) against aha_hip_generate_batch, at Qwen3-0.6B and Qwen3-VL-8B text
dimensions (configs.qwen3_0_6b / qwen3vl_8b_text, seeded random weights generated on the GPU, no stop tokens: every sequence runs to
max_new).  Prompts of --prompt tokens, --max-new new tokens, B sequences.

Predictions are the true greedy continuation with a seeded fraction of its positions corrupted ((t + 1) mod vocab): 0 = everything is
accepted, 1 = every token wrong.  Per (B, fraction, max_draft), --reps timed calls after one warm-up, median and min / max reported:
  decode_tok_s      B * (max_new - 1) / (t(max_new) - t(1)): the decode phase alone, prefill subtracted by the same rule as
                    scripts/bench_generate_batch.py;
  step_ms           the decode phase over the call's decode steps (aha_spec_stats);
  tok_per_step      tokens emitted per sequence per step;
  accept_rate       accepted / proposed draft tokens;
  draft_rows        rows beyond one per sequence per step, and draft_kv_GB, the KV those rows read: each draft row streams its
                    sequence's cache on its own, like any row (draft rows x mean cache length x bytes per token per layer x layers; the
                    attention's own byte count of a profiled run is reported next to it as attn_GB, with attn_GB_plain for generate_batch);
  vs_plain          decode_tok_s over generate_batch's on the same prompts in the same process.
One JSON object per line.  --lib PATH loads another build of libaha_hip.so (e.g. the parent commit's, for the two figures that are
compared against it); with --plain-only only generate_batch is timed, which is all an older build can do.
    python scripts/bench_speculative.py [--only 0.6b,8b] [--batches 1,4,16] [--drafts 1,3,7,15] [--fractions 0,0.25,0.5,1.0]
                                        [--prompt 512] [--max-new 256] [--reps 5] [--lib PATH] [--plain-only]"""
import argparse
import json
import os
import statistics
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


def timed_reps(fn, reps):
    fn()   # warm-up: scratch at this size, pages
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        ts.append(time.perf_counter() - t0)
    return ts, out


def spread(xs):
    return {"median": round(statistics.median(xs), 3), "min": round(min(xs), 3), "max": round(max(xs), 3)}


def attn_bytes(m, fn):
    m.set_profiling(False)
    m.set_profiling(True)
    fn()
    b = m.get_profile("attn_decode_batch")["bytes"]
    m.set_profiling(False)
    return b


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default="0.6b,8b")
    ap.add_argument("--batches", default="1,4,16")
    ap.add_argument("--drafts", default="1,3,7,15")
    ap.add_argument("--fractions", default="0,0.25,0.5,1.0")
    ap.add_argument("--prompt", type=int, default=512)
    ap.add_argument("--max-new", type=int, default=256)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--lib", default="", help="another build of libaha_hip.so to load instead of the tree's")
    ap.add_argument("--plain-only", action="store_true", help="time generate_batch only")
    a = ap.parse_args()
    from aha_amd import _lib
    if a.lib:
        import ctypes
        import torch  # noqa: F401  (before the library: one HIP runtime per process, see _lib.lib)
        _lib.LIB_PATH = os.path.abspath(a.lib)
        raw = ctypes.CDLL(_lib.LIB_PATH)
        _lib.SIGNATURES = {k: v for k, v in _lib.SIGNATURES.items() if hasattr(raw, k)}   # an older build: bind what it exports
    else:
        from aha_amd import build
        build.build()
    import torch
    from aha_amd.speculative import SpecConfig
    N = a.max_new
    for name in a.only.split(","):
        cfg, m = model_for(name)
        kv_tok_bytes = 2 * cfg.num_key_value_heads * 128 * 2 * cfg.num_hidden_layers   # K + V, bf16, every layer
        ps_all = prompts(max(int(b) for b in a.batches.split(",")), a.prompt, cfg.vocab_size)
        for B in (int(b) for b in a.batches.split(",")):
            ps = ps_all[:B]
            t1s, _ = timed_reps(lambda: m.generate_batch(ps, 1), a.reps)
            tns, truth = timed_reps(lambda: m.generate_batch(ps, N), a.reps)
            assert all(len(o) == N for o in truth)
            t1 = statistics.median(t1s)
            plain = [B * (N - 1) / (t - t1) for t in tns]
            plain_med = statistics.median(plain)
            rec = {"model": name, "B": B, "prompt": a.prompt, "max_new": N, "path": "generate_batch", "lib": a.lib or "tree",
                   "prefill_ms": round(t1 * 1e3, 2), "decode_tok_s": spread(plain), "step_ms": spread([(t - t1) / (N - 1) * 1e3 for t in tns])}
            if not a.plain_only:
                rec["attn_GB_plain"] = round(attn_bytes(m, lambda: m.generate_batch(ps, N)) / 1e9, 3)
            print(json.dumps(rec), flush=True)
            if a.plain_only:
                continue
            for frac in (float(f) for f in a.fractions.split(",")):
                g = np.random.default_rng(1000 + int(frac * 100))
                preds = [[(t + 1) % cfg.vocab_size if g.random() < frac else t for t in o] for o in truth]
                for D in (int(d) for d in a.drafts.split(",")):
                    spec = SpecConfig(D, 1, 3)
                    run = lambda: m.generate_batch_spec(ps, N, spec, preds, want_stats=True)
                    tss, (out, info) = timed_reps(run, a.reps)
                    assert out == truth, "draft-and-verify output differs from generate_batch"
                    st = info["stats"]
                    tok_s = [B * (N - 1) / (t - t1) for t in tss]
                    mandatory = B * st.decode_steps   # no stop tokens: every sequence is active in every step
                    draft_rows = st.rows - mandatory
                    print(json.dumps({
                        "model": name, "B": B, "prompt": a.prompt, "max_new": N, "path": "generate_batch_spec", "corrupt": frac, "max_draft": D,
                        "decode_tok_s": spread(tok_s), "vs_plain": round(statistics.median(tok_s) / plain_med, 3),
                        "decode_steps": st.decode_steps, "step_ms": spread([(t - t1) / max(st.decode_steps, 1) * 1e3 for t in tss]),
                        "tok_per_step": round((N - 1) / max(st.decode_steps, 1), 2),
                        "accept_rate": round(st.accepted / st.proposed, 3) if st.proposed else None,
                        "rows": st.rows, "draft_rows": draft_rows,
                        "draft_kv_GB": round(draft_rows * (a.prompt + N / 2) * kv_tok_bytes / 1e9, 3),
                        "attn_GB": round(attn_bytes(m, run) / 1e9, 3)}), flush=True)
        m.close()
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
