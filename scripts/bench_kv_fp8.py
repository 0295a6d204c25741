"""Measures the E4M3 KV cache against the bf16 cache; results go to profiles/kv_fp8.md.

  python scripts/bench_kv_fp8.py model --size 0.6b --kv bf16 --weights bf16 --seqs 16 --ctx 512
      ONE configuration in THIS process (run the bf16 and e4m3 caches in fresh processes, alternated, and repeat the bf16 one for its
      run-to-run spread): generate_batch of `seqs` random prompts of `ctx` tokens on random weights, --new tokens; prints the profile
      classes of the decode attention and of the conversion (ms per launch from the model's event profiler, bytes/s from ProfScope's
      bytes) and the wall time per decode step.
  python scripts/bench_kv_fp8.py launch --seqs 16 --ctx 512
      the op-level launches alone on random pages (32 q heads, 8 kv heads): ops.attn_decode_batch over bf16 pages, ops.attn_decode_batch_kv8
      over their conversion, ops.quantize_kv_pages -- each call once per repetition, for `rocprofv3 --kernel-trace --stats -- python ...`
      to time the kernels (the entries allocate and synchronise per call, so host-side timing of them says nothing about the kernels).
  python scripts/bench_kv_fp8.py --single --size 8b --kv e4m3 --weights mxfp4 --ctxs 512,4096,32768
      the SINGLE-sequence decode (results in profiles/kv_fp8_single.md): ONE (size, cache, weights) in THIS process
      (run bf16 and e4m3 in fresh processes, alternated, at least three each), and per context one JSON line: forward_initial of `ctx`
      random tokens, a warm-up decode_greedy, the wall time per step of decode_greedy over --new steps (the call ends in a stream
      synchronise), then a few steps with the model's event profiler on for the attention launch.  --kv e4m3 sets the cache with
      set_kv_format_with("e4m3", single=True).  AHA_ATTN_PAGES_PER_BLOCK in the environment changes the split rule under test.  Under
      `rocprofv3 --kernel-trace --stats -- python ...` the kernels to compare are attn_decode_fused_kernel and attn_decode_fused_kv8_kernel.
"""
import argparse
import json
import sys
import time

import numpy as np
import torch

sys.path.insert(0, __import__("os").path.dirname(__import__("os").path.dirname(__import__("os").path.abspath(__file__))))


def run_model(a):
    from aha_amd import configs
    from aha_amd.model import HipInferenceModel
    from aha_amd.weights import qwen3_text_weights
    cfg = configs.qwen3_0_6b() if a.size == "0.6b" else configs.qwen3vl_8b_text()
    m = HipInferenceModel(cfg, qwen3_text_weights(cfg, seed=0))
    if a.weights != "bf16":
        m.quantize_weights(a.weights)
    m.set_kv_format(a.kv)
    rng = np.random.default_rng(1)
    prompts = [[int(x) for x in rng.integers(0, cfg.vocab_size, size=a.ctx)] for _ in range(a.seqs)]
    m.generate_batch(prompts, 2, max_tokens_per_pass=8192)   # warm-up: slabs, page tables, code objects
    t0 = time.perf_counter()
    m.generate_batch(prompts, 1, max_tokens_per_pass=8192)
    t1 = time.perf_counter()
    m.generate_batch(prompts, a.new, max_tokens_per_pass=8192)
    t2 = time.perf_counter()
    m.set_profiling(True)
    m.generate_batch(prompts, a.new, max_tokens_per_pass=8192)
    attn = m.get_profile("attn_decode_batch_kv8" if a.kv == "e4m3" else "attn_decode_batch")
    conv = m.get_profile("kv_pages_quantize")
    out = dict(size=a.size, kv=a.kv, weights=a.weights, seqs=a.seqs, ctx=a.ctx, new=a.new,
               ms_per_decode_step=((t2 - t1) - (t1 - t0)) * 1e3 / (a.new - 1),
               attn_us_per_launch=attn["ms"] * 1e3 / max(attn["launches"], 1),
               attn_tb_per_s=attn["bytes"] / max(attn["ms"], 1e-9) / 1e9,
               convert_us_per_prompt_token=conv["ms"] * 1e3 / (a.seqs * a.ctx) if conv["launches"] else None)
    print(json.dumps(out))
    m.close()


def run_single(a):
    import os
    from aha_amd import configs
    from aha_amd.model import HipInferenceModel
    from aha_amd.weights import qwen3_text_weights
    cfg = configs.qwen3_0_6b() if a.size == "0.6b" else configs.qwen3vl_8b_text()
    m = HipInferenceModel(cfg, qwen3_text_weights(cfg, seed=0))
    if a.weights != "bf16":
        m.quantize_weights(a.weights)
    if a.kv == "e4m3":
        m.set_kv_format_with("e4m3", single=True)
    cls = "attn_decode_kv8" if a.kv == "e4m3" else "attn_decode"
    ids = [int(x) for x in np.random.default_rng(1).integers(0, cfg.vocab_size, size=max(a.ctxs))]
    for ctx in a.ctxs:
        m.clear_cache()
        _, tok = m.forward_initial(ids[:ctx], 0, want_logits=False)
        warm = m.decode_greedy(tok, ctx, 8)
        t0 = time.perf_counter()
        got = m.decode_greedy(warm[-1], ctx + len(warm), a.new)
        t1 = time.perf_counter()
        m.set_profiling(True)   # (clears the accumulators)
        m.decode_greedy(got[-1], ctx + len(warm) + len(got), 8)
        m.set_profiling(False)
        attn = m.get_profile(cls)
        print(json.dumps(dict(size=a.size, kv=a.kv, weights=a.weights, ctx=ctx, steps=len(got), pages_per_block=os.environ.get("AHA_ATTN_PAGES_PER_BLOCK", "4"),
                              form=m.debug_attn_decode_form(), ms_per_step=(t1 - t0) * 1e3 / max(len(got), 1),
                              attn_us_per_launch=attn["ms"] * 1e3 / max(attn["launches"], 1),
                              attn_gb_per_s=attn["bytes"] / max(attn["ms"], 1e-9) / 1e6)), flush=True)
    m.close()


def run_launch(a):
    from aha_amd import ops
    nh, kvh, D, R = 32, 8, 128, a.seqs
    npg = (a.ctx + 64) // 64
    P = R * npg
    g = torch.Generator(device="cuda").manual_seed(0)
    pool = torch.randn(P, 2 * kvh * 64 * D, generator=g, device="cuda", dtype=torch.float32).to(torch.bfloat16)
    pool8 = torch.zeros(P, ops.kv8_page_bytes(kvh), dtype=torch.uint8, device="cuda")
    ptrs = pool.data_ptr() + torch.arange(P, device="cuda") * pool.shape[1] * 2
    ptrs8 = pool8.data_ptr() + torch.arange(P, device="cuda") * pool8.shape[1]
    qkv = torch.randn(R, (nh + 2 * kvh) * D, generator=g, device="cuda").to(torch.bfloat16)
    w = torch.ones(D, device="cuda", dtype=torch.bfloat16)
    ang = torch.rand(R, 64, generator=g, device="cuda") * 6
    rope = torch.cat([torch.cos(ang), torch.sin(ang)], 1).to(torch.bfloat16).float().contiguous()
    page0, lens = [r * npg for r in range(R)], [a.ctx + 1] * R
    for _ in range(a.reps):   # alternated
        ops.quantize_kv_pages(ptrs, ptrs8, kvh)
        ops.attn_decode_batch(qkv, w, w, rope, ptrs, page0, lens, nh, kvh, 1e-6, D ** -0.5)
        ops.attn_decode_batch_kv8(qkv, w, w, rope, ptrs8, page0, lens, nh, kvh, 1e-6, D ** -0.5)
    torch.cuda.synchronize()
    print(json.dumps(dict(seqs=R, ctx=a.ctx, reps=a.reps, bf16_bytes_per_launch=R * a.ctx * 2 * kvh * D * 2,
                          kv8_bytes_per_launch=R * a.ctx * 2 * kvh * (D + 1), pages=P)))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="mode", required=True)
    pm = sub.add_parser("model")
    pm.add_argument("--size", choices=["0.6b", "8b"], default="0.6b")
    pm.add_argument("--kv", choices=["bf16", "e4m3"], default="bf16")
    pm.add_argument("--weights", choices=["bf16", "mxfp8"], default="bf16")
    pm.add_argument("--new", type=int, default=17)
    pl = sub.add_parser("launch")
    pl.add_argument("--reps", type=int, default=20)
    for p in (pm, pl):
        p.add_argument("--seqs", type=int, default=16)
        p.add_argument("--ctx", type=int, default=512)
    ps = sub.add_parser("single")
    ps.add_argument("--size", choices=["0.6b", "8b"], default="0.6b")
    ps.add_argument("--kv", choices=["bf16", "e4m3"], default="bf16")
    ps.add_argument("--weights", choices=["bf16", "mxfp4"], default="bf16")
    ps.add_argument("--ctxs", type=lambda v: [int(x) for x in v.split(",")], default=[512, 4096, 32768])
    ps.add_argument("--new", type=int, default=64)
    args = ap.parse_args(["single" if x == "--single" else x for x in sys.argv[1:]])
    {"model": run_model, "launch": run_launch, "single": run_single}[args.mode](args)
