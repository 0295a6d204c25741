"""Batched greedy generation (aha_hip_generate_batch) against serial decode_greedy, at Qwen3-0.6B and Qwen3-VL-8B text dimensions
(configs.qwen3_0_6b / qwen3vl_8b_text, seeded random weights generated on the GPU, no stop tokens so every sequence runs to max_new).
Prompts of --prompt tokens, --max-new new tokens.  Per batch size B:
  * aggregate tokens/s of one generate_batch call over B prompts (prefill included) and the decode step time, taken as
    (t(max_new) - t(1)) / (max_new - 1);
  * serial: forward_initial + decode_greedy on --serial prompts one after the other, decode tokens/s of that loop;
and, per projection shape, kernel A (gemv_rows) at R = 1, 16, 32 and above 32 rows (two row groups = the weights streamed twice), as
weight bytes / time and its fraction of the 8 TB/s HBM peak.  One JSON object per line.
With --sampler (the Qwen3 default request: T 0.6 / top_p 0.95 / top_k 20, repeat penalty 1.1 over the last 64 ids) each batch size is
also run through generate_batch_sampled (same timing rule; "sampled_vs_greedy" = its step over the greedy step), and the serial leg
is generate_generic_sampled (one host round trip per token) instead of decode_greedy.
    python scripts/bench_generate_batch.py [--only 0.6b,8b] [--batches 1,4,8,16,32,64] [--prompt 512] [--max-new 128] [--sampler]
    python scripts/bench_generate_batch.py --once 8b:16     # one generate_batch call and nothing else (rocprofv3 --kernel-trace --stats)
    python scripts/bench_generate_batch.py --once 8b:16 --sampler   # the same with generate_batch_sampled
With --vl: Qwen3-VL-8B with its vision tower (configs.qwen3vl_8b, seeded weights), B requests of one --image W x W image and --prompt
text tokens each, no stop tokens, through generate_batch_mm.  Per B: prefill ms (one call with max_new 1), ViT ms (vision_encode of
the B images in one call, timed apart: the tower's share of that prefill), decode step ms by the rule above, aggregate tok/s, and the
speed-up over a serial leg of forward_initial(mm) + decode_greedy on --serial requests (aggregate tok/s over whole requests).
    python scripts/bench_generate_batch.py --vl [--batches 1,4,8,16] [--image 448] [--prompt 512] [--max-new 64]
    python scripts/bench_generate_batch.py --vl --once vl8b:16   # one generate_batch_mm call (rocprofv3 --kernel-trace --stats)
With --asr: Qwen3-ASR-0.6B with its audio tower (configs.qwen3_asr_0_6b, seeded weights), B requests of one --clip-s second seeded clip
(raw samples) each, no stop tokens, through generate_batch_mm.  Per B: prefill ms (one call with max_new 1), tower ms (that prefill
minus the prefill of the same ids as text: the audio tower's share), the tower per clip, decode step ms by the rule above, aggregate
tok/s, audio seconds per wall second, and the speed-up over serial generate_asr (the ASR loop, greedy) on --serial requests.
    python scripts/bench_generate_batch.py --asr [--batches 1,4,16] [--clip-s 30] [--max-new 64]
    python scripts/bench_generate_batch.py --asr --once asr:16   # one generate_batch_mm call (rocprofv3 --kernel-trace --stats)"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

HBM_PEAK = 8.0e12


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


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return time.perf_counter() - t0, out


def bench_kernel_a(cfg, name):
    import torch
    from aha_amd import ops
    H, I, V = cfg.hidden_size, cfg.intermediate_size, cfg.vocab_size
    q, kv = cfg.num_attention_heads * 128, cfg.num_key_value_heads * 128
    shapes = {"qkv": (q + 2 * kv, H), "o_proj": (H, q), "gate_up": (2 * I, H), "down": (H, I), "lm_head": (V, H)}
    for sname, (N, K) in shapes.items():
        W = torch.randn(N, K, device="cuda", dtype=torch.bfloat16) * 0.02
        for R in (1, 16, 32, 64):
            reps = 20
            x = torch.randn(min(R, 32), K, device="cuda", dtype=torch.bfloat16)
            epi = ops.GEMV_ROWS_LOGITS if sname == "lm_head" else ops.GEMV_ROWS_STORE
            groups = (R + 31) // 32   # above 32 rows: one call per group of 32, each streaming the weights again
            ops.gemv_rows(W, x, epi)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(reps * groups):
                ops.gemv_rows(W, x, epi)
            torch.cuda.synchronize()
            # the op-level entry allocates its scratch and synchronises per call: an upper bound of the in-model kernel time
            dt = (time.perf_counter() - t0) / reps
            print(json.dumps({"kernel": "gemv_rows", "model": name, "shape": sname, "N": N, "K": K, "R": R, "us": round(dt * 1e6, 1),
                              "weight_GBps": round(N * K * 2 * groups / dt / 1e9, 1), "hbm_frac": round(N * K * 2 * groups / dt / HBM_PEAK, 3)}),
                  flush=True)
        del W


def sampler_params():
    from aha_amd.sampling import SamplingParams
    return SamplingParams(0.6, 0.95, 20, 1.1, 64)


def serial_sampled(m, ps, max_new):
    """generate_generic_sampled on each prompt: decode tokens/s and step time, the prefill token excluded (timed apart)."""
    import torch
    from aha_amd import sampling as hs
    dec = 0.0
    for j, p in enumerate(ps):
        sp = sampler_params()
        sp.seed = j
        t1, _ = timed(lambda: hs.generate_generic_sampled(m, p, sp.context(len(p), 1)))
        tn, out = timed(lambda: hs.generate_generic_sampled(m, p, sp.context(len(p), max_new)))
        assert len(out) == max_new
        dec += tn - t1
    torch.cuda.synchronize()
    return len(ps) * (max_new - 1) / dec, dec / (len(ps) * (max_new - 1))


def vl_requests(cfg, B, px, L, seed=0):
    import torch
    from aha_amd.vision_host import synthetic_image_request
    g = torch.Generator().manual_seed(seed)
    return [synthetic_image_request(cfg, px, L, g) for _ in range(B)]


def bench_vl(a):
    """generate_batch_mm on Qwen3-VL-8B with one image per request against serial forward_initial(mm) + decode_greedy."""
    import torch
    from aha_amd.configs import qwen3vl_8b
    from aha_amd.model import HipInferenceModel, MultiModalData
    from aha_amd.weights import qwen3vl_weights
    cfg = qwen3vl_8b()
    cfg.text.eos_token_ids = []
    w = qwen3vl_weights(cfg, seed=0, device="cuda")
    m = HipInferenceModel(cfg, w)
    del w
    torch.cuda.empty_cache()
    batches = [int(b) for b in a.batches.split(",")]
    if a.once:
        B = int(a.once.split(":")[1])
        reqs = vl_requests(cfg, B, a.image, a.prompt)
        m.generate_batch_mm([r[0] for r in reqs], [r[1] for r in reqs], a.max_new)
        torch.cuda.synchronize()
        m.close()
        return
    reqs_all = vl_requests(cfg, max(batches + [a.serial]), a.image, a.prompt)
    dec = 0.0
    for ids, data in reqs_all[:a.serial]:
        m.clear_cache()
        _, tok = m.forward_initial(ids, 0, data, want_logits=False)
        torch.cuda.synchronize()
        dt, _ = timed(lambda: m.decode_greedy(tok, len(ids), a.max_new - 1))
        dec += dt
        m.clear_cache()
    def serial_request(ids, data):
        _, tok = m.forward_initial(ids, 0, data, want_logits=False)
        return m.decode_greedy(tok, len(ids), a.max_new - 1)

    t_ser = 0.0
    for ids, data in reqs_all[:a.serial]:   # the whole serial request: prefill + decode
        t, _ = timed(lambda: serial_request(ids, data))
        m.clear_cache()
        t_ser += t
    serial_tps = a.serial * a.max_new / t_ser
    print(json.dumps({"model": "vl8b", "image": a.image, "prompt": a.prompt, "serial_decode_tok_s": round(a.serial * (a.max_new - 1) / dec, 1),
                      "serial_aggregate_tok_s": round(serial_tps, 1)}), flush=True)
    m.generate_batch_mm([reqs_all[0][0]], [reqs_all[0][1]], 2)   # warm-up
    for B in batches:
        reqs = reqs_all[:B]
        ps, ds = [r[0] for r in reqs], [r[1] for r in reqs]
        pv = torch.cat([d.pixel_values for d in ds], 0)
        grid = np.concatenate([d.image_grid_thw for d in ds], 0)
        torch.cuda.synchronize()
        tv, _ = timed(lambda: (m.vision_encode(MultiModalData(pv, grid)), torch.cuda.synchronize()))
        t1, _ = timed(lambda: m.generate_batch_mm(ps, ds, 1))
        tn, out = timed(lambda: m.generate_batch_mm(ps, ds, a.max_new))
        assert all(len(o) == a.max_new for o in out)
        step = (tn - t1) / (a.max_new - 1)
        print(json.dumps({"model": "vl8b", "B": B, "image": a.image, "prompt": a.prompt, "max_new": a.max_new, "prefill_ms": round(t1 * 1e3, 2),
                          "vit_ms": round(tv * 1e3, 2), "step_ms": round(step * 1e3, 3), "total_s": round(tn, 3),
                          "aggregate_tok_s": round(B * a.max_new / tn, 1), "vs_serial": round(B * a.max_new / tn / serial_tps, 2)}), flush=True)
    m.close()


def asr_requests(cfg, B, seconds, seed=0):
    """B (ids, MultiModalData) requests: a few text tokens, <|audio_start|>, one <|audio_pad|> per audio token, <|audio_end|>, text."""
    from aha_amd.model import MultiModalData
    from oracle.qwen3_asr import get_feat_extract_output_lengths
    g = np.random.default_rng(seed)
    out = []
    for _ in range(B):
        wave = np.clip(g.normal(0, 0.1, int(16000 * seconds)), -1, 1).astype(np.float32)
        n_tok = get_feat_extract_output_lengths(wave.size // 160)
        ids = [int(x) for x in g.integers(0, 150000, size=5)] + [cfg.audio_start_token_id] + [cfg.audio_token_id] * n_tok + \
              [cfg.audio_end_token_id] + [int(x) for x in g.integers(0, 150000, size=7)]
        out.append((ids, MultiModalData(audio_samples=wave)))
    return out


def bench_asr(a):
    """generate_batch_mm on Qwen3-ASR-0.6B with one clip per request against serial generate_asr."""
    import torch
    from aha_amd import sampling as hs
    from aha_amd.configs import qwen3_asr_0_6b
    from aha_amd.model import HipInferenceModel
    from aha_amd.weights import qwen3_asr_weights
    cfg = qwen3_asr_0_6b()
    cfg.text.eos_token_ids = []
    w = qwen3_asr_weights(cfg, seed=0, device="cuda")
    m = HipInferenceModel(cfg, w)
    del w
    torch.cuda.empty_cache()
    batches = [int(b) for b in a.batches.split(",")]
    if a.once:
        B = int(a.once.split(":")[1])
        reqs = asr_requests(cfg, B, a.clip_s)
        m.generate_batch_mm([r[0] for r in reqs], [r[1] for r in reqs], a.max_new)
        torch.cuda.synchronize()
        m.close()
        return
    reqs_all = asr_requests(cfg, max(batches + [a.serial]), a.clip_s)
    hs.generate_asr(m, [reqs_all[0]], 0.0, max_tokens=2)   # warm-up
    t_ser, t_pre = 0.0, 0.0
    for ids, data in reqs_all[:a.serial]:   # the whole ASR loop of one request: prefill + decode
        t, (out, _) = timed(lambda: hs.generate_asr(m, [(ids, data)], 0.0, max_tokens=a.max_new))
        assert len(out) == a.max_new
        t_ser += t
        tp, _ = timed(lambda: (m.forward_initial(ids, 0, data, want_logits=False), m.clear_cache()))
        t_pre += tp
    serial_tps = a.serial * a.max_new / t_ser
    print(json.dumps({"model": "asr0.6b", "clip_s": a.clip_s, "serial_prefill_ms": round(t_pre / a.serial * 1e3, 2),
                      "serial_request_s": round(t_ser / a.serial, 3), "serial_aggregate_tok_s": round(serial_tps, 1),
                      "serial_audio_s_per_s": round(a.serial * a.clip_s / t_ser, 1)}), flush=True)
    m.generate_batch_mm([reqs_all[0][0]], [reqs_all[0][1]], 2)   # warm-up
    tower1 = None
    for B in batches:
        reqs = reqs_all[:B]
        ps, ds = [r[0] for r in reqs], [r[1] for r in reqs]
        m.generate_batch_mm(ps, ds, 1)   # scratch at this size
        t1, _ = timed(lambda: m.generate_batch_mm(ps, ds, 1))
        tt, _ = timed(lambda: m.generate_batch_mm(ps, None, 1))
        tn, out = timed(lambda: m.generate_batch_mm(ps, ds, a.max_new))
        assert all(len(o) == a.max_new for o in out)
        step = (tn - t1) / (a.max_new - 1)
        tower = t1 - tt
        tower1 = tower if tower1 is None and B == 1 else tower1
        rec = {"model": "asr0.6b", "B": B, "clip_s": a.clip_s, "max_new": a.max_new, "prefill_ms": round(t1 * 1e3, 2),
               "tower_ms": round(tower * 1e3, 2), "tower_ms_per_clip": round(tower / B * 1e3, 3), "step_ms": round(step * 1e3, 3),
               "total_s": round(tn, 3), "aggregate_tok_s": round(B * a.max_new / tn, 1), "audio_s_per_s": round(B * a.clip_s / tn, 1),
               "vs_serial": round(B * a.max_new / tn / serial_tps, 2)}
        if tower1:
            rec["tower_per_clip_vs_alone"] = round(tower / B / tower1, 3)
        print(json.dumps(rec), flush=True)
    m.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default="0.6b,8b")
    ap.add_argument("--batches", default="1,4,8,16,32,64")
    ap.add_argument("--prompt", type=int, default=512)
    ap.add_argument("--max-new", type=int, default=128)
    ap.add_argument("--serial", type=int, default=4)
    ap.add_argument("--once", default="")
    ap.add_argument("--no-kernel", action="store_true")
    ap.add_argument("--sampler", action="store_true", help="also the batched sampled path; the serial leg samples too")
    ap.add_argument("--vl", action="store_true", help="Qwen3-VL-8B requests with one image each through generate_batch_mm")
    ap.add_argument("--image", type=int, default=448)
    ap.add_argument("--asr", action="store_true", help="Qwen3-ASR-0.6B requests with one audio clip each through generate_batch_mm")
    ap.add_argument("--clip-s", type=float, default=30.0)
    a = ap.parse_args()
    import torch
    from aha_amd import build
    build.build()
    if a.vl:
        bench_vl(a)
        return
    if a.asr:
        bench_asr(a)
        return
    if a.once:
        name, B = a.once.split(":")
        cfg, m = model_for(name)
        ps = prompts(int(B), a.prompt, cfg.vocab_size)
        if a.sampler:
            m.generate_batch_sampled(ps, sampler_params(), a.max_new)
        else:
            m.generate_batch(ps, a.max_new)
        torch.cuda.synchronize()
        m.close()
        return
    for name in a.only.split(","):
        cfg, m = model_for(name)
        ps_all = prompts(max(int(b) for b in a.batches.split(",")), a.prompt, cfg.vocab_size)
        if a.sampler:   # serial generate_generic_sampled over the first --serial prompts
            serial_tps, serial_step = serial_sampled(m, ps_all[:a.serial], a.max_new)
            print(json.dumps({"model": name, "serial_sampled_decode_tok_s": round(serial_tps, 1), "serial_sampled_step_ms": round(serial_step * 1e3, 3)}),
                  flush=True)
        else:   # serial decode_greedy over the first --serial prompts
            dec = 0.0
            for p in ps_all[:a.serial]:
                m.clear_cache()
                _, tok = m.forward_initial(p, 0, want_logits=False)
                torch.cuda.synchronize()
                dt, toks = timed(lambda: m.decode_greedy(tok, len(p), a.max_new - 1))
                dec += dt
                m.clear_cache()
            serial_tps = a.serial * (a.max_new - 1) / dec
            print(json.dumps({"model": name, "serial_decode_tok_s": round(serial_tps, 1), "serial_step_ms": round(dec / (a.serial * (a.max_new - 1)) * 1e3, 3)}),
                  flush=True)
        m.generate_batch(ps_all[:2], 4)   # warm-up
        if a.sampler:
            m.generate_batch_sampled(ps_all[:2], sampler_params(), 4)
        for B in (int(b) for b in a.batches.split(",")):
            ps = ps_all[:B]
            t1, _ = timed(lambda: m.generate_batch(ps, 1))
            tn, out = timed(lambda: m.generate_batch(ps, a.max_new))
            assert all(len(o) == a.max_new for o in out)
            step = (tn - t1) / (a.max_new - 1)
            rec = {"model": name, "B": B, "prompt": a.prompt, "max_new": a.max_new, "total_s": round(tn, 3),
                   "aggregate_tok_s": round(B * a.max_new / tn, 1), "step_ms": round(step * 1e3, 3), "decode_tok_s": round(B / step, 1)}
            if a.sampler:
                sp = sampler_params()
                s1, _ = timed(lambda: m.generate_batch_sampled(ps, sp, 1))
                sn, out = timed(lambda: m.generate_batch_sampled(ps, sp, a.max_new))
                assert all(len(o) == a.max_new for o in out)
                sstep = (sn - s1) / (a.max_new - 1)
                rec.update({"sampled_total_s": round(sn, 3), "sampled_step_ms": round(sstep * 1e3, 3), "sampled_decode_tok_s": round(B / sstep, 1),
                            "sampled_vs_greedy": round(sstep / step, 3), "sampled_vs_serial_sampled": round(B / sstep / serial_tps, 2)})
            else:
                rec["decode_vs_serial"] = round(B / step / serial_tps, 2)
            print(json.dumps(rec), flush=True)
        if not a.no_kernel:
            bench_kernel_a(cfg, name)
        m.close()
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
