"""GPU microbenchmark of the weight-streaming matvec at the Qwen3-VL-8B decode shapes (rotating over enough distinct
matrices to defeat the 256 MB Infinity Cache).  Knobs: AHA_GEMV_GRID / AHA_GEMV_R / AHA_GEMV_U env vars."""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from aha_amd import ops, build
build.build()
dev = torch.device("cuda:0")
shapes = [("qkv", 6144, 4096, True), ("o", 4096, 4096, False), ("down", 4096, 12288, False), ("gateup", 12288, 4096, True),
          ("lm_head", 151936, 4096, True), ("qkv0.6", 4096, 1024, True), ("down0.6", 1024, 3072, False)]
sel = os.environ.get("SHAPES")
for name, N, K, norm in shapes:
    if os.environ.get("FORMS"):
        break
    if sel and name not in sel.split(","):
        continue
    gate = name == "gateup"
    per = N * K * 2 * (2 if gate else 1)
    ncopy = int(os.environ.get('NCOPY', 0)) or max(2, min(16, int(1.2e9 // per)))
    Ws = [torch.randn(N, K, device=dev, dtype=torch.bfloat16) * 0.02 for _ in range(ncopy)]
    W2 = [torch.randn(N, K, device=dev, dtype=torch.bfloat16) * 0.02 for _ in range(ncopy)] if gate else None
    x = torch.randn(K, device=dev, dtype=torch.bfloat16)
    nw = torch.ones(K, device=dev, dtype=torch.bfloat16) if norm else None
    def run(i):
        if gate:
            return ops.gemv_gate_up(Ws[i % ncopy], W2[i % ncopy], x, nw)
        return ops.gemv(Ws[i % ncopy], x, nw)
    for i in range(ncopy): run(i)
    torch.cuda.synchronize()
    iters = ncopy * 6
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(iters): run(i)
    e1.record(); torch.cuda.synchronize()
    us = e0.elapsed_time(e1) * 1e3 / iters
    print(f"{name:8s} N={N:6d} K={K:5d} {per/1e6:8.1f} MB  {us:8.2f} us/launch  {per/us/1e6:6.2f} TB/s (incl. launch gaps)", flush=True)

# FORMS=pk13: the bf16 kernel against the exact 13-bit copy (ops.gemv_pk13) on the decode step's own epilogues, 20 launches per form,
# alternating, each timed by its own event pair over rotating matrices; p10 / p50 / p90 per form.  The rule (profiles/weights_pk13.md): a
# matrix goes to the packed kernel by plan only where its packed p90 is below its bf16 p10.  (The lm_head rows carry the entry's partials
# allocation and argmax launch in both forms.)
if os.environ.get("FORMS") == "pk13":
    import numpy as np
    epis = {"qkv": 0, "o": 1, "down": 1, "gateup": 2, "lm_head": 3}
    print("alternating, 20 launches per form: us p10 / p50 / p90")
    for name, N, K, norm in shapes:
        if name not in epis or (sel and name not in sel.split(",")):
            continue
        epi = epis[name]
        rows = 2 * N if epi == 2 else N
        per = rows * K * 2
        ncopy = max(2, min(16, int(1.2e9 // per)))
        Ws = [torch.randn(rows, K, device=dev, dtype=torch.bfloat16) * 0.02 for _ in range(ncopy)]
        for w in Ws:      # a stray sample 30 binades below the maximum would leave its matrix unpacked
            w[w.abs() < 2.0 ** -24] = 0
        Ps = [ops.pack_pk13(w) for w in Ws]
        assert all(p[2] == 0 for p in Ps), [p[2] for p in Ps]
        x = torch.randn(K, device=dev, dtype=torch.bfloat16)
        nw = torch.ones(K, device=dev, dtype=torch.bfloat16) if norm else None
        res = torch.randn(N, device=dev, dtype=torch.bfloat16) if epi == 1 else None
        out = torch.empty(N, device=dev, dtype=torch.bfloat16) if epi != 3 else None

        def launch(form, i):
            if form == 0:
                return ops.gemv_epi(Ws[i % ncopy], x, epi, norm_w=nw, residual=res, out=out)
            return ops.gemv_pk13(Ps[i % ncopy][0], Ps[i % ncopy][1], x, epi, norm_w=nw, residual=res, out=out)
        for i in range(ncopy):
            launch(0, i), launch(1, i)
        torch.cuda.synchronize()
        t = ([], [])
        for i in range(20):
            for form in (0, 1):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                launch(form, i)
                e1.record()
                torch.cuda.synchronize()
                t[form].append(e0.elapsed_time(e1) * 1e3)
        q = [np.percentile(v, (10, 50, 90)) for v in t]
        verdict = "packed by plan" if q[1][2] < q[0][0] else "stays on bf16"
        print(f"{name:8s} N={rows:6d} K={K:5d}  bf16 {q[0][0]:7.2f} {q[0][1]:7.2f} {q[0][2]:7.2f}   pk13 {q[1][0]:7.2f} {q[1][1]:7.2f} {q[1][2]:7.2f}   "
              f"{per / q[0][1] / 1e6:5.2f} -> {per * 0.8125 / q[1][1] / 1e6:5.2f} TB/s at p50   {verdict}", flush=True)
        del Ws, Ps
