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
# allocation and argmax launch in both forms.)  lm_head and gate+up also run the twin kernel (ops.gemv_pk13_rows) on copies of the same
# matrices with one planted exception row (a weight of 1e-30): its p50 should lie inside the plain packed kernel's p10 .. p90
# (profiles/weights_pk13_rows.md).
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

        forms = (0, 1, 2) if name in ("gateup", "lm_head") else (0, 1)
        Wx, Px = [], []
        if 2 in forms:      # the same matrices with one weight below the window, in a row of the middle of the matrix
            for w in Ws:
                wx = w.clone()
                wx[rows // 2 + 3, 1234] = 1e-30
                Wx.append(wx)
                Px.append(ops.pack_pk13_rows(wx))
            assert all(p[0] is not None and p[2] == [rows // 2 + 3] for p in Px), [p[2:] for p in Px]

        def launch(form, i):
            if form == 0:
                return ops.gemv_epi(Ws[i % ncopy], x, epi, norm_w=nw, residual=res, out=out)
            if form == 2:
                return ops.gemv_pk13_rows(Px[i % ncopy][0], Px[i % ncopy][1], Wx[i % ncopy], Px[i % ncopy][2], x, epi, norm_w=nw, residual=res, out=out)
            return ops.gemv_pk13(Ps[i % ncopy][0], Ps[i % ncopy][1], x, epi, norm_w=nw, residual=res, out=out)
        for i in range(ncopy):
            for form in forms:
                launch(form, i)
        torch.cuda.synchronize()
        t = ([], [], [])
        for i in range(20):
            for form in forms:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                launch(form, i)
                e1.record()
                torch.cuda.synchronize()
                t[form].append(e0.elapsed_time(e1) * 1e3)
        q = [np.percentile(v, (10, 50, 90)) for v in t if v]
        verdict = "packed by plan" if q[1][2] < q[0][0] else "stays on bf16"
        print(f"{name:8s} N={rows:6d} K={K:5d}  bf16 {q[0][0]:7.2f} {q[0][1]:7.2f} {q[0][2]:7.2f}   pk13 {q[1][0]:7.2f} {q[1][1]:7.2f} {q[1][2]:7.2f}   "
              f"{per / q[0][1] / 1e6:5.2f} -> {per * 0.8125 / q[1][1] / 1e6:5.2f} TB/s at p50   {verdict}", flush=True)
        if 2 in forms:
            inside = q[1][0] <= q[2][1] <= q[1][2]
            beats = "p90 below bf16 p10" if q[2][2] < q[0][0] else "p90 NOT below bf16 p10"
            print(f"{name:8s} one exception row: pk13 rows {q[2][0]:7.2f} {q[2][1]:7.2f} {q[2][2]:7.2f}   p50 {'inside' if inside else 'OUTSIDE'} the plain "
                  f"packed kernel's p10 .. p90 ({q[2][1] - q[1][1]:+.2f} us at p50); {beats}", flush=True)
        del Ws, Ps, Wx, Px
