"""Output digests of the batched decode matvec in its three weight forms and of the library's two MX quantisers.
tests/golden/gemv_rows_parent_digests.json holds them as computed by the library while gemv_rows_kernel, gemv_rows_mxfp8_kernel and
gemv_rows_mxfp4_kernel were three separate texts (`python tests/gemv_rows_digests.py OUT.json` on an MI355X);
tests/test_gemv_rows_digests_gpu.py recomputes them and asserts equality.  "MX output == bf16 output on W'" compares the one shared body
(csrc/gemv_rows_body.h) with itself; these digests hold the shared part -- k permutation, tail rules, summation order -- to what it was.

Per (N, K) of every plan branch, R in (1, 16, 17, 32) and epilogue: a sha256 over the output bits (and the argmax of the logits epilogue)
of gemv_rows on W', gemv_rows_mxfp8 and gemv_rows_mxfp4, W' being each format's own dequantised copy.  Per format and small matrix: a
sha256 over the q, scale and W' bytes ops.quantize_mxfp8 / ops.quantize_mxfp4 return."""
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

# ragged N, a partial last chunk and waves past the end of K; the plan's fallback to CW = 1 with two K splits; CW = 2 with one split;
# CW = 2 with two splits
SHAPES = ((40, 160), (96, 1024), (8192, 1024), (4096, 2048))
QUANTISER_SHAPES = SHAPES[:2]
ROWS = (1, 16, 17, 32)
EPILOGUES = {"store": 0, "residual": 1, "silu_mul": 2, "logits": 3}


def sha(*tensors) -> str:
    """sha256 over the bytes of the tensors (any dtype, bf16 included)."""
    import torch
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.contiguous().cpu().view(torch.uint8).numpy().tobytes())
    return h.hexdigest()


def inputs(i: int, N: int, K: int):
    """Seeded on the CPU: W with per-block magnitudes spread over 2^-6 .. 2^2 (neighbouring scales differ), 32 rows of x and residual."""
    import torch
    g = torch.Generator().manual_seed(700 + i)
    mag = torch.exp2(torch.randint(-6, 3, (N, K // 32, 1), generator=g).float()).expand(N, K // 32, 32).reshape(N, K)
    W = (torch.randn(N, K, generator=g) * mag * 0.05).bfloat16()
    x = torch.randn(32, K, generator=g).bfloat16()
    res = torch.randn(32, N, generator=g).bfloat16()
    return W, x, res


def compute() -> dict:
    import torch
    from aha_amd import ops, quant
    dev = torch.device("cuda:0")
    out = {}
    for i, (N, K) in enumerate(SHAPES):
        W, x, res = inputs(i, N, K)
        q8, s8, wr8 = quant.quantize_mxfp8(W)
        q4, s4, wr4 = quant.quantize_mxfp4(W)
        assert len(torch.unique(s8)) >= 5 and len(torch.unique(s4)) >= 5
        if (N, K) in QUANTISER_SHAPES:
            out[f"quantize_mxfp8/{N}x{K}"] = sha(*ops.quantize_mxfp8(W.to(dev)))
            out[f"quantize_mxfp4/{N}x{K}"] = sha(*ops.quantize_mxfp4(W.to(dev)))
        q8, s8, wr8, q4, s4, wr4, x, res = (t.to(dev) for t in (q8, s8, wr8, q4, s4, wr4, x, res))
        for R in ROWS:
            xs, rs = x[:R].contiguous(), res[:R].contiguous()
            for name, epi in EPILOGUES.items():
                if name == "silu_mul" and N % 32:
                    continue   # the gate / up block layout needs whole 32-row blocks
                r = rs if name == "residual" else None
                calls = {"bf16_on_mxfp8": lambda: ops.gemv_rows(wr8, xs, epi, r), "bf16_on_mxfp4": lambda: ops.gemv_rows(wr4, xs, epi, r),
                         "mxfp8": lambda: ops.gemv_rows_mxfp8(q8, s8, xs, epi, r), "mxfp4": lambda: ops.gemv_rows_mxfp4(q4, s4, xs, epi, r)}
                for form, call in calls.items():
                    got = call()
                    out[f"{form}/{N}x{K}/R{R}/{name}"] = sha(*got) if name == "logits" else sha(got)
    return out


if __name__ == "__main__":
    result = compute()
    print(json.dumps(result, indent=1))
    if len(sys.argv) > 1:
        os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
        with open(sys.argv[1], "w") as f:
            json.dump(result, f, indent=1, sort_keys=True)
