"""-m gpu: ops.score_rows (aha_hip_score_rows, csrc/kernels_score.hip) -- the lm_head GEMM fused with the log-softmax reduction -- against a
plain f64 log-softmax of the logits.  Exact case: inputs whose every logit is a multiple of 1/8 below 12 in magnitude, so the f32 matmul
is exact in any order and the bf16 rounding changes nothing: what is left is the kernel's own reduction, held to 2^-14 (the bound
tests/test_logprobs_gpu.py holds the materialised f32 pass to) with top_id exact.  General case: Gaussian inputs, where the kernel's bf16
rounding of each logit is allowed half a bf16 ulp of the row's largest logit."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROW_BLOCK = 128   # rows of a workgroup of score_rows_kernel
BIG = (33, 151936, 1024)


def exact_inputs(R, V, K, seed):
    g = torch.Generator().manual_seed(seed)
    h = torch.randint(-3, 4, (R, K), generator=g).float()
    W = torch.zeros(V, K)
    cols = torch.randint(0, K, (V, 16), generator=g)
    W.scatter_(1, cols, torch.randint(-2, 3, (V, 16), generator=g).float() / 8)   # <= 16 non-zeros per row (duplicates overwrite)
    for r in range(min(R, 3)):   # duplicated W rows: row r's maximum is tied at two indices, and top_id must be the smaller one
        a, dst = int((h[r] @ W.T).argmax()), V - 1 - r
        if dst > a:
            W[dst] = W[a]
    return h, W


def f32_logits(h, W):
    """(R, V) f32 logits in column chunks, asserted exact: == the f64 product == its bf16 round trip."""
    out = torch.empty(h.shape[0], W.shape[0])
    for c0 in range(0, W.shape[0], 16384):
        x = h @ W[c0:c0 + 16384].T
        assert torch.equal(x.double(), h.double() @ W[c0:c0 + 16384].double().T) and torch.equal(x, x.bfloat16().float())
        out[:, c0:c0 + 16384] = x
    assert float(out.abs().max()) <= 12
    return out


def targets_for(x, seed):
    """Column 0, column V - 1, the argmax, -1, and the rest spread over the vocabulary (so over the kernel's slices)."""
    R, V = x.shape
    t = np.random.default_rng(seed).integers(0, V, size=R)
    t[::4] = (np.arange(R)[::4] * 7919) % V
    t[0] = 0
    for r, v in ((1, V - 1), (2, int(x[2 % R].argmax())), (3, -1)):
        if r < R:
            t[r] = v
    return t


def check(x64, t, got, tol):
    lp, top, tlp = got
    ref = torch.log_softmax(x64, dim=-1)
    tt = torch.as_tensor(np.maximum(t, 0))
    ref_lp = torch.where(torch.as_tensor(t) >= 0, ref.gather(1, tt[:, None])[:, 0], torch.zeros(len(t), dtype=torch.float64)).numpy()
    ref_tlp = ref.max(dim=-1).values.numpy()
    print("max |logprob - ref| %.3e, max |top_logprob - ref| %.3e" % (np.abs(lp - ref_lp).max(), np.abs(tlp - ref_tlp).max()))
    assert (np.abs(lp - ref_lp) <= tol).all() and (np.abs(tlp - ref_tlp) <= tol).all()
    assert (lp[t >= 0] <= tlp[t >= 0]).all() and (tlp <= 0).all()   # (a row without a target reports logprob 0)
    return top


def run_exact(R, V, K):
    from aha_amd import ops
    h, W = exact_inputs(R, V, K, seed=R + V + K)
    x = f32_logits(h, W)
    t = targets_for(x, seed=1)
    got = ops.score_rows(h.bfloat16().cuda(), W.bfloat16().cuda(), t)
    top = check(x.double(), t, got, np.full(R, 2.0 ** -14))
    assert np.array_equal(top, x.argmax(dim=-1).numpy())   # torch's argmax of exact values: the first maximal index
    if V >= 257:
        assert int((x == x.max(dim=-1, keepdim=True).values).sum(dim=-1).max()) >= 2, "no tied maximum was planted"
    return h, W, t, got


@pytest.mark.parametrize("K", [64, 1024])
@pytest.mark.parametrize("V", [1, 257, 5003])
@pytest.mark.parametrize("R", [1, 67, ROW_BLOCK + 1])
def test_exact_inputs(gpu, R, V, K):
    run_exact(R, V, K)


def test_exact_inputs_full_vocabulary(gpu):
    run_exact(*BIG)


@pytest.mark.parametrize("R,V,K", [(67, 5003, 1024), (1, 257, 64)])
def test_gaussian_inputs(gpu, R, V, K):
    from aha_amd import ops
    g = torch.Generator().manual_seed(5)
    h = torch.randn(R, K, generator=g).bfloat16()
    W = (torch.randn(V, K, generator=g) / K ** 0.5).bfloat16()
    x64 = h.double() @ W.double().T
    t = targets_for(x64, seed=2)
    d = 2.0 ** -9 * x64.abs().max(dim=-1).values.numpy()   # half a bf16 ulp at the row's largest logit
    top = check(x64, t, ops.score_rows(h.cuda(), W.cuda(), t), 2 * d)
    assert (x64.gather(1, torch.as_tensor(top.astype(np.int64))[:, None])[:, 0].numpy() >= x64.max(dim=-1).values.numpy() - 2 * d).all()


def test_same_inputs_same_bytes(gpu):
    from aha_amd import ops
    h, W = exact_inputs(67, 5003, 1024, seed=9)
    hd, Wd, t = h.bfloat16().cuda(), W.bfloat16().cuda(), targets_for(h @ W.T, seed=3)
    a, b = ops.score_rows(hd, Wd, t), ops.score_rows(hd, Wd, t)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
