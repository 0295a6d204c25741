"""-m gpu: batched greedy generation (aha_hip_generate_batch / HipInferenceModel.generate_batch) and its two kernels.

  * gemv_rows (the R-row projection): against an f64 matmul on every model shape and epilogue, and each row of an R-row call bit-identical
    to the same row computed alone;
  * attn_decode_batch (all rows' fused decode attention in one launch): bit-identical per sequence to the single-sequence kernel
    (aha_hip_debug_attn_decode_fused) on mixed cache lengths, each append in its own slot, no other page touched;
  * the driver: exact greedy sequences on decisive-margin checkpoints (tests/decisive.py) against the oracle and generate_generic on each
    prompt alone, isolation between the sequences of a batch, stop tokens, the model's state afterwards, one attention launch per layer
    per step.
"""
import sys
import os

import numpy as np
import pytest
import torch

from aha_amd._lib import AhaHipError
from aha_amd.configs import tiny_qwen3, tiny_qwen3vl
from aha_amd.weights import qwen3_text_weights, qwen3vl_weights
from oracle import qwen3 as oq
from oracle.numerics import Numerics

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import decisive  # noqa: E402

pytestmark = pytest.mark.gpu

NM = Numerics("bf16", matmul_f64=True)
LOGIT_TOL_STD, LOGIT_RMS_STD = 0.05, 0.02   # tests/test_model_gpu.py check_logits: the decode-vs-oracle bound

# (N, K) of qkv, o_proj, gate+up, down_proj, lm_head at 0.6B and 8B
SHAPES_06B = [(4096, 1024), (1024, 2048), (6144, 1024), (1024, 3072), (151936, 1024)]
SHAPES_8B = [(6144, 4096), (4096, 4096), (24576, 4096), (4096, 12288), (151936, 4096)]


def ulp_bf16(x):
    e = torch.floor(torch.log2(x.abs().clamp_min(1e-30)))
    return torch.pow(2.0, e - 7)


def assert_close_ulps(got, ref, ulps, frac_exact, what):
    """The bound test_ops_gpu.py holds the matvec to: ulps bf16 ulps at max(|ref|, rms of the tensor), frac_exact bit-identical."""
    got, ref = got.float(), ref.float()
    assert torch.isfinite(got).all(), what
    rms = ref.pow(2).mean().sqrt()
    bad = (got - ref).abs() > ulps * ulp_bf16(torch.maximum(ref.abs(), rms))
    assert not bad.any(), f"{what}: {int(bad.sum())}/{bad.numel()} elements off by more than {ulps} ulp"
    fe = float((got == ref).float().mean())
    assert fe >= frac_exact, f"{what}: only {fe:.4f} bit-identical"


def rnd(shape, seed, std=1.0, mean=0.0, dev="cuda"):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(shape, generator=g) * std + mean).to(torch.bfloat16).to(dev)


def f64_linear(x, W):
    """(R, K) . (N, K)^T in f64, in column chunks (the f64 copy of a 151936 x 4096 matrix would be 5 GB)."""
    out = []
    xd = x.double()
    for n0 in range(0, W.shape[0], 16384):
        out.append(xd @ W[n0:n0 + 16384].double().T)
    return torch.cat(out, 1)


def pairs_to_gate_up(W):
    """(2I, K) in the 16-row gate / up block layout -> (gate (I, K), up (I, K))."""
    b = W.view(-1, 2, 16, W.shape[1])
    return b[:, 0].reshape(-1, W.shape[1]), b[:, 1].reshape(-1, W.shape[1])


# ---- kernel A ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,K", SHAPES_06B + SHAPES_8B)
def test_gemv_rows_against_f64_and_row_isolation(gpu, N, K):
    from aha_amd import ops
    W = rnd((N, K), 1, 0.02)
    x = rnd((32, K), 2)
    res = rnd((32, N), 3)
    ref = f64_linear(x, W)
    lm_head = N == 151936
    for R in (1, 5, 16, 17, 32):
        xs = x[:R].contiguous()
        if lm_head:
            lg, am = ops.gemv_rows(W, xs, ops.GEMV_ROWS_LOGITS)
            assert_close_ulps(lg, ref[:R].to(torch.bfloat16), 1, 0.98, f"logits R={R}")
            assert torch.equal(am.cpu(), torch.argmax(lg, 1).cpu()), "argmax: the first maximal index of the logits"
            alone = [ops.gemv_rows(W, x[r:r + 1].contiguous(), ops.GEMV_ROWS_LOGITS)[0] for r in range(R)]
            assert all(torch.equal(lg[r], alone[r][0]) for r in range(R)), "a row's logits depend on the other rows"
            continue
        y = ops.gemv_rows(W, xs, ops.GEMV_ROWS_STORE)
        assert_close_ulps(y, ref[:R].to(torch.bfloat16), 1, 0.98, f"store R={R}")
        yr = ops.gemv_rows(W, xs, ops.GEMV_ROWS_RESIDUAL, res[:R].contiguous())
        ref_r = (res[:R].float() + ref[:R].to(torch.bfloat16).float()).to(torch.bfloat16)
        assert_close_ulps(yr, ref_r, 1, 0.98, f"residual R={R}")
        ys = None
        if N % 32 == 0 and N > K:   # gate+up shapes: SiLU(gate) * up pairs
            ys = ops.gemv_rows(W, xs, ops.GEMV_ROWS_SILU_MUL)
            Wg, Wu = pairs_to_gate_up(W)
            lhs = torch.nn.functional.silu(f64_linear(xs, Wg).to(torch.bfloat16).float()).to(torch.bfloat16).float()
            ref_s = (lhs * f64_linear(xs, Wu).to(torch.bfloat16).float()).to(torch.bfloat16)
            assert_close_ulps(ys, ref_s, 2, 0.97, f"silu_mul R={R}")
        for r in range(R):   # each row alone: the same bits
            x1 = x[r:r + 1].contiguous()
            assert torch.equal(y[r], ops.gemv_rows(W, x1, ops.GEMV_ROWS_STORE)[0]), (R, r)
            assert torch.equal(yr[r], ops.gemv_rows(W, x1, ops.GEMV_ROWS_RESIDUAL, res[r:r + 1].contiguous())[0]), (R, r)
            if ys is not None:
                assert torch.equal(ys[r], ops.gemv_rows(W, x1, ops.GEMV_ROWS_SILU_MUL)[0]), (R, r)


# ---- kernel B ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nh,kvh", [(4, 2), (16, 8), (32, 8)])
def test_attn_decode_batch_bit_identical_to_the_single_sequence_kernel(gpu, nh, kvh):
    from aha_amd import ops
    lens = [1, 63, 64, 65, 256, 257, 1000, 4097]
    page_elems = 2 * kvh * 64 * 128
    npg = [(L + 63) // 64 for L in lens]
    P = sum(npg) + 3
    pool = rnd((P, page_elems), 5)
    perm = torch.randperm(P, generator=torch.Generator().manual_seed(6))
    ptrs = (pool.data_ptr() + perm.to(torch.int64) * page_elems * 2).to("cuda")
    page0 = list(np.cumsum([0] + npg[:-1]))
    R = len(lens)
    qkv = rnd((R, (nh + 2 * kvh) * 128), 7)
    qn, kn = rnd((128,), 8, 0.1, 1.0), rnd((128,), 9, 0.1, 1.0)
    ang = torch.rand(R, 64, generator=torch.Generator().manual_seed(10)) * 6.0
    rope = torch.cat([torch.cos(ang), torch.sin(ang)], 1).to(torch.bfloat16).float().to("cuda").contiguous()
    scale = float(torch.tensor(128 ** -0.5).to(torch.bfloat16))
    before = pool.clone()
    o = ops.attn_decode_batch(qkv, qn, kn, rope, ptrs, page0, lens, nh, kvh, 1e-6, scale)
    after_batch = pool.clone()
    pool.copy_(before)
    for r, L in enumerate(lens):
        p0 = int(page0[r])
        ref = ops.debug_attn_decode_fused(qkv[r].contiguous(), qn, kn, rope[r].contiguous(), ptrs[p0:].contiguous(), L, nh, kvh, 1e-6, scale)
        assert torch.equal(o[r].view(torch.int16), ref.view(torch.int16)), f"row {r} (cache length {L}) differs from the single-sequence kernel"
    torch.cuda.synchronize()
    assert torch.equal(pool.view(torch.int16), after_batch.view(torch.int16)), "the appends differ from the single-sequence kernel's"
    # only the page holding each sequence's new slot changed; every other page is byte-identical
    changed = set(torch.nonzero((after_batch.view(torch.int16) != before.view(torch.int16)).any(1)).flatten().tolist())
    expect = {int(perm[int(page0[r]) + (L - 1) // 64]) for r, L in enumerate(lens)}
    assert changed == expect


# ---- the driver ----------------------------------------------------------------------------------------------------------------
PROMPT_LENS = [1, 63, 64, 65, 300]
MAX_NEW = 70   # the 1-token prompt's appends cross the page edge at 64


def prompts_for(n, seed, vocab, lens=PROMPT_LENS):
    g = np.random.default_rng(seed)
    return [[int(x) for x in g.integers(0, vocab, size=lens[i % len(lens)])] for i in range(n)]


@pytest.fixture(scope="module")
def tied(gpu):
    from aha_amd.model import HipInferenceModel
    cfg = tiny_qwen3(layers=3, hidden=512, heads=4, kv_heads=2, inter=1024, vocab=2048, tie=True)
    w = qwen3_text_weights(cfg, seed=0)
    decisive.make_tied_decisive(w, "model.embed_tokens.weight", "model.norm.weight", scale=32.0, seed=7, n_text=2000)
    m = HipInferenceModel(cfg, w)
    yield cfg, w, m
    m.close()


@pytest.fixture(scope="module")
def untied_vl(gpu):
    from aha_amd.model import HipInferenceModel
    cfg = tiny_qwen3vl()
    w = qwen3vl_weights(cfg, seed=0)
    pi = decisive.make_untied_decisive(w, "model.language_model.embed_tokens.weight", "lm_head.weight", scale=32.0, seed=7, n_text=2000)
    m = HipInferenceModel(cfg, w)
    yield cfg, m, pi
    m.close()


def check_logits(got, ref, what):
    ref = np.asarray(ref, dtype=np.float32).reshape(-1)
    std = float(ref.std())
    diff = np.abs(got - ref)
    assert np.isfinite(got).all(), what
    assert float(diff.max()) <= LOGIT_TOL_STD * std, what
    assert float(np.sqrt((diff ** 2).mean())) <= LOGIT_RMS_STD * std, what


def test_generate_batch_tied_qwen3_exact_greedy(tied):
    from aha_amd.model import generate_generic
    cfg, w, m = tied
    pool = prompts_for(17, 21, 2000)
    o = oq.OracleQwen3(cfg, w, Numerics("bf16", matmul_f64=True))
    oracle = {}
    for i in range(len(PROMPT_LENS)):   # the oracle on one prompt of every length, margins asserted per step
        o.clear_cache()
        toks, lgs = oq.greedy_generate(o, pool[i], MAX_NEW, return_logits=True)
        assert min(decisive.margin_std(l) for l in lgs) >= 0.5
        oracle[i] = (toks, lgs[-1])
    single = {}
    for B in (1, 3, 16, 17, 40):
        prompts = [pool[i % len(pool)] for i in range(B)]
        got, lg = m.generate_batch(prompts, MAX_NEW, want_logits=True)
        assert m.cache_len() == 0
        for j, p in enumerate(prompts):
            i = j % len(pool)
            if i not in single:
                single[i] = generate_generic(m, p, MAX_NEW, device_loop=True)[0]
            assert got[j] == single[i], (B, j, len(p))
            assert got[j] == [p[-1] ^ 1, p[-1]] * (MAX_NEW // 2), (B, j)
            if i in oracle:
                assert got[j] == oracle[i][0], (B, j)
                check_logits(lg[j], oracle[i][1].numpy(), f"B={B} seq {j}")


def test_generate_batch_untied_qwen3vl_text_exact_greedy(untied_vl):
    from aha_amd.model import generate_generic
    cfg, m, pi = untied_vl
    prompts = prompts_for(17, 22, 2000)
    got = m.generate_batch(prompts, MAX_NEW, max_tokens_per_pass=256)   # several prefill passes
    for j, p in enumerate(prompts):
        walk, t = [], p[-1]
        for _ in range(MAX_NEW):
            t = int(pi[t])
            walk.append(t)
        assert got[j] == walk, j
        assert got[j] == generate_generic(m, p, MAX_NEW, device_loop=True)[0], j
    assert m.cache_len() == 0


@pytest.fixture(scope="module", params=["narrow", "wide"])
def rand_model(gpu, request):
    from aha_amd.model import HipInferenceModel
    if request.param == "narrow":
        cfg = tiny_qwen3(layers=3, hidden=512, heads=4, kv_heads=2, inter=1024, vocab=4096)
    else:
        cfg = tiny_qwen3(layers=2, hidden=1024, heads=16, kv_heads=8, inter=3072, vocab=4096)
    m = HipInferenceModel(cfg, qwen3_text_weights(cfg, seed=0))
    if request.param == "wide":
        m.debug_scramble_pages(True)
    yield cfg, m
    m.close()


def test_generate_batch_sequences_are_isolated(rand_model):
    """Random weights, no stop tokens: a sequence's tokens and logits do not depend on the other prompts (lengths kept), and permuting
    the batch permutes the results."""
    cfg, m = rand_model
    lens = [1, 63, 64, 65, 300, 7, 129, 64] * 5   # 40 sequences: two row groups
    seqs = prompts_for(len(lens), 31, cfg.vocab_size, lens)
    other = prompts_for(len(lens), 32, cfg.vocab_size, lens)
    base, lb = m.generate_batch(seqs, 20, want_logits=True)
    alt, la = m.generate_batch([other[j] if j % 2 else s for j, s in enumerate(seqs)], 20, want_logits=True)
    for j in range(0, len(seqs), 2):
        assert alt[j] == base[j], j
        assert np.array_equal(la[j].view(np.uint32), lb[j].view(np.uint32)), j
    perm = np.random.default_rng(33).permutation(len(seqs))
    pg, pl = m.generate_batch([seqs[i] for i in perm], 20, want_logits=True)
    for k, i in enumerate(perm):
        assert pg[k] == base[i]
        assert np.array_equal(pl[k].view(np.uint32), lb[i].view(np.uint32))
    assert all(len(t) == 20 for t in base)


def test_generate_batch_stop_tokens(tied):
    from aha_amd.model import HipInferenceModel
    cfg, w, _ = tied
    a = 600
    prompts = [[5, 9, a], [11, a ^ 1], [40, 41, 42, 43], [100] * 70]
    cfg2 = tiny_qwen3(layers=3, hidden=512, heads=4, kv_heads=2, inter=1024, vocab=2048, tie=True)
    cfg2.eos_token_ids = [a]
    m = HipInferenceModel(cfg2, w)
    try:
        got = m.generate_batch(prompts, 9)
    finally:
        m.close()
    assert got[0] == [a ^ 1, a]                # the second token is the stop token: kept, and the sequence ends
    assert got[1] == [a, a ^ 1, a]             # a first token equal to the stop token does not stop
    assert got[2] == [42, 43] * 4 + [42] and got[3] == [101, 100] * 4 + [101]


def test_generate_batch_state_errors_and_launches(tied):
    cfg, w, m = tied
    ids = prompts_for(1, 41, 2000, [90])[0]
    m.clear_cache()
    l0, t0 = m.forward_initial(ids, 0)
    l1, _ = m.forward_step(t0, len(ids))
    m.clear_cache()
    prompts = prompts_for(5, 42, 2000)
    m.set_profiling(False)
    m.set_profiling(True)
    m.generate_batch(prompts, 12)
    prof = m.get_profile("attn_decode_batch")
    m.set_profiling(False)
    assert prof["launches"] == cfg.num_hidden_layers * 11, prof   # one launch per layer per decode step, none per sequence
    assert m.cache_len() == 0
    for bad in ([[1, 2], []], [[1, 2], [3, 5000]]):
        with pytest.raises(AhaHipError):
            m.generate_batch(bad, 4)
        assert m.cache_len() == 0
    with pytest.raises(AhaHipError):
        m.generate_batch([[1, 2]], 0)
    k0, s0 = m.forward_initial(ids, 0)
    k1, _ = m.forward_step(s0, len(ids))
    m.clear_cache()
    assert s0 == t0 and np.array_equal(k0.view(np.uint32), l0.view(np.uint32)) and np.array_equal(k1.view(np.uint32), l1.view(np.uint32))
    assert m.generate_batch(prompts[:2], 4) == [[p[-1] ^ 1, p[-1]] * 2 for p in prompts[:2]]
