"""-m gpu: exception rows of the exact 13-bit weight copies -- a matrix with a few finite weights below its window is packed all the same,
and the twin kernel gemv_kernel_rows_pk13 computes the rows that hold one from the bf16 matrix: still the bf16 matvec on W, bit for bit.

  1. the device check and pack with rows equal aha_amd/quant.py: the same base, counts and row list, the same bytes outside the flagged
     weights; 16 rows are packed, 17 are not, Inf / NaN are not; the old entry keeps its contract;
  2. ops.gemv_pk13_rows(pack(W), W, rows, x, ...) == ops.gemv_epi(W, x, ...) on every output bit (and the argmax): K = 4096 and 8192, with
     and without norm weights, STORE / RESIDUAL N = 5 and 3080, SILU_MUL I = 32 and 3088, LOGITS N = 9 and 6160 (the large ones make a
     block walk a second tile).  Planted weights of about 1e-30: in row 0, in the last row (N = 5, 9: in a ragged tile), in a row of the
     second tile round, in unit 0 of one row and unit 1 of another (K = 8192), twice in one row, in a gate row and an up row of one output
     row and of different ones, and in 16 rows at once.  Flagged rows hold zeros apart from the planted weights (the code the copy has
     there decodes to a weight near the top of the window: a row that is not patched is off by 28 orders of magnitude), one case per
     epilogue plants into Gaussian rows, and for LOGITS the flagged row is the argmax, tied with an equal row behind it;
  3. a two-layer model with one such weight in gate+up (read from its copy by plan) and one in lm_head decodes the same tokens and logit
     bits with the switch at 0, 1 and 2, says so in its status lines, and reads fewer bytes than the bf16 run.
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_weights_fp8_cpu import bf16_bits  # noqa: E402
from test_weights_fp8_gpu import prompts  # noqa: E402
from test_wpack_cpu import LOGITS, RESIDUAL, SILU_MUL, STORE, edge_weights  # noqa: E402
from test_wpack_gpu import greedy, model_weights  # noqa: E402

pytestmark = pytest.mark.gpu

TINY = 1e-30          # bf16 E = 27: E >> 1 = 13, far below the window of a matrix whose maximum is about 0.1 (E >> 1 = 61, base 46)


# ---- 1. the check and the pack ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,K", [(64, 4096), (48, 8192)])
def test_device_pack_with_rows_equals_the_python_restatement(gpu, N, K):
    from aha_amd import ops, quant
    W = edge_weights(N, K, seed=N + 1)
    where = [(0, 0), (N - 1, K - 1), (17, 4095), (17, K - 4096), (5, 1234)]
    for r, c in where:
        W[r, c] = TINY if (r + c) & 1 else -TINY
    bh, nonfinite, rows = quant.check_pk13_rows(W)
    assert nonfinite == 0 and rows == [0, 5, 17, N - 1]
    P, gbh, grows, below, gnonf = ops.pack_pk13_rows(W.to(gpu))
    assert (gbh, grows, below, gnonf) == (bh, rows, len(where), 0) and P is not None and P.shape == (N, K // 4096, 6656)
    # the same matrix everywhere but at the flagged weights, and W itself once the flagged rows come from W
    flagged = torch.zeros(N, K, dtype=torch.bool)
    for r, c in where:
        flagged[r, c] = True
    got = quant.unpack_pk13(P.cpu(), bh)
    assert torch.equal(bf16_bits(got)[~flagged], bf16_bits(W)[~flagged])
    assert torch.equal(bf16_bits(quant.unpack_pk13_rows(P.cpu(), bh, W, grows)), bf16_bits(W))
    # byte for byte the restatement's copy in every unit without a flagged weight, and outside the weight's three bytes elsewhere
    ref = quant.pack_pk13_rows(W, bh)
    diff = {(int(r), int(u)) for r, u, _ in torch.nonzero(P.cpu() != ref).tolist()}
    assert diff <= {(r, c // 4096) for r, c in where}, diff
    assert int((P.cpu() != ref).sum()) <= 3 * len(where)          # a low byte, a code nibble, a sign bit per weight
    # the old entry: the count, nothing packed
    P0, bh0, bad0 = ops.pack_pk13(W.to(gpu))
    assert P0 is None and (bh0, bad0) == quant.check_pk13(W) == (bh, len(where))
    # a smaller cap than the rows: checked, not packed
    P1, _, rows1, _, _ = ops.pack_pk13_rows(W.to(gpu), cap=3)
    assert P1 is None and rows1 == rows[:3]
    # Inf / NaN: not packed, the rows still reported
    Wn = W.clone()
    Wn[3, 7] = float("inf")
    Wn[4, 9] = float("nan")
    P2, bh2, rows2, below2, nonf2 = ops.pack_pk13_rows(Wn.to(gpu))
    assert P2 is None and (bh2, rows2, below2, nonf2) == (bh, rows, len(where), 2) and quant.check_pk13_rows(Wn) == (bh, 2, rows)


def test_sixteen_rows_are_packed_and_seventeen_are_not(gpu):
    from aha_amd import ops, quant
    W = edge_weights(80, 4096, seed=9)
    rows16 = [0, 1, 2, 3, 4, 9, 15, 16, 31, 32, 47, 48, 63, 64, 78, 79]
    for i, r in enumerate(rows16):
        W[r, (i * 257) % 4096] = TINY
        W[r, (i * 911 + 5) % 4096] = -TINY          # twice in every row: 32 weights, 16 rows
    P, bh, rows, below, nonf = ops.pack_pk13_rows(W.to(gpu))
    assert P is not None and rows == rows16 == quant.check_pk13_rows(W)[2] and (below, nonf) == (32, 0)
    W[40, 100] = TINY
    P, bh, rows, below, nonf = ops.pack_pk13_rows(W.to(gpu))
    assert P is None and rows is None and (below, nonf) == (33, 0) and len(quant.check_pk13_rows(W)[2]) == 17


# ---- 2. the matvec ----------------------------------------------------------------------------------------------------------------------
_BASE = {}


def base(gpu, K):
    """(6176, K) normal(0, 0.02) bf16 inside the window (with zeros), x, a residual vector and norm weights; one K resident at a time."""
    if K not in _BASE:
        _BASE.clear()
        g = torch.Generator(device=gpu).manual_seed(900 + K)
        W = torch.randn(6176, K, generator=g, device=gpu) * 0.02
        W = torch.where(W.abs() < 2.0 ** -24, torch.zeros_like(W), W).bfloat16()
        x = torch.randn(K, generator=g, device=gpu)
        x = torch.where(x.abs() < 0.05, torch.full_like(x, 0.5), x).bfloat16()          # non-zero in every column
        res = torch.randn(6176, generator=g, device=gpu).bfloat16()
        nw = (1.0 + 0.1 * torch.randn(K, generator=g, device=gpu)).bfloat16()
        _BASE[K] = (W, x, res, nw)
    return _BASE[K]


def fused(j, up):
    """Row of the fused gate / up matrix behind output row j."""
    return (j >> 4) * 32 + (j & 15) + (16 if up else 0)


def cases(epi, K):
    """[(matrix rows N, [(row, column)], zero the flagged rows first?)]"""
    u1 = K - 4096          # a column of the last unit (unit 1 at K = 8192)
    if epi in (STORE, RESIDUAL):
        big = 3080         # 770 tiles of 4 rows on 768 blocks: rows 3072 .. 3079 are the second round of blocks 0 and 1
        return [(5, [(0, 3), (4, K - 1)], True),                                         # row 0; the last row, in a ragged tile
                (5, [(4, 100), (4, u1 + 4000)], True),                                   # twice in one row
                (big, [(0, 0), (3079, K - 1), (3073, 777), (1500, 5), (1501, u1 + 5)], True),      # second round; unit 0 / unit 1
                (big, [(r, (r * 37) % K) for r in (0, 1, 2, 3, 4, 5, 777, 1024, 2047, 2048, 3071, 3072, 3075, 3076, 3078, 3079)], True),
                (big, [(2, 9), (3074, u1 + 9)], False)]                                  # into Gaussian rows
    if epi == SILU_MUL:
        big = 3088         # output rows: 772 tiles on 768 blocks, rows 3072 .. 3087 are the second round of blocks 0 .. 3
        return [(64, [(fused(5, False), 3), (fused(20, True), K - 1), (fused(31, False), 8), (fused(31, False), u1 + 2000)], True),
                (64, [(fused(0, False), 11), (fused(0, True), u1 + 12)], False),         # gate and up of one output row (Gaussian rows)
                (2 * big, [(fused(0, True), 0), (fused(3087, False), K - 1), (fused(3073, True), 5), (fused(1500, False), 6),
                           (fused(1501, True), u1 + 6)], True),
                (2 * big, [(fused(j, j & 1 == 1), (j * 53) % K) for j in (0, 1, 2, 3, 15, 16, 17, 1023, 2048, 3071, 3072, 3073, 3080, 3085, 3086,
                                                                           3087)], True),
                (2 * big, [(fused(7, False), 9), (fused(7, True), 10), (fused(3075, True), u1 + 9)], False)]
    big = 6160             # LOGITS, R = 2: 770 tiles of 8 rows on 768 blocks, rows 6144 .. 6159 are the second round of blocks 0 and 1
    return [(9, [(0, 3), (8, K - 1)], True),                                             # the last row alone in a ragged tile
            (9, [(1, 100), (1, u1 + 4000)], True),
            (big, [(0, 0), (6159, K - 1), (6145, 777), (3000, 5), (3001, u1 + 5)], True),
            (big, [(r, (r * 37) % K) for r in (0, 1, 2, 7, 8, 9, 777, 2048, 4095, 4096, 6143, 6144, 6145, 6151, 6158, 6159)], True),
            (big, [(2, 9), (6150, u1 + 9)], False)]


def run_both(ops, epi, W, P, bh, rows, x, nw, res):
    """[(got, want, argmax got, argmax want)] without and with norm weights."""
    out = []
    for norm in (False, True):
        kw = dict(norm_w=nw if norm else None, eps=1e-6, residual=res if epi == RESIDUAL else None)
        got = ops.gemv_pk13_rows(P, bh, W, rows, x, epi, **kw)
        want = ops.gemv_epi(W, x, epi, **kw)
        if epi == LOGITS:
            assert torch.equal(got[0].view(torch.int32), want[0].view(torch.int32)), norm
            assert got[1] == want[1] == int(torch.argmax(want[0])), norm
            out.append((got[0], want[0], got[1], want[1]))
        else:
            assert got.shape == want.shape and torch.equal(bf16_bits(got), bf16_bits(want)), norm
            out.append((got, want, None, None))
            if epi == RESIDUAL:          # the output aliasing the residual
                ya, yb = res.clone(), res.clone()
                ops.gemv_pk13_rows(P, bh, W, rows, x, epi, norm_w=kw["norm_w"], residual=ya, out=ya)
                ops.gemv_epi(W, x, epi, norm_w=kw["norm_w"], residual=yb, out=yb)
                assert torch.equal(bf16_bits(ya), bf16_bits(yb)) and torch.equal(bf16_bits(ya), bf16_bits(got)), norm
    return out


@pytest.mark.parametrize("K", [4096, 8192])
@pytest.mark.parametrize("epi", [STORE, RESIDUAL, SILU_MUL, LOGITS])
def test_matvec_with_exception_rows_is_bit_identical_to_the_bf16_matvec(gpu, epi, K):
    from aha_amd import ops
    Wall, x, res_all, nw = base(gpu, K)
    for N, where, zero in cases(epi, K):
        W = Wall[:N].clone()
        want_rows = sorted({r for r, _ in where})
        if zero:
            W[want_rows] = 0
        sx = torch.sign(x.float()).cpu()
        for r, c in where:
            W[r, c] = TINY * float(sx[c])          # every planted product positive: two in a row cannot cancel
        P, bh, rows, below, nonf = ops.pack_pk13_rows(W)
        assert P is not None and rows == want_rows and (below, nonf) == (len(where), 0), (N, rows)
        n_out = N // 2 if epi == SILU_MUL else N
        res = res_all[:n_out].contiguous()
        for got, want, _, _ in run_both(ops, epi, W, P, bh, rows, x, nw, res):
            # the rows in question come out non-zero: a zero row with a planted weight gives about 1e-30 (times the up row for SILU_MUL)
            outs = sorted({((r >> 5) * 16 + (r & 15)) if epi == SILU_MUL else r for r in want_rows})
            if epi != RESIDUAL:
                assert bool((want.float()[outs] != 0).all()), (N, outs)
                if zero and epi != SILU_MUL:
                    assert float(want.float()[outs].abs().max()) < 1e-25, (N, outs)
            assert bool(torch.isfinite(got.float()).all())
        # no list: the plain kernel on the same copy computes something else in exactly those rows
        if zero and epi in (STORE, LOGITS):
            plain = ops.gemv_pk13(P, bh, x, epi)
            plain = plain[0] if epi == LOGITS else plain
            ref = ops.gemv_epi(W, x, epi)
            ref = ref[0] if epi == LOGITS else ref
            differ = torch.nonzero(plain.float() != ref.float()).flatten().tolist()
            assert differ == want_rows, (N, differ)


@pytest.mark.parametrize("K", [4096, 8192])
def test_a_flagged_row_that_is_the_argmax_wins_its_tie_with_a_later_row(gpu, K):
    from aha_amd import ops
    Wall, x, _, nw = base(gpu, K)
    for N, first, later in ((9, 3, 8), (6160, 2050, 6150), (6160, 6146, 6147)):
        W = Wall[:N].clone()
        big = (0.05 * torch.sign(x.float())).bfloat16()          # a logit far above every Gaussian row's
        W[first] = big
        W[later] = big
        c = K - 4096 + 77
        W[later, c] = 0
        W[first, c] = TINY          # the rows differ in one weight that does not reach the rounded sum: a tie
        P, bh, rows, below, nonf = ops.pack_pk13_rows(W)
        assert rows == [first] and P is not None
        for got, want, am, am_want in run_both(ops, LOGITS, W, P, bh, rows, x, nw, None):
            assert am == am_want == first and float(want[first]) == float(want[later]) == float(want.max()), (N, first, later)
        # and the other way round: the flagged row behind its equal
        W[first, c] = 0
        W[later, c] = -TINY
        P, bh, rows, _, _ = ops.pack_pk13_rows(W)
        assert rows == [later]
        for got, want, am, am_want in run_both(ops, LOGITS, W, P, bh, rows, x, nw, None):
            assert am == am_want == first and float(want[first]) == float(want[later]), (N, first, later)


# ---- 3. the model -----------------------------------------------------------------------------------------------------------------------
def test_model_with_exception_rows_decodes_the_same_bits(gpu):
    from aha_amd.model import HipInferenceModel
    cfg, w = model_weights()
    wn = dict(w)
    gate, head = "model.layers.0.mlp.gate_proj.weight", "lm_head.weight"
    wn[gate] = w[gate].clone()
    wn[gate][1234, 2000] = TINY          # gate row 1234 = row 77 * 32 + 2 of the fused matrix
    wn[head] = w[head].clone()
    wn[head][4001, 4095] = -TINY
    m = HipInferenceModel(cfg, wn)
    try:
        st = m.pk13_status()
        assert len(st) == 4 * 2 + 1
        assert st.pop("layers.0.mlp.gate_proj/up_proj.weight") == f"1 weights outside the window: packed, rows {77 * 32 + 2} read from bf16"
        assert st.pop("lm_head.weight") == "1 weights outside the window: packed, rows 4001 read from bf16"
        assert set(st.values()) == {"packed"}, st
        ids = prompts(24, (19,), vocab=4096)[0]
        t1, l1, p1 = greedy(m, ids)          # by plan: gate+up from its copy
        m.debug_pk13_single(0)
        t0, l0, p0 = greedy(m, ids)
        m.debug_pk13_single(2)               # every copy, lm_head's among them
        t2, l2, p2 = greedy(m, ids)
        assert t1 == t0 == t2 and len(t1) == 13 and len(set(t1)) > 3
        assert np.array_equal(l1, l0) and np.array_equal(l2, l0)
        assert p1["launches"] == p0["launches"] == p2["launches"] > 0 and p2["bytes"] < 0.85 * p0["bytes"] and p2["bytes"] < p1["bytes"] < p0["bytes"]
        # the launch-per-step path reduces the twin's own partials
        m.clear_cache()
        _, tok = m.forward_initial(ids, 0)
        for i in range(3):
            lg, tok = m.forward_step(tok, len(ids) + i)
            assert tok == t1[i + 1] == int(np.argmax(lg))
    finally:
        m.close()
