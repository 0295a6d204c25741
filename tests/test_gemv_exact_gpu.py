"""-m gpu: the single-sequence matvec on inputs whose dot products are exact (tests/gemv_exact.py), every weight form against the same
integer reference with zero tolerance -- not against the bf16 kernel, and not through the quantiser.

  1. bf16 (gemv_kernel): shapes that between them select every (R, U, epilogue, FAST, PRO) the plan can reach (asserted through
     aha_hip_debug_plan_gemv, the function the launch itself calls), multi-tile FAST walks for every epilogue.  Per shape, with and without
     the exact norm prologue: STORE, RESIDUAL (and again with the output aliasing the residual), LOGITS (every logit bit and the argmax
     over planted ties: the first maximal index), PARTIAL_F32 through aha_hip_debug_gemv_partial_f32 -- all bit for bit -- and SILU_MUL
     through both weight layouts, whose dot products are exact and whose f32 expf / divide are held to test_gemv_gate_up's bound;
  2. one Gaussian case per R against the f64 chain with test_gemv's bound: 1 / rms values that are not a power of two;
  3. MXFP8, MXFP4 and the 13-bit copies over their own shape lists (which prove cover of their instantiations in their own files);
  4. no case silently left out: each test counts the cases it ran against a count computed from the lists.
"""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gemv_exact as gx  # noqa: E402
from gemv_exact import LOGITS, PARTIAL_F32, RESIDUAL, SILU_MUL, SILU_SHIFT, STORE  # noqa: E402
from test_ops_gpu import assert_close_ulps  # noqa: E402
from test_weights_fp8_single_gpu import SHAPES as MX_SHAPES  # noqa: E402  (test_weights_fp4_single_gpu.py runs the same list)
from test_wpack_gpu import rows_of as pk13_rows_of  # noqa: E402

pytestmark = pytest.mark.gpu

PK13_KS = (4096, 12288)          # tests/test_wpack_gpu.py's
RAN = {}                         # (form, shape) -> cases run


def seed_of(form, rows, K):
    return 7919 * ("bf16", "mxfp8", "mxfp4", "pk13", "gauss").index(form) + 31 * rows + K


def silu_bound(got, want, what):
    """tests/test_ops_gpu.py test_gemv_gate_up's: 2 bf16 ulps, at least 0.97 of the outputs bit-identical."""
    assert_close_ulps(got, gx.as_bf16(want).float(), 2, 0.97, what)


def check_ties(c, what):
    """The planted ties exist: every target row holds the maximum, so the expected index is the smallest of them."""
    for norm, t in zip((False, True), c["ties"]):
        lg, am = gx.expected(c, LOGITS, norm)
        rows = sorted(v for k, v in t.items())
        assert len(rows) >= 2 and all(float(lg[r]) == float(lg.max()) for r in rows) and am <= rows[0], (what, norm, t, am)


# ---- 1. bf16 ----------------------------------------------------------------------------------------------------------------------------
def test_the_shapes_select_every_instantiation_the_plan_can_reach(hip_lib):
    from aha_amd import ops
    want = gx.bf16_reachable(ops.plan_gemv)
    assert len(want) == 131
    hit = gx.bf16_covered(ops.plan_gemv)
    assert hit == want, (sorted(want - hit), sorted(hit - want))
    # PARTIAL_F32 takes STORE's plans
    assert {i[:2] + i[3:] for i in gx.bf16_covered(ops.plan_gemv, (PARTIAL_F32,))} == {i[:2] + i[3:] for i in want if i[2] == STORE}
    gx.assert_multi_tile_fast(ops.plan_gemv)
    assert ops.plan_gemv(100000, 64, STORE, False)[2:] == (768, 0)        # and the general form walks several tiles


@pytest.mark.parametrize("rows,K", gx.BF16_SHAPES)
def test_bf16_matvec_gives_the_exact_sums(gpu, rows, K):
    from aha_amd import ops
    r, _, grid, _ = ops.plan_gemv(rows, K, LOGITS, False)
    assert ops.plan_gemv(rows, K, LOGITS, True)[:3:2] == (r, grid)
    c = gx.make_case(rows, K, device=gpu, seed=seed_of("bf16", rows, K), tie_plan=(r, grid))
    check_ties(c, (rows, K))
    W, res = c["W"], c["res"]
    Wg = gx.weights(c, SILU_SHIFT)
    Wu = torch.roll(Wg, 1, 0).contiguous()
    Wf = gx.fuse_gate_up(Wg, Wu) if rows % 16 == 0 else None
    ran = 0
    for norm in (False, True):
        x, kw = (c["xn"], dict(norm_w=c["nw"], eps=0.0)) if norm else (c["x"], dict(norm_w=None, eps=0.0))
        what = f"bf16 {rows} x {K} norm={norm} plan={ops.plan_gemv(rows, K, STORE, norm)}"
        gx.assert_same_bits(ops.gemv_epi(W, x, STORE, **kw), gx.expected(c, STORE, norm), what + " STORE")
        ran += 1
        want = gx.expected(c, RESIDUAL, norm)
        gx.assert_same_bits(ops.gemv_epi(W, x, RESIDUAL, residual=res, **kw), want, what + " RESIDUAL")
        y = res.clone()
        ops.gemv_epi(W, x, RESIDUAL, residual=y, out=y, **kw)
        gx.assert_same_bits(y, want, what + " RESIDUAL, the output aliasing the residual")
        ran += 1
        gx.assert_logits(ops.gemv_epi(W, x, LOGITS, **kw), gx.expected(c, LOGITS, norm), what + " LOGITS")
        ran += 1
        gx.assert_same_bits(ops.gemv_partial_f32(W, x, **kw), gx.expected(c, PARTIAL_F32, norm), what + " PARTIAL_F32")
        ran += 1
        want = gx.expected_silu_separate(c, norm)
        silu_bound(ops.gemv_gate_up(Wg, Wu, x, **kw), want, what + " SILU_MUL, separate gate / up")
        ran += 1
        if Wf is not None:
            silu_bound(ops.gemv_epi(Wf, x, SILU_MUL, **kw), want, what + " SILU_MUL, fused blocks")
            ran += 1
    assert ran == gx.bf16_case_count(rows)
    RAN["bf16", (rows, K)] = ran


# ---- 2. Gaussian inputs -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,K,R", [s + (r,) for s, r in zip(gx.GAUSSIAN_SHAPES, (1, 2, 4))])
def test_bf16_matvec_on_gaussian_inputs_against_the_f64_chain(gpu, rows, K, R):
    from aha_amd import ops
    assert ops.plan_gemv(rows, K, STORE, True)[0] == ops.plan_gemv(rows, K, RESIDUAL, False)[0] == R
    c = gx.gaussian_case(rows, K, device=gpu, seed=seed_of("gauss", rows, K))
    for norm, residual in ((False, False), (True, False), (False, True)):          # tests/test_ops_gpu.py test_gemv's, and its bound
        got = ops.gemv(c["W"], c["x"], c["nw"] if norm else None, 1e-6, c["res"] if residual else None)
        want = gx.as_bf16(gx.gaussian_expected(c, norm, residual, 1e-6)).float()
        assert_close_ulps(got, want, 1, 0.98, f"gemv {rows} x {K} R={R} norm={norm} residual={residual}")


# ---- 3. the other weight forms ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,K", MX_SHAPES)
@pytest.mark.parametrize("form", ["mxfp8", "mxfp4"])
def test_mx_matvec_gives_the_exact_sums(gpu, form, N, K):
    from aha_amd import ops
    plan, run, enc = ((ops.plan_gemv_mxfp8, ops.gemv_mxfp8, gx.encode_mxfp8) if form == "mxfp8" else
                      (ops.plan_gemv_mxfp4, ops.gemv_mxfp4, gx.encode_mxfp4))
    r, _, grid, _ = plan(N, K, LOGITS, False)
    c = gx.make_case(N, K, fp4=form == "mxfp4", device=gpu, seed=seed_of(form, N, K), tie_plan=(r, grid))
    check_ties(c, (form, N, K))
    q, s = enc(c)
    assert len(torch.unique(s)) == len(gx.BLOCK_SHIFTS)
    res = c["res"]
    ran = 0
    for norm in (False, True):
        x, kw = (c["xn"], dict(norm_w=c["nw"], eps=0.0)) if norm else (c["x"], dict(norm_w=None, eps=0.0))
        what = f"{form} {N} x {K} norm={norm} plan={plan(N, K, STORE, norm)}"
        gx.assert_same_bits(run(q, s, x, STORE, **kw), gx.expected(c, STORE, norm), what + " STORE")
        ran += 1
        want = gx.expected(c, RESIDUAL, norm)
        gx.assert_same_bits(run(q, s, x, RESIDUAL, residual=res, **kw), want, what + " RESIDUAL")
        y = res.clone()
        run(q, s, x, RESIDUAL, residual=y, out=y, **kw)
        gx.assert_same_bits(y, want, what + " RESIDUAL, the output aliasing the residual")
        ran += 1
        gx.assert_logits(run(q, s, x, LOGITS, **kw), gx.expected(c, LOGITS, norm), what + " LOGITS")
        ran += 1
        if N % 32 == 0:          # the fused gate / up layout comes in whole 32-row blocks (the entries refuse anything else)
            qs, ss = enc(c, SILU_SHIFT)
            silu_bound(run(qs, ss, x, SILU_MUL, **kw), gx.expected_silu_fused(c, norm), what + " SILU_MUL")
            ran += 1
    assert ran == gx.mx_case_count(N)
    RAN[form, (N, K)] = ran


@pytest.mark.parametrize("K", PK13_KS)
@pytest.mark.parametrize("epi", [STORE, RESIDUAL, SILU_MUL, LOGITS])
def test_pk13_matvec_gives_the_exact_sums(gpu, epi, K):
    from aha_amd import ops, quant
    ran = 0
    for n_out in pk13_rows_of(epi):
        N = 2 * n_out if epi == SILU_MUL else n_out          # matrix rows
        tie_plan = ops.plan_gemv_pk13(N, K, LOGITS, False)[:3:2] if epi == LOGITS else None
        c = gx.make_case(N, K, device=gpu, seed=seed_of("pk13", N, K), tie_plan=tie_plan)
        W = gx.weights(c, SILU_SHIFT) if epi == SILU_MUL else c["W"]
        bh, bad = quant.check_pk13(W)
        assert bad == 0
        P = quant.pack_pk13(W, bh)          # torch on the GPU: aha_amd/quant.py's restatement, not the library's pack kernel
        for norm in (False, True):
            x, kw = (c["xn"], dict(norm_w=c["nw"], eps=0.0)) if norm else (c["x"], dict(norm_w=None, eps=0.0))
            what = f"pk13 {N} x {K} epi={epi} norm={norm} plan={ops.plan_gemv_pk13(N, K, epi, norm)}"
            if epi == SILU_MUL:
                silu_bound(ops.gemv_pk13(P, bh, x, epi, **kw), gx.expected_silu_fused(c, norm), what)
            elif epi == LOGITS:
                check_ties(c, what)
                gx.assert_logits(ops.gemv_pk13(P, bh, x, epi, **kw), gx.expected(c, epi, norm), what)
            else:
                want = gx.expected(c, epi, norm)
                gx.assert_same_bits(ops.gemv_pk13(P, bh, x, epi, residual=c["res"] if epi == RESIDUAL else None, **kw), want, what)
                if epi == RESIDUAL:
                    y = c["res"].clone()
                    ops.gemv_pk13(P, bh, x, epi, residual=y, out=y, **kw)
                    gx.assert_same_bits(y, want, what + ", the output aliasing the residual")
            ran += 1
    assert ran == 2 * len(pk13_rows_of(epi))
    RAN["pk13", (epi, K)] = ran


# ---- 4. nothing left out ----------------------------------------------------------------------------------------------------------------
def test_no_case_was_left_out(gpu):
    """The (form, shape, epilogue, norm) cases the tests above ran, against the count the lists give.  The only cases a form leaves out are
    SILU_MUL on the fused layout with N % 32 != 0, and (pk13) K that is no multiple of 4096: its list holds none."""
    want = {("bf16", s): gx.bf16_case_count(s[0]) for s in gx.BF16_SHAPES}
    want.update({(f, s): gx.mx_case_count(s[0]) for f in ("mxfp8", "mxfp4") for s in MX_SHAPES})
    want.update({("pk13", (e, K)): 2 * len(pk13_rows_of(e)) for e in (STORE, RESIDUAL, SILU_MUL, LOGITS) for K in PK13_KS})
    assert all(K % 4096 == 0 for K in PK13_KS)
    for key, n in RAN.items():
        assert want[key] == n, key
    print(f"exact matvec cases run: {sum(RAN.values())} of {sum(want.values())} "
          + ", ".join(f"{f} {sum(n for k, n in RAN.items() if k[0] == f)}/{sum(n for k, n in want.items() if k[0] == f)}" for f in ("bf16", "mxfp8", "mxfp4", "pk13")))
    if not set(want) - set(RAN):          # the whole file ran (a -k selection is held to the per-shape counts above)
        assert sum(RAN.values()) == sum(want.values())
