"""-m gpu: the batched decode matvec (gemv_rows_body in its bf16, MXFP8 and MXFP4 forms, the merge kernel, argmax_rows_kernel) on inputs
whose dot products are exact (tests/gemv_rows_exact.py), against the integer reference with zero tolerance -- not against the bf16 kernel,
not through the quantiser, and not against what the kernels gave before.

  1. exact sums: every shape of ROWS_SHAPES x R in {1, 15, 16, 17, 31, 32} x epilogue x weight form, every output bit, and for LOGITS the
     argmax of every row;
  2. probes: a launch of unit vectors e_k returns column k of W for the k at and around every chunk, fragment and tail boundary;
  3. ties: planted maxima in the same merge block, across a block boundary, in two blocks one argmax thread reads, in the last column
     and in the two MFMA tiles of a block -- every row's argmax is the first maximal index;
  4. canary and in place: through out=, the rows around the output keep a sentinel; RESIDUAL with out = residual (the form the model
     runs) gives the bits of the out-of-place call;
  5. Gaussian inputs at one ragged shape per plan branch against the f64 chain, with test_generate_batch_gpu.py's bound;
  6. coverage: the shapes select all four <CW, NRT> with 1, 2 and >= 3 K splits, and a sweep of the plan query finds nothing else.

On the MI355X all 618 (shape, form, R, epilogue) cases are exact: v_mfma_f32_16x16x32_bf16 loses nothing on these addends (multiples of 2^-2,
or 2^-12 with the SiLU shift, below 2^22), as derived in tests/gemv_rows_exact.py.  SILU_MUL is held to the bit as well: the merge kernel's
f32 expf and divide land on the f64 chain's bf16 value at every gate these seeded cases produce, and a zero product keeps its sign (-0
where a zero gate or up sum meets a negative partner).
"""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gemv_exact as gx  # noqa: E402
import gemv_rows_exact as gr  # noqa: E402
from gemv_exact import LOGITS, RESIDUAL, SILU_MUL, SILU_SHIFT, STORE  # noqa: E402
from test_generate_batch_gpu import assert_close_ulps  # noqa: E402

pytestmark = pytest.mark.gpu

RAN = {}                         # (N, K) -> {(form, R, epi)} the exact-sums test ran
SENTINEL = 0x5A5A                # bf16 bit pattern of the canary rows
EPI_NAME = {STORE: "STORE", RESIDUAL: "RESIDUAL", SILU_MUL: "SILU_MUL", LOGITS: "LOGITS"}


def operands(c, form, silu=False):
    """(the op wrapper, its weight arguments) of a case in one weight form; silu: the weights scaled by 2^SILU_SHIFT."""
    from aha_amd import ops
    shift = SILU_SHIFT if silu else 0
    if form == "bf16":
        return ops.gemv_rows, (gx.weights(c, shift) if silu else c["W"],)
    if form == "mxfp8":
        return ops.gemv_rows_mxfp8, gx.encode_mxfp8(c, shift)
    return ops.gemv_rows_mxfp4, gx.encode_mxfp4(c, shift)


def case_of(N, K, form, dev, cache):
    """The integer case of a form: E2M1's grid for MXFP4, -8 .. 8 for the others (shared between them)."""
    fp4 = form == "mxfp4"
    if fp4 not in cache:
        cache[fp4] = gr.make_rows_case(N, K, fp4, gr.seed_of(N, K, fp4), dev)
    return cache[fp4]


# ---- 1. exact sums, 2. probes -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,K", gr.ROWS_SHAPES)
def test_gemv_rows_gives_the_exact_sums(gpu, N, K):
    from aha_amd import ops
    plan = ops.plan_gemv_rows(N, K)
    assert plan == gr.PLANS[N, K]
    cache, ran = {}, set()
    for form in gr.forms(K):
        c = case_of(N, K, form, gpu, cache)
        for epi in gr.epilogues(N, K):
            run, w = operands(c, form, epi == SILU_MUL)
            want = gr.expected_rows(c, gr.MAX_ROWS, epi)          # rows are independent: a call with R rows gives the first R
            for R in gr.ROW_COUNTS:
                got = run(*w, c["x"][:R].contiguous(), epi, c["res"][:R].contiguous() if epi == RESIDUAL else None)
                gr.assert_rows(got, tuple(t[:R] for t in want) if epi == LOGITS else want[:R], epi,
                               f"{form} {N} x {K} plan={plan} R={R} {EPI_NAME[epi]}")
                ran.add((form, R, epi))
        ks, xp = gr.probe_rows(K, gpu)
        run, w = operands(c, form)
        what = f"{form} {N} x {K} plan={plan} probes"
        probe = (lambda x: run(*w, x, LOGITS)[0]) if (N, K) in gr.LOGITS_ONLY else (lambda x: run(*w, x, STORE))
        gr.assert_probes(probe(xp), c["W"], ks, what)
        # and in the second row tile, behind sixteen rows of zeros
        got = probe(torch.cat([torch.zeros_like(xp[:1]).expand(16, K), xp]).contiguous())
        assert not bool(got[:16].any()), what + ": zero rows with nonzero outputs"
        gr.assert_probes(got[16:], c["W"], ks, what + ", second row tile")
    assert len(ran) == len(gr.forms(K)) * len(gr.epilogues(N, K)) * len(gr.ROW_COUNTS)
    RAN[N, K] = ran


# ---- 3. ties ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,K", gr.TIE_SHAPES)
def test_argmax_is_the_first_maximal_index_over_planted_ties(gpu, N, K):
    cache = {}
    for form in gr.forms(K):
        fresh = (form == "mxfp4") not in cache
        c = case_of(N, K, form, gpu, cache)
        if fresh:
            c["achieved"] = gr.plant_row_ties(c)
        # beforehand, on the inputs: every relation that exists for the shape is there
        pairs = gr.tie_pairs(N)
        assert set(pairs) <= set(c["achieved"]), (form, pairs, c["achieved"])
        assert len(pairs) == (5 if N > 65536 + 256 else 4 if N > 256 else 3)
        run, w = operands(c, form)
        want = gr.expected_rows(c, gr.MAX_ROWS, LOGITS)
        tied = sorted({r for rows in c["achieved"].values() for r in rows})
        assert len(tied) >= len(pairs) and tied[len(pairs) - 1] < 16          # a row of its own per relation, all in a one-tile call too
        for R in (16, 32):
            got = run(*w, c["x"][:R].contiguous(), LOGITS)
            gr.assert_rows(got, tuple(t[:R] for t in want), LOGITS, f"{form} {N} x {K} R={R} ties {c['achieved']}")


# ---- 4. canary and in place -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,K", [(40, 160), (8200, 672)])          # ragged N; <CW, NRT> = <1 | 2, 1 | 2> with R = 1 | 17
def test_output_rows_alone_are_written_and_in_place_residual(gpu, N, K):
    from aha_amd import ops
    assert N % 32 != 0 and ops.plan_gemv_rows(N, K)[0] == (1 if N == 40 else 2)
    cache = {}
    for form in gr.forms(K):
        c = case_of(N, K, form, gpu, cache)
        run, w = operands(c, form)
        for R in (1, 17):
            x, res = c["x"][:R].contiguous(), c["res"][:R].contiguous()
            for epi in (STORE, RESIDUAL):
                what = f"{form} {N} x {K} R={R} {EPI_NAME[epi]}"
                want = gr.expected_rows(c, R, epi)
                buf = torch.full((R + 2, N), SENTINEL, dtype=torch.int16, device=gpu).view(torch.bfloat16)
                y = buf[1:R + 1]
                assert y.is_contiguous() and y.data_ptr() == buf.data_ptr() + 2 * N
                out = run(*w, x, epi, res if epi == RESIDUAL else None, out=y)
                assert out.data_ptr() == y.data_ptr()
                gr.assert_rows(buf[1:R + 1], want, epi, what + " into a larger buffer")
                outer = gx.bits(buf)[[0, R + 1]]
                assert bool((outer == SENTINEL).all()), f"{what}: {int((outer != SENTINEL).sum())} elements outside the output rows were written"
            y = res.clone()
            run(*w, x, RESIDUAL, y, out=y)
            what = f"{form} {N} x {K} R={R} RESIDUAL, the output aliasing the residual"
            gr.assert_rows(y, run(*w, x, RESIDUAL, res), RESIDUAL, what + ", against the out-of-place call")
            gr.assert_rows(y, gr.expected_rows(c, R, RESIDUAL), RESIDUAL, what)
            assert torch.equal(res, c["res"][:R])


# ---- 5. Gaussian inputs -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,K", gr.GAUSSIAN_SHAPES)
def test_gemv_rows_on_gaussian_inputs_against_the_f64_chain(gpu, N, K):
    """The f64 chain rounded at the op boundaries, test_generate_batch_gpu.py assert_close_ulps' bound: 1 bf16 ulp for store, residual and
    the logits (2 for silu_mul, which no shape of this list runs: all are ragged in N).  frac_exact = 0: exactness is the other tests' job."""
    from aha_amd import ops
    assert N % 32 != 0
    for R in (1, 17):
        c = gr.gaussian_rows_case(N, K, R, gpu, gr.seed_of(N, K) + R)
        for epi in (STORE, RESIDUAL, LOGITS):
            got = ops.gemv_rows(c["W"], c["x"], epi, c["res"] if epi == RESIDUAL else None)
            want = gr.gaussian_rows_expected(c, epi)
            assert_close_ulps(got[0] if epi == LOGITS else got, want, 1, 0.0, f"gaussian {N} x {K} R={R} {EPI_NAME[epi]}")


# ---- 6. coverage ------------------------------------------------------------------------------------------------------------------------
def test_the_shapes_cover_every_launch_the_plan_can_reach(gpu):
    from aha_amd import ops
    every = {(cw, nrt, k) for cw in (1, 2) for nrt in (1, 2) for k in (1, 2, 3)}
    assert gr.launches(ops.plan_gemv_rows) == every
    assert gr.reachable(ops.plan_gemv_rows) == {(cw, k) for cw, _, k in every}
    # what ran: every (form, R, epilogue) of each shape, so the launches above are the launches that ran
    for (N, K), ran in RAN.items():
        assert ran == {(f, R, e) for f in gr.forms(K) for R in gr.ROW_COUNTS for e in gr.epilogues(N, K)}, (N, K)
    if set(RAN) == set(gr.ROWS_SHAPES):          # the whole file ran (a -k selection is held to the per-shape sets above)
        assert gr.launches(ops.plan_gemv_rows, list(RAN)) == every
    print(f"exact gemv_rows cases run: {sum(len(v) for v in RAN.values())} on {len(RAN)} of {len(gr.ROWS_SHAPES)} shapes")
