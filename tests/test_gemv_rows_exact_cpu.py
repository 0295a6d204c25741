"""CPU tier of the exact batched-matvec tests (tests/gemv_rows_exact.py, tests/test_gemv_rows_exact_gpu.py): everything those tests rest on
that needs no GPU.

  * the plan query aha_hip_debug_plan_gemv_rows in every layer of the ABI, its argument checks, gemv_rows_plan's documented facts, the
    plan of every shape of the list and the cover of every launch the plan can reach;
  * the generator's preconditions on every shape and both integer tables, in full;
  * the directly written MX codes of every MX case decode, through aha_amd/quant.py, to exactly the bf16 W;
  * the probes and the planted ties are what they claim;
  * the comparison catches planted defects in a correct output.
"""
import ctypes as C
import functools
import os
import re
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gemv_exact as gx  # noqa: E402
import gemv_rows_exact as gr  # noqa: E402
from gemv_exact import LOGITS, RESIDUAL, SILU_MUL, SILU_SHIFT, STORE  # noqa: E402


@functools.lru_cache(maxsize=None)
def case(N, K, fp4):
    return gr.make_rows_case(N, K, fp4, gr.seed_of(N, K, fp4))          # asserts the preconditions


# ---- 1. the ABI and the plan ------------------------------------------------------------------------------------------------------------
def test_plan_query_in_every_layer(hip_lib):
    from aha_amd import _lib, ops
    import test_host_cpu
    header = open(os.path.join(ROOT, "include", "aha_hip.h")).read()
    assert re.search(r"int aha_hip_debug_plan_gemv_rows\(int32_t N, int32_t K, int32_t\* cw, int32_t\* nks\);", header)
    assert header.index("int aha_hip_debug_plan_gemv(") < header.index("int aha_hip_debug_plan_gemv_rows(") < header.index("int aha_hip_debug_gemv_partial_f32(")
    assert hasattr(C.CDLL(_lib.LIB_PATH), "aha_hip_debug_plan_gemv_rows")
    assert _lib.SIGNATURES["aha_hip_debug_plan_gemv_rows"] == (C.c_int, [C.c_int32, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int32)])
    names = list(_lib.SIGNATURES)
    assert names.index("aha_hip_debug_plan_gemv_rows") == names.index("aha_hip_debug_plan_gemv") + 1
    assert set(_lib.SIGNATURES) == set(test_host_cpu._declared_symbols())
    assert callable(ops.plan_gemv_rows)
    src = open(os.path.join(ROOT, "rust", "aha-hip", "src", "lib.rs")).read()
    ext = src[src.index('extern "C" {'):]
    ext = ext[:ext.index("\n    }\n")]
    assert re.search(r"pub fn aha_hip_debug_plan_gemv_rows\(n: i32, k: i32, cw: \*mut i32, nks: \*mut i32\) -> i32;", ext)
    # launch and query call one function
    text = open(os.path.join(ROOT, "aha_amd", "csrc", "capi.hip")).read()
    body = text[text.index("int aha_hip_debug_plan_gemv_rows("):]
    assert "gemv_rows_plan(N, K, &c, &s);" in body[:body.index("\n}\n")]
    assert "gemv_rows_plan(a.N, a.K, &cw, &nks);" in open(os.path.join(ROOT, "aha_amd", "csrc", "gemv_rows_body.h")).read()
    # out= on the three wrappers
    import inspect
    for f in (ops.gemv_rows, ops.gemv_rows_mxfp8, ops.gemv_rows_mxfp4):
        assert inspect.signature(f).parameters["out"].default is None, f.__name__


def test_plan_query_argument_checks_need_no_gpu(hip_lib):
    err = hip_lib.aha_hip_last_error
    a, b = C.c_int32(-7), C.c_int32(-7)
    for N, K in ((0, 64), (-1, 64), (64, 0), (64, 4), (64, 36), (64, -8)):
        assert hip_lib.aha_hip_debug_plan_gemv_rows(N, K, C.byref(a), C.byref(b)) == -1, (N, K)
        assert b"debug_plan_gemv_rows" in err() and (a.value, b.value) == (-7, -7)
    assert hip_lib.aha_hip_debug_plan_gemv_rows(64, 64, None, C.byref(b)) == -1 and b"debug_plan_gemv_rows" in err()
    assert hip_lib.aha_hip_debug_plan_gemv_rows(64, 64, C.byref(a), None) == -1 and b"debug_plan_gemv_rows" in err()
    assert hip_lib.aha_hip_debug_plan_gemv_rows(1, 8, C.byref(a), C.byref(b)) == 0 and (a.value, b.value) == (1, 1)


def test_plan_facts_and_the_plan_of_every_shape(hip_lib):
    from aha_amd import ops
    plan = ops.plan_gemv_rows
    # gemv_rows_plan: at most four chunks -> one chunk per wave, one split, whatever N
    assert {plan(N, K) for N in (1, 40, 8192, 151936) for K in range(8, 512 + 8, 8)} == {(1, 1)}
    assert plan(96, 1024) == (1, 2)            # two chunks per wave would leave CUs idle: 3 blocks x 1 split
    assert plan(8192, 1024) == (2, 1)          # 256 blocks
    assert plan(4096, 2048) == (2, 2)          # 128 blocks x 2 splits
    assert plan(8160, 1024) == (1, 2) and plan(8161, 1024) == (2, 1)          # the threshold: blocks x splits >= 256
    assert plan(151936, 4096) == (2, 4) and plan(4096, 12288) == (2, 12) and plan(1024, 3072) == (1, 6)          # lm_head, down_proj
    assert len(set(gr.ROWS_SHAPES)) == len(gr.ROWS_SHAPES) == 13 and set(gr.PLANS) == set(gr.ROWS_SHAPES)
    assert {s: plan(*s) for s in gr.ROWS_SHAPES} == gr.PLANS
    # nks = ceil(chunks / 4 cw), and what each shape is there for
    for (N, K), (cw, nks) in gr.PLANS.items():
        assert nks == -(-(-(-K // 128)) // (4 * cw))
    assert 1032 - 2 * 512 == 8 and 4128 - 8 * 512 == 32          # fallback: the last split one partial chunk
    assert 672 - 5 * 128 == 32 and -(-672 // 128) == 6           # CW = 2: wave 2's second chunk partial, wave 3 past the end
    assert 2080 - 2 * 1024 == 32                                 # CW = 2: the third split holds 32 k
    assert -(-65800 // 256) == 258 and 65800 % 256 == 8          # more than 256 merge tiles, the last ragged


def test_the_shapes_cover_every_launch_the_plan_can_reach(hip_lib):
    from aha_amd import ops
    every = {(cw, nrt, k) for cw in (1, 2) for nrt in (1, 2) for k in (1, 2, 3)}
    assert gr.launches(ops.plan_gemv_rows) == every
    assert gr.reachable(ops.plan_gemv_rows) == {(cw, k) for cw, _, k in every}
    assert {K % 32 for N, K in gr.ROWS_SHAPES} == {0, 8} and {N % 32 for N, K in gr.ROWS_SHAPES} == {0, 8}
    for shapes in (gr.TIE_SHAPES[:2], gr.GAUSSIAN_SHAPES):
        assert set(shapes) <= set(gr.ROWS_SHAPES)
    assert {ops.plan_gemv_rows(*s)[0] for s in gr.GAUSSIAN_SHAPES} == {1, 2} and all(N % 32 for N, _ in gr.GAUSSIAN_SHAPES)
    assert {gr.nks_class(ops.plan_gemv_rows(*s)[1]) for s in gr.GAUSSIAN_SHAPES} == {1, 3}


# ---- 2. the generator, 3. the encodings -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,K", gr.ROWS_SHAPES + gr.TIE_SHAPES[2:])
def test_preconditions_hold_and_the_mx_codes_decode_to_w(N, K):
    from aha_amd import quant
    for fp4 in (False, True):
        c = case(N, K, fp4)          # asserts them, on the full matrix and all 32 activation rows
        assert c["W"].shape == (N, K) and c["W"].dtype == c["x"].dtype == c["res"].dtype == torch.bfloat16
        assert c["sums"].shape == (gr.MAX_ROWS, N) and c["sums"].dtype == torch.float64
        assert bool((c["x"] != 0).all())
        assert torch.equal(c["W"], gx.make_inputs(N, K, fp4, "cpu", gr.seed_of(N, K, fp4))["W"])          # gemv_exact's weights, unchanged
        if N * K >= 4096:
            assert len(torch.unique(c["j"])) == 5
        # the sums, again, by another route: int64 arithmetic on ints * 2^(j + 2)
        n = min(N, 64)
        w4 = c["ints"][:n].long() * torch.exp2((c["j"][:n].float() + 2)).long().repeat_interleave(32, dim=1)[:, :K]
        assert torch.equal((c["x"].long() @ w4.T).double() / 4, c["sums"][:, :n])
        if K % 32:
            continue
        for shift in (0, SILU_SHIFT) if N % 32 == 0 else (0,):
            W = gx.weights(c, shift)
            q, s = gx.encode_mxfp8(c, shift)
            assert q.shape == (N, K) and s.shape == (N, K // 32)
            assert torch.equal(gx.bits(quant.dequantize_mxfp8(q, s)), gx.bits(W))
            if fp4:
                q, s = gx.encode_mxfp4(c, shift)
                assert q.shape == (N, K // 2) and s.shape == (N, K // 32)
                assert torch.equal(gx.bits(quant.dequantize_mxfp4(q, s)), gx.bits(W))


def test_every_sum_stays_far_inside_the_exact_range():
    worst = max(float(gr.sums_of(case(N, K, fp4))[1].max()) for N, K in gr.ROWS_SHAPES for fp4 in (False, True))
    print(f"largest sum |x W| {worst:.0f} of {gx.EXACT_BOUND:.0f}")
    assert worst < gx.EXACT_BOUND / 2          # K = 12288: 12288 * 8 * 32 is the hard limit, 3/4 of 2^22; the draws stay below half


def test_silu_mul_keeps_the_sign_of_a_zero_product():
    """A gate or an up sum of exactly 0 next to a negative partner: -0 in the reference's bf16 multiply (and in the merge kernel's f32
    one).  The exact comparison is on bits, so the expectation holds -0 there, and +0 in its place is a difference."""
    c = case(4096, 2048, False)
    want = gr.expected_rows(c, gr.MAX_ROWS, SILU_MUL)
    neg0 = torch.nonzero(gx.bits(want) == -32768).tolist()
    assert neg0 and not bool((gx.bits(gr.expected_rows(c, gr.MAX_ROWS, STORE)) == -32768).any())
    gi, ui = gx.gate_up_rows(4096)
    for r, n in neg0:
        g, u = float(c["sums"][r, gi[n]]), float(c["sums"][r, ui[n]])
        assert (g == 0 and u < 0) or (u == 0 and g < 0), (r, n, g, u)          # silu(+0) = +0 times a negative up, or the reverse
    flat = want.clone()
    flat[neg0[0][0], neg0[0][1]] = 0.0
    with pytest.raises(AssertionError, match="1 of .* outputs differ.*got 0.0, want -0.0"):
        gr.assert_rows(flat, want, SILU_MUL)


# ---- 4. probes and ties -----------------------------------------------------------------------------------------------------------------
def test_probes_are_unit_vectors_at_the_boundaries():
    assert gr.probe_ks(8) == [0, 7] and gr.probe_ks(32) == [0, 7, 8, 23, 24, 31]
    assert gr.probe_ks(160) == [0, 7, 8, 31, 32, 127, 128, 151, 152, 159]
    assert gr.probe_ks(12288) == [0, 7, 8, 31, 32, 127, 128, 511, 512, 12255, 12256, 12279, 12280, 12287]
    for _, K in gr.ROWS_SHAPES:
        ks, x = gr.probe_rows(K)
        assert 2 <= len(ks) <= 14 and x.shape == (len(ks), K) and x.dtype == torch.bfloat16
        assert torch.equal(x.float().sum(1), torch.ones(len(ks))) and x.float().argmax(1).tolist() == ks
    # on a correct output the probes pass, and a k read from its neighbour's place is named
    c = case(40, 264, False)
    ks, x = gr.probe_rows(264)
    good = (x.double() @ c["W"].double().T)
    gr.assert_probes(gx.as_bf16(gx.bf16_rne(good)), c["W"], ks)
    moved = c["W"].double().clone()
    moved[:, 256:264] = moved[:, 248:256]          # the ragged last fragment re-read at K - 16
    with pytest.raises(AssertionError, match=r"k = \[256, 263\]"):
        gr.assert_probes(gx.as_bf16(gx.bf16_rne(x.double() @ moved.T)), c["W"], ks)


@pytest.mark.parametrize("N,K", gr.TIE_SHAPES)
def test_planted_ties_are_in_the_inputs(N, K):
    pairs = gr.tie_pairs(N)
    assert list(pairs) == [n for n in gr.RELATIONS if n != "same argmax thread" or N == 65800]          # 258 tiles: only there
    assert len({col for pq in pairs.values() for col in pq}) == 2 * len(pairs)
    if N == 65800:
        p, q = pairs["same argmax thread"]
        assert (p // 256, q // 256) == (1, 257) and q // 256 == -(-N // 256) - 1          # the ragged last tile
    for fp4 in (False, True):
        c = gr.make_rows_case(N, K, fp4, gr.seed_of(N, K, fp4))
        before = gr.relations_achieved(c)
        achieved = gr.plant_row_ties(c)
        assert set(pairs) <= set(achieved) and not set(pairs) <= set(before)
        lg, am = gr.expected_rows(c, gr.MAX_ROWS, LOGITS)
        cols = gr.max_columns(c)
        for name, (p, q) in pairs.items():
            rows = [r for r in achieved[name] if p in cols[r] and q in cols[r]]
            assert rows, name
            for r in rows:
                assert float(lg[r, p]) == float(lg[r, q]) == float(lg[r].max()) and int(am[r]) == cols[r][0] <= p
        assert all(int(am[r]) == cols[r][0] for r in range(gr.MAX_ROWS))


# ---- 5. the comparison catches what it is for -------------------------------------------------------------------------------------------
def test_comparison_detects_planted_defects():
    N, K = 296, 160
    c = gr.make_rows_case(N, K, False, gr.seed_of(N, K))
    achieved = gr.plant_row_ties(c)
    W, x, good = c["W"].double(), c["x"].double(), c["sums"]
    want = {e: gr.expected_rows(c, gr.MAX_ROWS, e) for e in (STORE, RESIDUAL, LOGITS)}

    def outputs(s):
        return {e: gr.epilogue(s, c["res"], e) for e in (STORE, RESIDUAL, LOGITS)}

    def caught(s, what, epis=(STORE, RESIDUAL, LOGITS)):
        for e in epis:
            with pytest.raises(AssertionError, match="outputs differ"):
                gr.assert_rows(gr.epilogue(s, c["res"], e), want[e], e, what)

    for e, got in outputs(good).items():
        gr.assert_rows(got, want[e], e)
    for k in range(K):          # any single k dropped, from every row (every epilogue at the probed k)
        caught(good - x[:, k:k + 1] * W[:, k][None, :], f"k = {k} dropped", (STORE, RESIDUAL, LOGITS) if k in gr.probe_ks(K) else (STORE,))
    tail = x[:, K - 8:] @ W[:, K - 8:].T
    caught(good - tail, "the last 8 k dropped")
    caught(good + tail, "the last 8 k added twice")
    caught(good[list(range(16, 32)) + list(range(16))], "rows r and r + 16 swapped")
    s = good.clone()
    s[:, N - 1] = s[:, N - 2]
    caught(s, "column N - 1 replaced by column N - 2")
    # a half-way sum rounded away from even
    a = good.abs().contiguous().view(torch.int64)
    tied = torch.nonzero((a & ((1 << 45) - 1)) == (1 << 44))
    assert tied.shape[0] > 100, "no sum of this case lies half way between two bf16 values"
    r, n = (int(v) for v in tied[0])
    lin = gx.bf16_rne(good)
    other = 2 * good[r, n] - lin[r, n]          # the bf16 neighbour on the other side of the tie
    assert float(gx.bf16_rne(other.reshape(1))) == float(other) and abs(float(other - good[r, n])) == abs(float(lin[r, n] - good[r, n]))
    wrong = want[STORE].clone()
    wrong[r, n] = other
    with pytest.raises(AssertionError, match=f"1 of {gr.MAX_ROWS * N} outputs differ; first at row {r}, column {n}:"):
        gr.assert_rows(wrong, want[STORE], STORE, "tie away from even")
    # an argmax that returns the second of two tied columns
    lg, am = want[LOGITS]
    cols = gr.max_columns(c)
    for name, rows in achieved.items():
        r = rows[0]
        assert len(cols[r]) >= 2 and int(am[r]) == cols[r][0]
        later = am.clone()
        later[r] = cols[r][1]
        with pytest.raises(AssertionError, match=f"argmax of row {r} is {cols[r][1]}, the first maximal index is {cols[r][0]}"):
            gr.assert_rows((lg, later), (lg, am), LOGITS, name)
