"""CPU tier of the exact matvec tests (tests/gemv_exact.py, tests/test_gemv_exact_gpu.py): everything those tests rest on that needs no GPU.

  * the plan query aha_hip_debug_plan_gemv and the test entry aha_hip_debug_gemv_partial_f32 in every layer of the ABI, their argument checks;
  * the generator's preconditions on every shape of the lists (every K; the rows capped at CPU_ROWS here -- the rows are independent
    draws, and make_case asserts the same on the full matrix of every GPU case), the rounding helper against torch's own conversion;
  * the weights survive the three quantisers unchanged, and the directly written MX codes decode to them through aha_amd/quant.py;
  * the query's sweep gives the reachable set, the GPU list covers it, every reachable instantiation is in the code object;
  * the comparison catches planted errors in a correct output: a dropped term, two k swapped, a tie rounded away from even, the second
    of two tied maxima.
"""
import ctypes as C
import os
import re
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gemv_exact as gx  # noqa: E402
from gemv_exact import LOGITS, PARTIAL_F32, RESIDUAL, SILU_MUL, SILU_SHIFT, STORE  # noqa: E402
from test_isa_cpu import kernels  # noqa: E402,F401  (its module-scoped fixture)
from test_weights_fp8_single_gpu import SHAPES as MX_SHAPES  # noqa: E402  (the list only: nothing there runs at import)
from test_wpack_gpu import rows_of as pk13_rows_of  # noqa: E402

CPU_ROWS = 1056


# ---- 1. the ABI -------------------------------------------------------------------------------------------------------------------------
def test_plan_query_and_partial_entry_in_every_layer(hip_lib):
    from aha_amd import _lib, ops
    import test_host_cpu
    header = open(os.path.join(ROOT, "include", "aha_hip.h")).read()
    assert re.search(r"int aha_hip_debug_plan_gemv\(int32_t N, int32_t K, int32_t epi, int32_t has_norm, int32_t\* R, int32_t\* U, "
                     r"int32_t\* grid, int32_t\* form\);", header)
    assert re.search(r"int aha_hip_debug_gemv_partial_f32\(const void\* W, const void\* x, float\* y_f32, int32_t N, int32_t K, "
                     r"const void\* norm_w, float eps,\s+void\* stream\);", header)
    raw = C.CDLL(_lib.LIB_PATH)
    for name, nargs in (("aha_hip_debug_plan_gemv", 8), ("aha_hip_debug_gemv_partial_f32", 8)):
        assert hasattr(raw, name) and len(_lib.SIGNATURES[name][1]) == nargs, name
    # the twin of the FP8 query, without by_plan
    assert _lib.SIGNATURES["aha_hip_debug_plan_gemv"][1] == _lib.SIGNATURES["aha_hip_debug_plan_gemv_mxfp8"][1][:8]
    assert set(_lib.SIGNATURES) == set(test_host_cpu._declared_symbols())
    assert callable(ops.plan_gemv) and callable(ops.gemv_partial_f32)
    src = open(os.path.join(ROOT, "rust", "aha-hip", "src", "lib.rs")).read()
    ext = src[src.index('extern "C" {'):]
    ext = ext[:ext.index("\n    }\n")]
    assert re.search(r"pub fn aha_hip_debug_plan_gemv\(\s+n: i32,", ext) and re.search(r"pub fn aha_hip_debug_gemv_partial_f32\(", ext)
    # launch and query share one function for the forms (and the query is host code: the device code is the parent's)
    text = open(os.path.join(ROOT, "aha_amd", "csrc", "kernels_gemv.hip")).read()
    assert len(re.findall(r"\bform_of\(p, ", text)) == 2 and text.count("AHA_GEMV_FAST") == 1


def test_argument_checks_need_no_gpu(hip_lib):
    err = hip_lib.aha_hip_last_error
    buf = (C.c_uint8 * 4096)()
    p = C.addressof(buf)
    r = C.c_int32()
    f = C.c_float(0)
    for bad in ((0, 64, 0), (64, 0, 0), (64, 36, 0), (64, 32776, 0), (64, 64, 5), (64, 64, -1), (63, 64, 2)):
        assert hip_lib.aha_hip_debug_plan_gemv(bad[0], bad[1], bad[2], 0, C.byref(r), C.byref(r), C.byref(r), None) == -1, bad
        assert b"debug_plan_gemv" in err()
    assert hip_lib.aha_hip_debug_plan_gemv(64, 64, 0, 0, None, C.byref(r), C.byref(r), None) == -1
    assert hip_lib.aha_hip_debug_plan_gemv(80, 160, 2, 0, C.byref(r), C.byref(r), C.byref(r), None) == 0       # gate+up of 40 rows: no 32-row blocks
    for args in ((None, p, p, 32, 64), (p, None, p, 32, 64), (p, p, None, 32, 64), (p, p, p, 0, 64), (p, p, p, 32, 36), (p, p, p, 32, 32776)):
        assert hip_lib.aha_hip_debug_gemv_partial_f32(*args, None, f, None) == -1 and b"debug_gemv_partial_f32" in err(), args


def test_plan_of_the_decode_shapes_and_the_thresholds(hip_lib):
    from aha_amd import ops
    # Qwen3-8B's step: qkv, o_proj, gate+up, down, lm_head
    assert ops.plan_gemv(6144, 4096, STORE, True) == (1, 8, 768, 3)
    assert ops.plan_gemv(4096, 4096, RESIDUAL, False) == (1, 8, 512, 2)             # whole rounds: 1024 tiles on 512 blocks
    assert ops.plan_gemv(24576, 4096, SILU_MUL, True) == (2, 4, 768, 3)
    assert ops.plan_gemv(4096, 12288, RESIDUAL, False) == (1, 8, 512, 2)
    assert ops.plan_gemv(151936, 4096, LOGITS, True) == (4, 4, 768, 3)
    assert ops.plan_gemv(4096, 12288, PARTIAL_F32, False) == ops.plan_gemv(4096, 12288, STORE, False)
    # rows per wave: 1024 tiles or more
    assert [ops.plan_gemv(n, 512, STORE)[0] for n in (8184, 8185, 16368, 16369)] == [1, 2, 2, 4]
    assert [ops.plan_gemv(2 * n, 512, SILU_MUL)[0] for n in (8184, 8185, 16368, 16369)] == [1, 2, 2, 2]
    # the forms: FAST = K a multiple of 512 * U; straight-line up to 8192 with norm weights, 16384 without
    assert [ops.plan_gemv(64, k, STORE, nm)[3] for k, nm in ((4104, False), (20480, False), (16384, False), (12288, True), (8192, True))] == [0, 1, 2, 1, 3]
    for n, k, e, nm in ((40, 160, 0, False), (100000, 64, 3, True), (16416, 18432, 1, False), (32832, 4096, 2, True)):
        r, u, grid, form = ops.plan_gemv(n, k, e, nm)
        rows = n // 2 if e == SILU_MUL else n
        assert 1 <= grid <= min(768, -(-rows // (4 * r))) and (form != 0) == (k % (512 * u) == 0), (n, k, e, nm)


# ---- 2. the generator -------------------------------------------------------------------------------------------------------------------
def test_rounding_helper_is_round_to_nearest_even():
    g = torch.Generator().manual_seed(1)
    v = (torch.randn(200000, generator=g) * torch.exp2(torch.randint(-20, 21, (200000,), generator=g).float())).double()
    assert torch.equal(gx.bf16_rne(v), v.float().to(torch.bfloat16).double())          # f32 values: torch's conversion rounds once
    # ties: 1 + (2 n + 1) * 2^-8 lies half way between two bf16 values; the even one has an even 7-bit mantissa
    n = torch.arange(0, 127, dtype=torch.float64)
    tie = 1.0 + (2 * n + 1) * 2.0 ** -8
    want = 1.0 + 2 * torch.floor((n + 1) / 2) * 2.0 ** -7
    assert torch.equal(gx.bf16_rne(tie), want) and torch.equal(gx.bf16_rne(-tie), -want)
    assert torch.equal(gx.bf16_rne(torch.tensor([0.0, 255.5, 256.5, 257.0, 2.0 ** 22 - 0.25], dtype=torch.float64)),
                       torch.tensor([0.0, 256.0, 256.0, 256.0, 2.0 ** 22], dtype=torch.float64))
    assert gx.bits(gx.as_bf16(gx.bf16_rne(torch.tensor([-0.0, 0.0], dtype=torch.float64)))).tolist() == [0, 0]      # a zero sum is +0


def capped(rows):
    return min(rows, CPU_ROWS)


def test_preconditions_hold_for_every_shape_of_the_lists():
    assert len(set(gx.BF16_SHAPES)) == len(gx.BF16_SHAPES) and max(r * k for r, k in gx.BF16_SHAPES) == 16416 * 18432
    worst, ties, n = 0.0, 0.0, 0
    shapes = [(r, k, False) for r, k in gx.BF16_SHAPES] + [(r, k, f) for r, k in MX_SHAPES for f in (False, True)]
    shapes += [(2 * r if e == SILU_MUL else r, k, False) for e in (STORE, RESIDUAL, SILU_MUL, LOGITS) for k in (4096, 12288) for r in pk13_rows_of(e)]
    shapes.append((64, 32768, False))          # the largest K the entries take: the expected |sum| is about 1.1e6
    for i, (rows, K, fp4) in enumerate(shapes):
        c = gx.make_case(capped(rows), K, fp4=fp4, seed=i)          # asserts them
        worst = max(worst, float(gx.row_sums(c["W"], gx.activations(c))[1].max()))
        assert len(torch.unique(c["j"])) == 5 and c["W"].dtype == torch.bfloat16 and c["W"].shape == (capped(rows), K)
        if capped(rows) >= 1000:
            ties, n = ties + gx.tie_fraction(c), n + 1
    assert worst < gx.EXACT_BOUND / 2          # a factor of two to spare at K = 32768
    print(f"largest sum |x W| {worst:.0f}; rows on a bf16 tie {ties / n:.4f}")
    assert ties / n > 0.02                     # bf16's rounding itself is exercised: rows on a tie, about 6 %


def test_planted_ties_land_where_the_plan_says():
    # R = 2, grid = 3: tile = 8 rows; row 9 = tile 1, wave 0, first row of its wave
    # R = 2, grid = 3: a tile is 8 rows; row 8 = tile 1, wave 0, the first row of its wave; row 9 the last
    assert gx.tie_targets(8, 100, 2, 3) == {"same wave": 9, "other wave": 10, "same block": 32, "other block": 16, "last row": 99}
    assert gx.tie_targets(9, 100, 2, 3) == {"other wave": 11, "same block": 33, "other block": 17, "last row": 99}
    assert gx.tie_targets(15, 16, 2, 3) == {"other wave": 9, "other block": 7}          # wave 3 of the last tile, and the last row itself
    assert gx.tie_targets(5, 40, 1, 10) == {"other wave": 6, "other block": 9, "last row": 39}
    for rows, K, R, grid in ((100, 64, 2, 3), (40, 160, 1, 10), (4100, 64, 4, 8)):
        c = gx.make_case(rows, K, seed=3, tie_plan=(R, grid))
        for norm, t in zip((False, True), c["ties"]):
            lg, am = gx.expected(c, LOGITS, norm)
            held = [v for k, v in t.items()]
            assert len(held) >= 3 and all(float(lg[v]) == float(lg.max()) for v in held) and am == min(held)
            assert am == int(torch.argmax(lg)) or float(lg[am]) == float(lg.max())
        # both rounds kept their rows, and W still is ints * 2^j
        assert torch.equal(c["W"], gx.weights(c))


# ---- 3. the weights in every form -------------------------------------------------------------------------------------------------------
def test_weights_survive_the_three_quantisers_and_the_direct_codes_decode_to_them():
    from aha_amd import quant
    for rows, K in ((64, 4096), (40, 160), (33, 1056)):
        c = gx.make_case(rows, K, seed=5)
        for shift in (0, SILU_SHIFT):
            W = gx.weights(c, shift)
            q, s, wr = quant.quantize_mxfp8(W)
            assert torch.equal(gx.bits(wr), gx.bits(W))
            qd, sd = gx.encode_mxfp8(c, shift)
            assert torch.equal(gx.bits(quant.dequantize_mxfp8(qd, sd)), gx.bits(W)) and sd.dtype == qd.dtype == torch.uint8
            assert set(torch.unique(sd).tolist()) == {127 + j + shift for j in gx.BLOCK_SHIFTS}
        c4 = gx.make_case(rows, K, fp4=True, seed=6)
        assert set(torch.unique(c4["ints"]).tolist()) == set(gx.FP4_VALUES)
        for shift in (0, SILU_SHIFT):
            W = gx.weights(c4, shift)
            q, s, wr = quant.quantize_mxfp4(W)
            assert torch.equal(wr, W)          # the values; a block's zeros may come back as -0 only if W held -0, and it holds none
            qd, sd = gx.encode_mxfp4(c4, shift)
            assert qd.shape == (rows, K // 2) and torch.equal(quant.dequantize_mxfp4(qd, sd), W)
            assert not bool(((qd & 0xf) == 8).any() | ((qd >> 4) == 8).any())
    # blocks whose maximum is 1, 2 or 3 (E2M1 has no 5, and 3 = 1.5 * 2: the block exponent moves)
    for top in (1, 2, 3):
        W = (torch.tensor([0, 1, -1, top, -top] * 7)[:32].float() * torch.exp2(torch.arange(-2, 3).float())[:, None]).bfloat16()
        assert torch.equal(quant.quantize_mxfp4(W)[2], W), top
    # the integers' E4M3 codes, against torch's conversion
    v = torch.arange(0, 9).float()
    assert v.to(torch.float8_e4m3fn).view(torch.uint8).tolist() == list(gx.E4M3_OF_INT)
    assert (-v[1:]).to(torch.float8_e4m3fn).view(torch.uint8).tolist() == [0x80 | b for b in gx.E4M3_OF_INT[1:]]
    assert [quant.E2M1_GRID[i] for i in gx.E2M1_OF_INT if i >= 0] == [0.0, 1.0, 2.0, 3.0, 4.0, 6.0]
    # the 13-bit copies
    for K, shift in ((4096, 0), (12288, 0), (4096, SILU_SHIFT)):
        c = gx.make_case(48, K, seed=7)
        W = gx.weights(c, shift)
        bh, bad = quant.check_pk13(W)
        assert bad == 0
        assert torch.equal(gx.bits(quant.unpack_pk13(quant.pack_pk13(W, bh), bh)), gx.bits(W))


# ---- 4. the reachable set ---------------------------------------------------------------------------------------------------------------
def test_sweep_gives_the_reachable_set_and_the_list_covers_it(hip_lib):
    from aha_amd import ops
    want = gx.bf16_reachable(ops.plan_gemv)
    assert len(want) == 131
    # the same structure as the FP8 kernel's set: U at the plan's cap in four forms, below it never FAST without the straight-line prologue
    from test_weights_fp8_single_cpu import shipped
    assert want == shipped()
    hit = gx.bf16_covered(ops.plan_gemv)
    assert hit == want, (sorted(want - hit), sorted(hit - want))
    gx.assert_multi_tile_fast(ops.plan_gemv)


def test_every_reachable_instantiation_is_in_the_code_object(hip_lib, kernels):  # noqa: F811
    from aha_amd import ops
    want = gx.bf16_reachable(ops.plan_gemv) | gx.bf16_reachable(ops.plan_gemv, (PARTIAL_F32,))
    got = set()
    for n in kernels:
        if "gemv_kernelI" not in n:          # not gemv_kernel_pk13, gemv_mxfp8_kernel, ...
            continue
        m = re.search(r"gemv_kernelILi(\d+)ELi(\d+)ELi(\d+)ELb(\d)ELb(\d)ELi(\d)EE", n)
        assert m, n
        r, u, e, fast, trace, pro = (int(x) for x in m.groups())
        if not trace:
            got.add((r, u, e, fast, pro))
    assert want <= got, sorted(want - got)
    assert len(want) == 131 + 36


# ---- 5. the comparison catches what it is for -------------------------------------------------------------------------------------------
def test_comparison_detects_planted_errors():
    c = gx.make_case(4100, 1032, seed=11, tie_plan=(2, 768))
    W, x = c["W"].double(), c["x"].double()
    good = c["sums"][:, 0].clone()

    def outputs(s):
        lin = gx.bf16_rne(s)
        return gx.as_bf16(lin), gx.as_bf16(gx.bf16_rne(c["res"].double() + lin)), gx.as_f32(lin), gx.as_f32(s)

    want = (gx.expected(c, STORE, False), gx.expected(c, RESIDUAL, False), gx.expected(c, LOGITS, False)[0], gx.expected(c, PARTIAL_F32, False))
    for got, w in zip(outputs(good), want):
        gx.assert_same_bits(got, w)
    # one term dropped from one row: the f32 sums show any, the bf16 outputs every one that moves its row's rounded value
    term = W * x[None, :]
    k = int(torch.argmax(x.abs()))
    row = int(torch.nonzero(term[:, k] != 0).flatten()[0])
    s = good.clone()
    s[row] -= term[row, k]
    with pytest.raises(AssertionError, match=f"row {row}:"):
        gx.assert_same_bits(outputs(s)[3], want[3], "dropped term")
    moved = torch.nonzero(gx.bf16_rne(good - term[:, k]) != gx.bf16_rne(good)).flatten()
    assert moved.numel() > 0
    s = good.clone()
    s[moved[0]] -= term[moved[0], k]
    for i in (0, 1, 2):
        with pytest.raises(AssertionError, match=f"row {int(moved[0])}:"):
            gx.assert_same_bits(outputs(s)[i], want[i], "dropped term")
    # two k swapped in one row
    k1, k2 = next((a, b) for a in range(1032) for b in range(a + 1, 1032) if float(W[row, a] * x[b] + W[row, b] * x[a]) != float(term[row, a] + term[row, b]))
    s = good.clone()
    s[row] += W[row, k1] * x[k2] + W[row, k2] * x[k1] - term[row, k1] - term[row, k2]
    with pytest.raises(AssertionError, match=f"row {row}:"):
        gx.assert_same_bits(outputs(s)[3], want[3], "swapped k")
    # a bf16 tie rounded away from even
    a = good.abs().contiguous().view(torch.int64)
    tied = torch.nonzero((a & ((1 << 45) - 1)) == (1 << 44)).flatten()
    assert tied.numel() > 100
    t = int(tied[0])
    lin = gx.bf16_rne(good)
    other = 2 * good[t] - lin[t]          # the bf16 neighbour on the other side of the tie
    assert float(gx.bf16_rne(other.reshape(1))) == float(other) and abs(float(other - good[t])) == abs(float(lin[t] - good[t]))
    wrong = gx.as_bf16(lin).clone()
    wrong[t] = other
    with pytest.raises(AssertionError, match=f"row {t}:"):
        gx.assert_same_bits(wrong, want[0], "tie away from even")
    # the second of two tied maxima
    lg, am = gx.expected(c, LOGITS, False)
    later = sorted(v for v in c["ties"][0].values())
    assert am == later[0] and len(later) >= 4
    gx.assert_logits((lg, am), (lg, am))
    for v in later[1:]:
        with pytest.raises(AssertionError, match="first maximal index"):
            gx.assert_logits((lg, v), (lg, am), "later tie")
