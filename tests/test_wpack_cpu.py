"""CPU tier: exact 13-bit weight copies (aha_amd/quant.py pack_pk13 / check_pk13 / unpack_pk13, aha_amd/csrc/kernels_gemv_pk13.hip).

  * pack -> unpack is the identity, on random weights with +-0, bf16 subnormals and E = 1 among them and on both edges of the window;
  * the check counts Inf, NaN and the values below the window, and chooses the base from the matrix maximum;
  * the layout: where a weight's low byte, code and sign land in its unit;
  * one lane's decoding restated in numpy gives the bits lo_bf / hi_bf give on W;
  * the plan, gemv_pk13_by_plan, the entries' GPU-free argument checks;
  * the instantiations the launcher can reach, pinned against the shipped gfx950 code object.
"""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_isa_cpu as isa  # noqa: E402
from test_isa_cpu import kernels  # noqa: E402,F401  (its module-scoped fixture)
from test_decode_preload_cpu import kernels as preload_kernels  # noqa: E402,F401

from aha_amd import quant  # noqa: E402

STORE, RESIDUAL, SILU_MUL, LOGITS = 0, 1, 2, 3


def shipped():
    """{(R, EPI, PRO)}: one row per wave for the layer epilogues, two for the logits; every prologue form."""
    return {(2 if e == LOGITS else 1, e, pro) for e in (STORE, RESIDUAL, SILU_MUL, LOGITS) for pro in (0, 1, 2)}


def from_bits(bits):
    return torch.from_numpy(np.asarray(bits, dtype=np.uint16).astype(np.int16)).view(torch.bfloat16)


def bits_of(W):
    return W.contiguous().view(torch.int16).numpy().astype(np.uint16)


def edge_weights(N=6, K=8192, seed=0):
    """normal(0, 0.02) weights with +-0, bf16 subnormals, E = 1 (codes of h = 0) planted in every row."""
    g = torch.Generator().manual_seed(seed)
    W = (torch.randn(N, K, generator=g) * 0.02).bfloat16()
    b = bits_of(W).copy()
    b[:, 3] = 0x8000          # -0
    b[:, 5] = 0x0000          # +0
    b[:, 64] = 0x0001         # smallest subnormal
    b[:, 65] = 0x807f         # largest subnormal, negative
    b[:, 700] = 0x0080        # E = 1, m = 0
    b[:, 4095] = 0x80ff       # E = 1, m = 127, negative
    b[:, K - 1] = 0x00c5      # E = 1 at the end of the last unit
    return from_bits(b)


# ---- 1. the identity ------------------------------------------------------------------------------------------------------------------
def test_pack_then_unpack_is_the_identity():
    W = edge_weights()
    bh, bad = quant.check_pk13(W)
    assert bad == 0 and bh == int(((bits_of(W) >> 8) & 0x7f).max()) - 15
    P = quant.pack_pk13(W, bh)
    assert P.shape == (6, 2, 6656) and P.dtype == torch.uint8
    assert P.numel() * 8 == W.numel() * 13           # 13 bits per weight
    assert np.array_equal(bits_of(quant.unpack_pk13(P, bh)), bits_of(W))


def test_both_edges_of_the_window_round_trip_and_one_binade_further_does_not():
    for top in (127, 126, 60, 16, 15, 9):        # E >> 1 of the matrix maximum; below 16 the base is 0 and the window ends at E = 2
        bh = max(top - 15, 0)
        hi = [(top << 8) | lo for lo in ((0x00, 0x7f, 0x01, 0x7e) if top == 127 else (0x00, 0x7f, 0x80, 0xff))]      # both E of the top code (E = 255 is Inf / NaN)
        lo_edge = [((bh + 1) << 8) | lo for lo in (0x00, 0xff)]
        vals = hi + lo_edge + [v | 0x8000 for v in hi + lo_edge] + [0x0000, 0x8000, 0x0001, 0x00ff, 0x80ff]
        b = np.resize(np.array(vals, dtype=np.uint16), (2, 4096))
        W = from_bits(b)
        assert quant.check_pk13(W) == (bh, 0), top
        assert np.array_equal(bits_of(quant.unpack_pk13(quant.pack_pk13(W, bh), bh)), b), top
        if bh > 0:          # one code further down: E >> 1 == bh is outside (code 0 is taken by E >> 1 == 0)
            b2 = b.copy()
            b2[1, 77] = (bh << 8) | 0xff
            b2[0, 9] = 0x8000 | (1 << 8)       # E >> 1 = 1 <= bh as well
            assert quant.check_pk13(from_bits(b2)) == (bh, 2 if bh >= 1 else 1), top


def test_check_counts_inf_nan_and_values_below_the_window():
    W = edge_weights(4, 4096, seed=1)
    b = bits_of(W).copy()
    bh, bad = quant.check_pk13(W)
    assert bad == 0
    b[1, 30] = ((bh + 1) << 8) | 0x11         # on the lower edge of the window
    b[2, 31] = 0x8000 | ((bh + 1) << 8)
    assert quant.check_pk13(from_bits(b)) == (bh, 0)
    b[0, 10] = 0x7f80         # +Inf
    b[1, 11] = 0xff80         # -Inf
    b[2, 12] = 0x7fc0         # NaN
    b[3, 13] = 0xffff         # NaN
    assert quant.check_pk13(from_bits(b)) == (bh, 4)          # the non-finite values do not move the base
    b[0, 20] = 0x0100         # E = 2: a normal value far below the window
    b[0, 21] = (bh << 8) | 0x80       # E >> 1 == bh: just below
    assert quant.check_pk13(from_bits(b)) == (bh, 6)
    b[0, 22] = ((bh + 16) << 8)       # a larger maximum moves the window up by one code ...
    got_bh, got_bad = quant.check_pk13(from_bits(b))
    below = int((((b >> 8) & 0x7f) == bh + 1).sum())          # ... and everything on the old lower edge falls out
    assert got_bh == bh + 1 and got_bad == 6 + below and below == 2


# ---- 2. the layout --------------------------------------------------------------------------------------------------------------------
def test_piece_offsets_of_one_weight():
    """Weight (row, k) with k = unit * 4096 + chunk * 512 + lane * 8 + e of a matrix that is +1.0 everywhere else."""
    N, K = 3, 8192
    one = 0x3f80                                  # 1.0: E >> 1 = 63, low byte 0x80
    bh = 63 - 15
    base = quant.pack_pk13(from_bits(np.full((N, K), one, dtype=np.uint16)), bh).numpy()
    assert (base[:, :, :4096] == 0x80).all() and (base[:, :, 4096:6144] == 0xff).all() and (base[:, :, 6144:] == 0).all()
    g = np.random.default_rng(2)
    for _ in range(64):
        row, unit, c, lane, e = (int(g.integers(0, n)) for n in (N, 2, 8, 64, 8))
        b = np.full((N, K), one, dtype=np.uint16)
        b[row, unit * 4096 + c * 512 + lane * 8 + e] = 0x8000 | ((bh + 3) << 8) | 0x55      # negative, code 3, low byte 0x55
        P = quant.pack_pk13(from_bits(b), bh).numpy()
        diff = {tuple(int(v) for v in i): (int(base[tuple(i)]), int(P[tuple(i)])) for i in np.argwhere(P != base)}
        lo_at = (c >> 1) * 1024 + lane * 16 + (c & 1) * 8 + e
        code_at = 4096 + (c >> 2) * 1024 + lane * 16 + (c & 3) * 4 + (e & 3)
        sign_at = 6144 + lane * 8 + (c >> 2) * 4 + (e & 3)
        code = 0xf3 if e < 4 else 0x3f
        assert diff == {(row, unit, lo_at): (0x80, 0x55), (row, unit, code_at): (0xff, code),
                        (row, unit, sign_at): (0, 1 << ((c & 3) * 2 + (e >> 2)))}, (row, unit, c, lane, e)
    assert quant.PK13_UNIT_BYTES == 4 * 1024 + 2 * 1024 + 512 == 6656 and quant.PK13_UNIT_K == 4096


# ---- 3. one lane's decoding -----------------------------------------------------------------------------------------------------------
def lane_operands(unit, lane, c, bh):
    """What consume() hands to its fmas for chunk c: gemv_pk13_body.h restated on the unit's bytes, dword by dword."""
    d = np.frombuffer(unit.tobytes(), dtype="<u4")
    lo = [int(d[((c >> 1) * 1024 + lane * 16) // 4 + (c & 1) * 2 + j]) for j in (0, 1)]
    hd = int(d[(4096 + (c >> 2) * 1024 + lane * 16) // 4 + (c & 3)])
    sd = int(d[(6144 + lane * 8) // 4 + (c >> 2)])
    out = []
    for half in (0, 1):
        x = (hd >> (4 * half)) & 0x0f0f0f0f
        nz = ((x + 0x0f0f0f0f) >> 4) & 0x01010101
        hb = 0
        for h16 in (0, 16):      # the packed 16-bit multiply-add
            hb |= ((((nz >> h16) & 0xffff) * bh + ((x >> h16) & 0xffff)) & 0xffff) << h16
        hb |= (sd << (7 - ((c & 3) * 2 + half))) & 0x80808080
        for e in range(4):       # v_perm_b32: high byte, low byte, two zero bytes
            out.append((((hb >> (8 * e)) & 0xff) << 24) | (((lo[half] >> (8 * e)) & 0xff) << 16))
    return np.array(out, dtype=np.uint32)


def test_lane_decoding_gives_the_bf16_kernel_operands_bit_for_bit():
    W = edge_weights(3, 8192, seed=3)
    bh, bad = quant.check_pk13(W)
    assert bad == 0
    P = quant.pack_pk13(W, bh).numpy()
    want = bits_of(W).astype(np.uint32) << 16          # lo_bf / hi_bf of W
    for row in range(3):
        for unit in range(2):
            for c in range(8):
                for lane in range(64):
                    k0 = unit * 4096 + c * 512 + lane * 8
                    assert np.array_equal(lane_operands(P[row, unit], lane, c, bh), want[row, k0:k0 + 8]), (row, unit, c, lane)


# ---- 4. the plan and the entries --------------------------------------------------------------------------------------------------------
DECODE_SHAPES = [("8b qkv", 6144, 4096, STORE, True), ("8b o_proj", 4096, 4096, RESIDUAL, False), ("8b gate_up", 24576, 4096, SILU_MUL, True),
                 ("8b down", 4096, 12288, RESIDUAL, False), ("8b lm_head", 151936, 4096, LOGITS, True)]


def test_plan(hip_lib):
    from aha_amd import ops
    have = shipped()
    assert ops.plan_gemv_pk13(6144, 4096, STORE, True) == (1, 8, 768, 3)
    assert ops.plan_gemv_pk13(4096, 4096, RESIDUAL, False) == (1, 8, 512, 2)          # whole rounds: 1024 tiles on 512 blocks
    assert ops.plan_gemv_pk13(24576, 4096, SILU_MUL, True) == (1, 8, 768, 3)          # 3072 tiles, four rounds
    assert ops.plan_gemv_pk13(4096, 12288, RESIDUAL, False) == (1, 8, 512, 2)
    assert ops.plan_gemv_pk13(151936, 4096, LOGITS, True) == (2, 8, 768, 3)
    assert ops.plan_gemv_pk13(64, 12288, STORE, True)[3] == 1 and ops.plan_gemv_pk13(64, 20480, STORE, False)[3] == 1
    g = np.random.default_rng(0)
    for _ in range(300):
        e = int(g.integers(0, 4))
        n = int(g.integers(1, 200000))
        n = max(32, n // 32 * 32) if e == SILU_MUL else n
        k = int(g.integers(1, 9)) * 4096
        nm = bool(g.integers(0, 2))
        r, u, grid, form = ops.plan_gemv_pk13(n, k, e, nm)
        rows = n // 2 if e == SILU_MUL else n
        assert (r, e, form - 1) in have and u == 8
        assert 1 <= grid <= min(768, -(-rows // (4 * r)))          # no block without a tile: the first request is unconditional
        assert 7 * r * (2 if e == SILU_MUL else 1) <= 14             # loads per buffer
        assert (form >= 2) == (k <= (8192 if nm else 16384)) and (form == 3) == (form >= 2 and nm)
    # by plan (profiles/weights_pk13.md): of the 8B decode matrices gate+up, down and lm_head -- qkv and o_proj measured no faster;
    # nothing below 2^25 elements, nothing in part units
    assert [ops.gemv_pk13_by_plan(n, k, e) for _, n, k, e, _ in DECODE_SHAPES] == [False, False, True, True, True]
    assert not ops.gemv_pk13_by_plan(8160, 4096, SILU_MUL) and ops.gemv_pk13_by_plan(8192, 4096, SILU_MUL)
    for n, k, e in ((4096, 1024, STORE), (1024, 2048, RESIDUAL), (6144, 1024, SILU_MUL), (1024, 3072, RESIDUAL), (151936, 1024, LOGITS)):
        assert not ops.gemv_pk13_by_plan(n, k, e)          # Qwen3-0.6B: no whole unit in a row


def test_entries_in_every_layer_and_argument_checks_need_no_gpu(hip_lib):
    from aha_amd import _lib, model, ops
    import test_host_cpu
    header = open(os.path.join(ROOT, "include", "aha_hip.h")).read()
    for decl in (r"int aha_hip_debug_pk13_single\(aha_model\* m, int on\);", r"int aha_hip_pk13_status\(const aha_model\* m, char\* buf, size_t cap\);",
                 r"int aha_hip_pack_pk13\(const void\* W, int32_t N, int32_t K, void\* out, int32_t\* bh_out, int64_t\* bad_out, void\* stream\);",
                 r"int aha_hip_gemv_pk13\(const void\* packed, int32_t bh, const void\* x,", r"int aha_hip_debug_plan_gemv_pk13\(int32_t N,"):
        assert re.search(decl, header), decl
    raw = C.CDLL(_lib.LIB_PATH)
    for name, nargs in (("aha_hip_debug_pk13_single", 2), ("aha_hip_pk13_status", 3), ("aha_hip_pack_pk13", 7), ("aha_hip_gemv_pk13", 13),
                        ("aha_hip_debug_plan_gemv_pk13", 9)):
        assert hasattr(raw, name) and len(_lib.SIGNATURES[name][1]) == nargs, name
    assert set(_lib.SIGNATURES) == set(test_host_cpu._declared_symbols())
    assert all(callable(f) for f in (ops.pack_pk13, ops.gemv_pk13, ops.plan_gemv_pk13, model.HipInferenceModel.debug_pk13_single,
                                     model.HipInferenceModel.pk13_status))
    err = hip_lib.aha_hip_last_error
    buf = (C.c_uint8 * 4096)()
    p = C.addressof(buf)
    f = C.c_float(1e-6)
    bh, bad = C.c_int32(), C.c_int64()
    assert hip_lib.aha_hip_debug_pk13_single(None, 1) == -1 and b"debug_pk13_single: null model" in err()
    assert hip_lib.aha_hip_pk13_status(None, None, 0) == -1 and b"pk13_status" in err()
    assert hip_lib.aha_hip_pack_pk13(p, 4, 2048, p, C.byref(bh), C.byref(bad), None) == -1 and b"multiple of 4096" in err()
    assert hip_lib.aha_hip_pack_pk13(None, 4, 4096, p, C.byref(bh), C.byref(bad), None) == -1 and b"pack_pk13" in err()
    assert hip_lib.aha_hip_gemv_pk13(p, 40, p, p, 32, 4104, 0, None, f, None, None, None, None) == -1 and b"gemv_pk13: K must be a multiple of 4096" in err()
    assert hip_lib.aha_hip_gemv_pk13(p, 40, p, p, 32, 36864, 0, None, f, None, None, None, None) == -1 and b"at most 32768" in err()
    assert hip_lib.aha_hip_gemv_pk13(p, 113, p, p, 32, 4096, 0, None, f, None, None, None, None) == -1 and b"bh must be 0..112" in err()
    assert hip_lib.aha_hip_gemv_pk13(None, 40, p, p, 32, 4096, 0, None, f, None, None, None, None) == -1 and b"null matrix or x" in err()
    assert hip_lib.aha_hip_gemv_pk13(p, 40, p, p, 32, 4096, 1, None, f, None, None, None, None) == -1 and b"needs a residual" in err()
    assert hip_lib.aha_hip_gemv_pk13(p, 40, p, p, 48, 4096, 2, None, f, None, None, None, None) == -1 and b"N % 32" in err()
    assert hip_lib.aha_hip_gemv_pk13(p, 40, p, None, 32, 4096, 3, None, f, None, None, None, None) == -1 and b"logits and argmax_out" in err()
    r = C.c_int32()
    assert hip_lib.aha_hip_debug_plan_gemv_pk13(64, 2048, 0, 0, C.byref(r), C.byref(r), C.byref(r), None, None) == -1 and b"debug_plan_gemv_pk13" in err()
    # only AHA_WPACK is read from the environment, and only where a model is created
    for fn in ("kernels_gemv_pk13.hip", "gemv_pk13_body.h"):
        assert "getenv" not in open(os.path.join(ROOT, "aha_amd", "csrc", fn)).read(), fn
    from aha_amd import build
    assert "kernels_gemv_pk13.hip" in build.SOURCES and build.FLAGS_LIKE["kernels_gemv_pk13.hip"] == "kernels_gemv.hip"


# ---- 5. the code object ---------------------------------------------------------------------------------------------------------------
def test_instantiations_in_the_code_object(kernels):  # noqa: F811
    fam = {n: k for n, k in kernels.items() if "gemv_kernel_pk13" in n}
    got = set()
    for n, k in fam.items():
        m = re.search(r"gemv_kernel_pk13ILi(\d+)ELi(\d+)ELi(\d)EE", n)
        assert m, n
        got.add(tuple(int(x) for x in m.groups()))
        assert k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0 and k["private_segment_fixed_size"] == 0, (n, k)
        assert k["max_flat_workgroup_size"] == 256 and k["group_segment_fixed_size"] == 0, (n, k)     # launch bounds 256; LDS is dynamic
        assert k["vgpr_count"] <= 170, (n, k["vgpr_count"])          # 12 waves per CU, as the bf16 kernel
    assert got == shipped(), (sorted(got - shipped()), sorted(shipped() - got))
    # the name carries "gemv_kernel": bench.py and scripts/pmc_summary.py sum the matvec class by that substring, and the packed launches
    # belong to it; the bf16 kernel's own scans match "gemv_kernelI", which these names do not contain
    assert not any("gemv_kernelI" in n for n in fam) and all(isa.family(n) == "gemv_kernel" for n in fam)


def test_leading_arguments_are_preloaded(preload_kernels):  # noqa: F811
    """packed, x, norm_w, y, the residual vector, N, K and bh: 13 dwords in user SGPRs at wave launch, as the bf16 matvec's."""
    fam = {n: k for n, k in preload_kernels.items() if "gemv_kernel_pk13" in n}
    assert len(fam) == len(shipped())
    assert all(k["kernarg_preload_length"] >= 13 for k in fam.values()), {n: k["kernarg_preload_length"] for n, k in fam.items()}
