"""CPU tier: MXFP4 weight copies (aha_hip_model_quantize_weights with AHA_WQ_MXFP4_E2M1) -- the reference quantiser of aha_amd/quant.py
against an independent restatement of the format and against its stated properties, the nibble and scale-word orders, the new entries in
every layer of the ABI with their GPU-free argument checks, and the FP4 matvec's instantiations in the shipped gfx950 code object."""
import ctypes as C
import glob
import inspect
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_isa_cpu as isa  # noqa: E402  (helpers only: family, LLVM, and its module-scoped `kernels` fixture below)
from test_isa_cpu import kernels  # noqa: E402,F401

GRID = (0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0)
# v = |w| / 2^e half way between two magnitudes -> the index of the even code
TIES = ((0.25, 0), (0.75, 2), (1.25, 2), (1.75, 4), (2.5, 4), (3.5, 6), (5.0, 6))
ONE_STEP_ABOVE_LIMIT = 0x7f41          # bf16 pattern of 1.5 * 2^127 plus one step
ROUNDS_DOWN_ROW = 40                   # edge_matrix: the block whose amax rounds down


def bf16_bits(t):
    return t.contiguous().view(torch.int16)


def from_bits(pattern):
    return torch.tensor([pattern], dtype=torch.int32).to(torch.int16).view(torch.bfloat16)[0]


def edge_matrix():
    """(96, 160) bf16: random rows of mixed magnitude plus the hand-built edge blocks."""
    g = torch.Generator().manual_seed(7)
    W = (torch.randn(96, 160, generator=g) * torch.exp2(torch.randint(-12, 6, (96, 5, 1), generator=g).float()).expand(96, 5, 32)
         .reshape(96, 160)).bfloat16()
    W[3, 32:64] = 0.0                                  # an all-zero block
    W[3, 40] = -0.0                                    # a -0.0 inside it
    W[17, 5] = -0.0                                    # +-0 inside ordinary blocks
    W[17, 6] = 0.0
    # every tie at several block exponents: the block's amax is 6 * 2^e exactly, its other elements are the tie values of both signs
    for r, e in ((20, -20), (21, -3), (22, 0), (23, 7), (24, 100), (25, -124)):
        W[r, 0:32] = 0.0
        W[r, 0] = 6.0 * 2.0 ** e
        for j, (v, _) in enumerate(TIES):
            W[r, 1 + 2 * j] = v * 2.0 ** e
            W[r, 2 + 2 * j] = -v * 2.0 ** e
    W[30, 64:96] = (torch.rand(32, generator=g) * 2.0 ** -8).bfloat16()   # below the amax set next
    W[30, 70] = 6.0 * 2.0 ** -9                        # amax exactly 6 * 2^-9: scale byte 118
    W[31, 64:96] = W[30, 64:96]
    W[31, 70] = from_bits(int(bf16_bits(W[30, 70:71])[0]) + 1)   # one bf16 step above it: scale byte 119
    W[33, 96:128] = (torch.randn(32, generator=g) * 1e-39).bfloat16()    # bf16 subnormals: e clamps at -125
    W[33, 100] = from_bits(0x0060)                     # 0.75 * 2^-126 = 0.375 * 2^-125 -> 0.5 * 2^-125 = 2^-126
    W[33, 101] = from_bits(0x0040)                     # 2^-127 = 0.25 * 2^-125: the tie to 0
    W[33, 102] = from_bits(0x8001)                     # the smallest negative subnormal -> -0
    W[35, 128:160] = (torch.randn(32, generator=g) * 1e30).bfloat16()
    W[35, 130] = 1.5 * 2.0 ** 127                      # the largest weight the format takes: e = 125, code 7
    W[35, 131] = -1.5 * 2.0 ** 127
    W[ROUNDS_DOWN_ROW, 0:32] = 0.0                     # amax 3.25 rounds down to 3: W' quantises with e - 1 and doubled codes
    W[ROUNDS_DOWN_ROW, 0] = 3.25
    W[ROUNDS_DOWN_ROW, 1] = -1.0
    W[ROUNDS_DOWN_ROW, 2] = 0.5
    return W.contiguous()


def independent_quantize(W):
    """The format restated without aha_amd.quant: the exponent by exact search in float64, the elements by nearest-grid search with the
    tie rule (of two equally near magnitudes the one with the even index).  Returns unpacked codes (N, K), scale bytes, W' in float64."""
    N, K = W.shape
    w = W.double().reshape(N, K // 32, 32)
    amax = w.abs().amax(-1)
    e = torch.full(amax.shape, -125, dtype=torch.int64)
    for cand in range(125, -126, -1):                  # the smallest e in [-125, 125] with amax <= 6 * 2^e
        e = torch.where(amax <= 6.0 * 2.0 ** cand, torch.full_like(e, cand), e)
    assert bool((amax <= 6.0 * torch.exp2(e.double())).all())
    assert bool(((amax > 6.0 * torch.exp2((e - 1).double())) | (e == -125)).all())
    v = w.abs() / torch.exp2(e.double())[..., None]    # exact
    grid = torch.tensor(GRID, dtype=torch.float64)
    d = (v[..., None] - grid).abs()                    # (N, nb, 32, 8)
    best = d.amin(-1, keepdim=True)
    near = d == best                                   # one or two candidates
    even = torch.tensor([i % 2 == 0 for i in range(8)])
    pick = torch.where(near.sum(-1, keepdim=True) > 1, near & even, near)
    assert bool((pick.sum(-1) == 1).all())
    idx = pick.to(torch.int64).argmax(-1)
    neg = torch.signbit(w)
    mag = grid[idx] * torch.exp2(e.double())[..., None]
    wr = torch.where(neg, -mag, mag).reshape(N, K)
    codes = (idx + 8 * neg.to(torch.int64)).to(torch.uint8).reshape(N, K)
    return codes, (e + 127).to(torch.uint8), wr


def test_reference_quantiser_against_independent_restatement():
    from aha_amd import quant
    W = edge_matrix()
    q, s, wr = quant.quantize_mxfp4(W)
    assert q.dtype == torch.uint8 and s.dtype == torch.uint8 and wr.dtype == torch.bfloat16
    assert q.shape == (96, 80) and s.shape == (96, 5) and wr.shape == (96, 160)
    c2, s2, wr2 = independent_quantize(W)
    c = quant.unpack_nibbles(q)
    assert torch.equal(s, s2)
    assert torch.equal(c, c2)
    assert torch.equal(wr.double(), wr2) and torch.equal(torch.signbit(wr), torch.signbit(wr2))   # W' is exact in bf16, -0 included
    # the edge blocks
    assert int(s[3, 1]) == -125 + 127 and not bool((c[3, 32:64] & 7).any()) and int(c[3, 40]) == 0x8 and int(c[3, 41]) == 0
    assert int(c[17, 5]) == 0x8 and int(bf16_bits(wr)[17, 5]) == -32768 and int(c[17, 6]) == 0 and int(bf16_bits(wr)[17, 6]) == 0
    for r, e in ((20, -20), (21, -3), (22, 0), (23, 7), (24, 100), (25, -124)):
        assert int(s[r, 0]) == e + 127 and int(c[r, 0]) == 7, r
        for j, (v, idx) in enumerate(TIES):
            assert int(c[r, 1 + 2 * j]) == idx and int(c[r, 2 + 2 * j]) == 8 + idx, (r, v)
            assert float(wr[r, 1 + 2 * j]) == GRID[idx] * 2.0 ** e and float(wr[r, 2 + 2 * j]) == -GRID[idx] * 2.0 ** e, (r, v)
    assert int(s[30, 2]) == 118 and int(c[30, 70]) == 7
    assert int(s[31, 2]) == 119 and int(c[31, 70]) == 5            # 6.03 * 2^-9 = 3.02 * 2^-8 -> 3
    assert int(s[33, 3]) == -125 + 127
    assert int(c[33, 100]) == 1 and float(wr[33, 100]) == 2.0 ** -126 and int(c[33, 101]) == 0 and int(c[33, 102]) == 0x8
    assert int(s[35, 4]) == 125 + 127 and int(c[35, 130]) == 7 and int(c[35, 131]) == 15
    assert float(wr[35, 130]) == 1.5 * 2.0 ** 127 and float(wr[35, 131]) == -1.5 * 2.0 ** 127
    assert torch.equal(bf16_bits(quant.dequantize_mxfp4(q, s)), bf16_bits(wr))
    # the block whose amax rounds down (3.25 -> 3 at e = 0): W' = (3, -1, 0.5, 0...) round-trips, with e - 1 and doubled codes
    r = ROUNDS_DOWN_ROW
    assert int(s[r, 0]) == 127 and [int(x) for x in c[r, 0:3]] == [5, 10, 1]
    q3, s3, wr3 = quant.quantize_mxfp4(wr)
    assert torch.equal(bf16_bits(wr3), bf16_bits(wr))
    assert int(s3[r, 0]) == 126 and [int(x) for x in quant.unpack_nibbles(q3)[r, 0:3]] == [7, 12, 2]


def test_block_whose_amax_rounds_down_round_trips_with_other_bytes():
    from aha_amd import quant
    W = torch.zeros(1, 32).bfloat16()
    W[0, 0], W[0, 1], W[0, 2] = 3.25, -1.0, 0.5        # e = 0 (3 < 3.25 <= 6): 3.25 -> 3, so W' has amax 3 = 6 * 2^-1
    q, s, wr = quant.quantize_mxfp4(W)
    assert int(s[0, 0]) == 127 and [float(x) for x in wr[0, 0:3]] == [3.0, -1.0, 0.5]
    q2, s2, wr2 = quant.quantize_mxfp4(wr)
    assert torch.equal(bf16_bits(wr2), bf16_bits(wr))  # W' round-trips
    assert int(s2[0, 0]) == 126 and not torch.equal(q2, q)   # with e - 1 and doubled codes


@pytest.mark.parametrize("seed", [0, 1])
def test_reference_quantiser_properties(seed):
    from aha_amd import quant
    g = torch.Generator().manual_seed(seed)
    mats = [edge_matrix(), (torch.randn(64, 256, generator=g) * 0.02).bfloat16(),
            (torch.randn(32, 96, generator=g) * torch.exp2(torch.randint(-100, 100, (32, 1), generator=g).float())).bfloat16()]
    grid = torch.tensor(GRID, dtype=torch.float64)
    for W in mats:
        q, s, wr = quant.quantize_mxfp4(W)
        c2, s2, wr2 = independent_quantize(W)
        assert torch.equal(quant.unpack_nibbles(q), c2) and torch.equal(s, s2)
        c = quant.unpack_nibbles(q)
        e = (s.to(torch.int32) - 127).double().repeat_interleave(32, dim=1)
        w, w2 = W.double(), wr.double()
        exact = torch.where((c & 8) != 0, -1.0, 1.0) * grid[(c & 7).long()] * torch.exp2(e)   # q * 2^e in f64: no rounding
        assert bool(torch.isfinite(exact).all()) and torch.equal(w2, exact)                   # W' is exact in bf16
        assert bool(((w2 == 0) | (w2.abs() >= 2.0 ** -126)).all())
        assert torch.equal(bf16_bits(quant.dequantize_mxfp4(q, s)), bf16_bits(wr))
        assert bool(((w2 - w).abs() <= torch.maximum(w.abs() / 4, torch.exp2(e - 2))).all())
        _, _, wr3 = quant.quantize_mxfp4(wr)
        assert torch.equal(bf16_bits(wr3), bf16_bits(wr))                                     # a fixed point on W'


def test_reference_quantiser_refuses():
    from aha_amd import quant
    with pytest.raises(ValueError):
        quant.quantize_mxfp4(torch.zeros(4, 48).bfloat16())          # K % 32
    with pytest.raises(ValueError):
        quant.quantize_mxfp4(torch.zeros(4, 64))                     # not bf16
    for bad_value in (float("nan"), float("inf"), -float("inf")):
        bad = torch.zeros(4, 64).bfloat16()
        bad[1, 3] = bad_value
        with pytest.raises(ValueError):
            quant.quantize_mxfp4(bad)
    ok = torch.zeros(4, 64).bfloat16()
    ok[2, 9] = 1.5 * 2.0 ** 127
    assert float(quant.quantize_mxfp4(ok)[2][2, 9]) == 1.5 * 2.0 ** 127
    for sign in (0, 0x8000):
        over = torch.zeros(4, 64).bfloat16()
        over[2, 9] = from_bits(ONE_STEP_ABOVE_LIMIT | sign)
        assert abs(float(over[2, 9])) == 1.5078125 * 2.0 ** 127
        with pytest.raises(ValueError):
            quant.quantize_mxfp4(over)


def test_nibble_and_scale_word_orders():
    from aha_amd import quant
    codes = (torch.arange(2 * 64, dtype=torch.int32).reshape(2, 64) * 7 % 16).to(torch.uint8)
    q = quant.pack_nibbles(codes)
    assert q.dtype == torch.uint8 and q.shape == (2, 32)
    assert int(q[1, 5]) == int(codes[1, 10]) | int(codes[1, 11]) << 4          # even k in bits 0..3, odd k in bits 4..7
    assert torch.equal(quant.unpack_nibbles(q), codes)
    W = torch.zeros(1, 32).bfloat16()
    W[0, 0], W[0, 1] = 6.0, -0.5                                                # codes 7 and 9 -> byte 0x97
    assert int(quant.quantize_mxfp4(W)[0][0, 0]) == 0x97
    s = torch.arange(3 * 5, dtype=torch.uint8).reshape(3, 5) + 100              # the FP8 layout, shared
    k = quant.scales_to_kernel(s)
    assert k.dtype == torch.int32 and k.shape == (3, 2)
    b = k.numpy().view(np.uint32)
    assert int(b[1, 0]) == (105 | 106 << 8 | 107 << 16 | 108 << 24) and int(b[1, 1]) == (109 | 127 << 8 | 127 << 16 | 127 << 24)
    assert torch.equal(quant.scales_from_kernel(k, 160), s)


def test_header_arithmetic_equals_reference_on_every_bf16_pattern(tmp_path):
    """csrc/mxfp4.h compiled for the host (tests/mxfp4_host_quantize.cpp runs it block by block as the kernel does) against quant.py:
    the edge matrix, and every bf16 pattern the format takes -- each block of 32 neighbouring patterns, and the same patterns transposed
    so that a block mixes magnitudes from 2^-133 to 2^127."""
    import struct
    from aha_amd import quant
    cxx = f"{isa.LLVM}/clang++"
    if not os.path.exists(cxx):
        pytest.skip("ROCm clang++ not found")
    exe = tmp_path / "mxfp4_host_quantize"
    subprocess.run([cxx, "-O1", "-std=c++17", "-I", os.path.join(ROOT, "aha_amd", "csrc"), os.path.join(ROOT, "tests", "mxfp4_host_quantize.cpp"),
                    "-o", str(exe)], check=True, capture_output=True)
    pats = torch.arange(0, 65536, dtype=torch.int32).to(torch.int16).view(torch.bfloat16).reshape(2048, 32).clone()
    pats[(bf16_bits(pats).int() & 0x7fff) >= ONE_STEP_ABOVE_LIMIT] = 0.0
    for W in (edge_matrix(), pats, pats.t().contiguous().reshape(2048, 32)):
        N, K = W.shape
        (tmp_path / "in.bin").write_bytes(struct.pack("ii", N, K) + bf16_bits(W).numpy().tobytes())
        subprocess.run([str(exe), str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], check=True)
        raw = np.fromfile(tmp_path / "out.bin", dtype=np.uint8)
        nq, ns = N * K // 2, N * K // 32
        q, s, wr = quant.quantize_mxfp4(W)
        assert np.array_equal(raw[:nq].reshape(N, K // 2), q.numpy())
        assert np.array_equal(raw[nq:nq + ns].reshape(N, K // 32), s.numpy())
        assert np.array_equal(raw[nq + ns:].view(np.int16).reshape(N, K), bf16_bits(wr).numpy())


def test_weights_fp4_entries_in_every_layer(hip_lib):
    from aha_amd import _lib, model, ops, quant
    header = open(os.path.join(ROOT, "include", "aha_hip.h")).read()
    assert re.search(r"int aha_hip_quantize_mxfp4\(const void\* W, int32_t N, int32_t K, void\* q_out, uint32_t\* scales_out, "
                     r"void\* w_roundtrip_out, void\* stream\);", header)
    assert re.search(r"int aha_hip_gemv_rows_mxfp4\(const void\* q, const uint32_t\* scales, const void\* x, void\* y, int32_t R, int32_t N, "
                     r"int32_t K, int32_t epi,\s+const void\* residual, float\* logits, uint32_t\* argmax_out, void\* stream\);", header)
    assert re.search(r"#define AHA_WQ_MXFP4_E2M1 2\b", header) and re.search(r"#define AHA_WQ_MXFP8_E4M3 1\b", header)
    assert _lib.AHA_WQ_MXFP4_E2M1 == 2 and _lib.AHA_WQ_MXFP8_E4M3 == 1 and _lib.AHA_WQ_NONE == 0
    for name, nargs in (("aha_hip_quantize_mxfp4", 7), ("aha_hip_gemv_rows_mxfp4", 12)):
        assert hasattr(hip_lib, name), name
        assert len(_lib.SIGNATURES[name][1]) == nargs, name
    assert _lib.SIGNATURES["aha_hip_gemv_rows_mxfp4"] == _lib.SIGNATURES["aha_hip_gemv_rows_mxfp8"]
    assert _lib.SIGNATURES["aha_hip_quantize_mxfp4"] == _lib.SIGNATURES["aha_hip_quantize_mxfp8"]
    assert callable(ops.quantize_mxfp4) and callable(ops.gemv_rows_mxfp4)
    assert callable(quant.quantize_mxfp4) and callable(quant.dequantize_mxfp4)
    src = inspect.getsource(model.HipInferenceModel.quantize_weights) + inspect.getsource(model.HipInferenceModel.weight_format.fget)
    assert '"mxfp4"' in src and "AHA_WQ_MXFP4_E2M1" in src
    rs = open(os.path.join(ROOT, "rust", "aha-hip", "src", "lib.rs")).read()
    ext = rs[rs.index('extern "C" {'):]
    ext = ext[:ext.index("\n    }\n")]
    assert re.search(r"pub fn aha_hip_quantize_mxfp4\(", ext) and re.search(r"pub fn aha_hip_gemv_rows_mxfp4\(", ext)
    assert re.search(r"pub const AHA_WQ_MXFP4_E2M1: i32 = 2;", rs) and re.search(r"Mxfp4E2m1 = 2,", rs)
    assert re.search(r"sys::AHA_WQ_MXFP4_E2M1 => Some\(\(WeightFormat::Mxfp4E2m1", rs)      # handled in weight_format
    build = open(os.path.join(ROOT, "aha_amd", "build.py")).read()
    assert '"kernels_gemv_rows_fp4.hip"' in build


def test_weights_fp4_argument_checks_need_no_gpu(hip_lib):
    err = hip_lib.aha_hip_last_error
    assert hip_lib.aha_hip_model_quantize_weights(None, 2, 0) == -1 and b"quantize_weights: null model" in err()
    assert hip_lib.aha_hip_quantize_mxfp4(None, 4, 64, None, None, None, None) == -1 and b"quantize_mxfp4: bad arguments" in err()
    buf = (C.c_uint8 * 4096)()
    p = C.addressof(buf)
    assert hip_lib.aha_hip_quantize_mxfp4(p, 4, 48, p, p, None, None) == -1 and b"multiple of 32" in err()       # K % 32
    assert hip_lib.aha_hip_gemv_rows_mxfp4(None, None, None, None, 0, 0, 0, 0, None, None, None, None) == -1
    assert b"gemv_rows_mxfp4: bad arguments" in err()
    assert hip_lib.aha_hip_gemv_rows_mxfp4(p, p, p, p, 33, 32, 64, 0, None, None, None, None) == -1              # R > 32
    assert hip_lib.aha_hip_gemv_rows_mxfp4(p, p, p, p, 1, 32, 40, 0, None, None, None, None) == -1               # K % 32
    assert hip_lib.aha_hip_gemv_rows_mxfp4(p, p, p, p, 1, 32, 64, 3, None, None, None, None) == -1               # logits epilogue without outputs
    assert hip_lib.aha_hip_gemv_rows_mxfp4(p, None, p, p, 1, 32, 64, 0, None, None, None, None) == -1            # null scales
    assert hip_lib.aha_hip_gemv_rows_mxfp4(p, p, p, None, 1, 32, 64, 1, None, None, None, None) == -1            # residual epilogue without residual
    from aha_amd.model import HipInferenceModel
    with pytest.raises(ValueError):
        HipInferenceModel.quantize_weights(object(), "int4")
    with pytest.raises(ValueError):
        HipInferenceModel.quantize_weights(object(), "mxfp6")


def test_fp4_matvec_kernels_in_the_code_object(kernels, tmp_path):  # noqa: F811
    fam = {n: k for n, k in kernels.items() if isa.family(n) == "gemv_rows_mxfp4_kernel"}
    assert len(fam) == 4, sorted(fam)                   # <CW, NRT> in {1, 2} x {1, 2}
    for n, k in fam.items():
        assert k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0 and k["private_segment_fixed_size"] == 0, (n, k)
        assert k["vgpr_count"] <= 256 and k["max_flat_workgroup_size"] == 256, (n, k)    # launch bounds (256, 2)
    assert any(isa.family(n) == "mxfp4_quantize_kernel" for n in kernels) and any(isa.family(n) == "mxfp4_check_kernel" for n in kernels)
    assert len([n for n in kernels if isa.family(n) == "gemv_rows_mxfp8_kernel"]) == 4   # a kernel of its own, not a variant of the FP8 one
    # global loads only, nothing through scratch, the same MFMA count as the bf16 kernel's instantiation, and the FP4 conversion
    shutil.copy(os.path.join(ROOT, "aha_amd", "csrc", "libaha_hip.so"), tmp_path / "lib.so")
    subprocess.run([f"{isa.LLVM}/llvm-objdump", "--offloading", "lib.so"], cwd=tmp_path, capture_output=True, check=True)
    mfma, cvt, bad, count = {}, {}, {}, {}
    for o in sorted(glob.glob(str(tmp_path / "lib.so.*gfx950"))):
        dis = subprocess.run([f"{isa.LLVM}/llvm-objdump", "-d", "--no-show-raw-insn", o], capture_output=True, text=True, check=True).stdout
        cur = None
        for line in dis.splitlines():
            m = re.match(r"^[0-9a-f]+ <(\S+)>:", line)
            if m:
                cur = m.group(1)
                continue
            if not cur or isa.family(cur) not in ("gemv_rows_mxfp4_kernel", "gemv_rows_mxfp8_kernel", "gemv_rows_kernel"):
                continue
            op = line.split()[0] if line.split() else ""
            key = (isa.family(cur), tuple(int(x) for x in re.findall(r"Li(\d+)E", cur)[:2]))
            if op in ("global_load_dwordx4", "global_load_dword", "s_barrier"):
                count[key + (op,)] = count.get(key + (op,), 0) + 1
            if op.startswith("v_mfma"):
                mfma[key] = mfma.get(key, 0) + 1
            if op == "v_cvt_scalef32_pk_bf16_fp4":
                cvt[key] = cvt.get(key, 0) + 1
            if isa.family(cur) == "gemv_rows_mxfp4_kernel" and (op.startswith("flat_load") or op.startswith("scratch_")):
                bad.setdefault(cur, []).append(op)
    assert not bad, bad
    for cw in (1, 2):
        for nrt in (1, 2):
            assert mfma[("gemv_rows_mxfp4_kernel", (cw, nrt))] == mfma[("gemv_rows_kernel", (cw, nrt))] == 8 * cw * nrt
            assert cvt[("gemv_rows_mxfp4_kernel", (cw, nrt))] == 32 * cw                # 4 per fragment, 4 fragments, 2 column tiles
    # the three weight forms are one body (csrc/gemv_rows_body.h): per chunk 4 x loads per row tile and L 16-byte weight loads for each of
    # the two column tiles, one scale dword per column tile for the MX forms, and the one barrier of the LDS reduction
    for family, L in (("gemv_rows_kernel", 4), ("gemv_rows_mxfp8_kernel", 2), ("gemv_rows_mxfp4_kernel", 1)):
        for cw in (1, 2):
            for nrt in (1, 2):
                assert count.get((family, (cw, nrt), "global_load_dwordx4"), 0) == cw * (4 * nrt + 2 * L), (family, cw, nrt)
                assert count.get((family, (cw, nrt), "global_load_dword"), 0) == (0 if family == "gemv_rows_kernel" else 2 * cw), (family, cw, nrt)
                assert count.get((family, (cw, nrt), "s_barrier"), 0) == 1, (family, cw, nrt)
