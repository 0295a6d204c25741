"""CPU tier: MXFP8 weight copies (aha_hip_model_quantize_weights) -- the reference quantiser aha_amd/quant.py against an independent
restatement of the format and against its stated properties, the new entries in every layer of the ABI with their GPU-free argument
checks, and the FP8 matvec's instantiations in the shipped gfx950 code object."""
import ctypes as C
import inspect
import os
import re
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_isa_cpu as isa  # noqa: E402  (helpers only: family, LLVM, and its module-scoped `kernels` fixture below)
from test_isa_cpu import kernels  # noqa: E402,F401


def edge_matrix():
    """(96, 160) bf16: random rows of mixed magnitude plus the hand-built edge blocks."""
    g = torch.Generator().manual_seed(7)
    W = (torch.randn(96, 160, generator=g) * torch.exp2(torch.randint(-12, 6, (96, 5, 1), generator=g).float()).expand(96, 5, 32)
         .reshape(96, 160)).bfloat16()
    W[3, 32:64] = 0.0                                  # an all-zero block
    W[5, 0:32] = (torch.rand(32, generator=g) * 0.5).bfloat16()
    W[5, 7] = 448.0 * 2.0 ** -9                        # amax exactly 448 * 2^-9: scale byte 118
    W[8, 64:96] = 0.0
    W[8, 64] = 3.0
    W[8, 65] = 1e-6                                    # beside 3.0: far below the block's subnormal grid
    W[8, 67] = 3.0 * 2.0 ** -15                        # a subnormal of the block: e = -7, grid step 2^-16
    W[11, 128:160] = (torch.randn(32, generator=g) * 1e-30).bfloat16()   # a block scaled by 1e-30
    W[13, 96:128] = (torch.randn(32, generator=g) * 1e-39).bfloat16()    # bf16 subnormals: e clamps at -117
    W[17, 5] = -0.0
    W[3, 40] = -0.0                                    # a -0.0 inside the all-zero block
    return W.contiguous()


def independent_quantize(W):
    """The format restated without aha_amd.quant: exponent by exact search in float64, elements through torch.float8_e4m3fn."""
    N, K = W.shape
    w = W.double().reshape(N, K // 32, 32)
    amax = w.abs().amax(-1)
    m, x = torch.frexp(amax)                           # amax = m * 2^x, m in [0.5, 1)
    e = (x - 9).to(torch.int64)                        # 448 * 2^(x - 9) = 0.875 * 2^x: enough iff m <= 0.875
    e = torch.where(amax > 448.0 * torch.exp2(e.double()), e + 1, e)
    e = torch.where(amax <= 448.0 * torch.exp2((e - 1).double()), e - 1, e)
    e = torch.where(amax == 0, torch.full_like(e, -117), e).clamp(-117, 120)
    assert bool((amax <= 448.0 * torch.exp2(e.double())).all())
    assert bool(((amax > 448.0 * torch.exp2((e - 1).double())) | (e == -117)).all())   # the smallest such e
    v = (w / torch.exp2(e.double())[..., None]).float()
    q8 = v.to(torch.float8_e4m3fn)
    wr = (q8.float().double() * torch.exp2(e.double())[..., None]).reshape(N, K)
    return q8.view(torch.uint8).reshape(N, K), (e + 127).to(torch.uint8), wr


def bf16_bits(t):
    return t.contiguous().view(torch.int16)


def test_reference_quantiser_against_independent_restatement():
    from aha_amd import quant
    W = edge_matrix()
    q, s, wr = quant.quantize_mxfp8(W)
    assert q.dtype == torch.uint8 and s.dtype == torch.uint8 and wr.dtype == torch.bfloat16
    assert q.shape == (96, 160) and s.shape == (96, 5) and wr.shape == (96, 160)
    q2, s2, wr2 = independent_quantize(W)
    assert torch.equal(s, s2)
    assert torch.equal(q, q2)
    assert torch.equal(wr.double(), wr2)               # W' is exact in bf16
    # the edge blocks
    assert int(s[3, 1]) == -117 + 127 and not bool((q[3, 32:64] & 0x7f).any()) and int(q[3, 40]) == 0x80
    assert int(s[5, 0]) == 118 and int(q[5, 7]) == 0x7e
    assert int(s[8, 2]) == 127 - 7 and int(q[8, 64]) == 0x7c and int(q[8, 65]) == 0 and float(wr[8, 65]) == 0.0
    assert 0 < int(q[8, 67]) < 8 and float(wr[8, 67]) == 3.0 * 2.0 ** -15     # a subnormal code, kept exactly
    assert int(s[13, 3]) == -117 + 127
    assert int(q[17, 5]) == 0x80 and int(bf16_bits(wr)[17, 5]) == -32768
    assert torch.equal(bf16_bits(quant.dequantize_mxfp8(q, s)), bf16_bits(wr))


@pytest.mark.parametrize("seed", [0, 1])
def test_reference_quantiser_properties(seed):
    from aha_amd import quant
    g = torch.Generator().manual_seed(seed)
    mats = [edge_matrix(), (torch.randn(64, 256, generator=g) * 0.02).bfloat16(),
            (torch.randn(32, 96, generator=g) * torch.exp2(torch.randint(-100, 100, (32, 1), generator=g).float())).bfloat16()]
    for W in mats:
        q, s, wr = quant.quantize_mxfp8(W)
        e = (s.to(torch.int32) - 127).double().repeat_interleave(32, dim=1)
        w, w2 = W.double(), wr.double()
        exact = q.view(torch.float8_e4m3fn).float().double() * torch.exp2(e)                  # q * 2^e in f64: no rounding
        assert bool(torch.isfinite(exact).all()) and torch.equal(w2, exact)                   # W' is exact in bf16
        assert torch.equal(bf16_bits(quant.dequantize_mxfp8(q, s)), bf16_bits(wr))
        assert bool(((w2 - w).abs() <= torch.maximum(w.abs() * 2.0 ** -4, 2.0 ** -10 * torch.exp2(e))).all())
        assert not bool(((q & 0x7f) == 0x7f).any())                                           # no NaN code
        _, _, wr3 = quant.quantize_mxfp8(wr)
        assert torch.equal(bf16_bits(wr3), bf16_bits(wr))                                     # a fixed point on W'
    with pytest.raises(ValueError):
        quant.quantize_mxfp8(torch.zeros(4, 48).bfloat16())
    bad = torch.zeros(4, 64).bfloat16()
    bad[1, 3] = float("nan")
    with pytest.raises(ValueError):
        quant.quantize_mxfp8(bad)


def test_scale_order_conversion():
    from aha_amd import quant
    s = torch.arange(3 * 5, dtype=torch.uint8).reshape(3, 5) + 100
    k = quant.scales_to_kernel(s)
    assert k.dtype == torch.int32 and k.shape == (3, 2)
    b = k.numpy().view(np.uint32)
    assert int(b[1, 0]) == (105 | 106 << 8 | 107 << 16 | 108 << 24) and int(b[1, 1]) == (109 | 127 << 8 | 127 << 16 | 127 << 24)
    assert torch.equal(quant.scales_from_kernel(k, 160), s)


def test_weights_fp8_entries_in_every_layer(hip_lib):
    from aha_amd import _lib, model, ops
    header = open(os.path.join(ROOT, "include", "aha_hip.h")).read()
    assert re.search(r"int aha_hip_model_quantize_weights\(aha_model\* m, int32_t format, uint32_t flags\);", header)
    assert re.search(r"int aha_hip_model_weight_format\(const aha_model\* m, int32_t\* format, uint32_t\* flags\);", header)
    assert re.search(r"int aha_hip_debug_fp8_rows\(aha_model\* m, int on\);", header)
    assert re.search(r"int aha_hip_quantize_mxfp8\(const void\* W, int32_t N, int32_t K, void\* q_out, uint32_t\* scales_out, "
                     r"void\* w_roundtrip_out, void\* stream\);", header)
    assert re.search(r"int aha_hip_gemv_rows_mxfp8\(const void\* q, const uint32_t\* scales, const void\* x, void\* y, int32_t R, int32_t N, "
                     r"int32_t K, int32_t epi,\s+const void\* residual, float\* logits, uint32_t\* argmax_out, void\* stream\);", header)
    assert re.search(r"#define AHA_WQ_MXFP8_E4M3 1\b", header) and re.search(r"#define AHA_WQ_LM_HEAD 1u", header)
    assert _lib.AHA_WQ_MXFP8_E4M3 == 1 and _lib.AHA_WQ_LM_HEAD == 1 and _lib.AHA_WQ_NONE == 0
    for name, nargs in (("aha_hip_model_quantize_weights", 3), ("aha_hip_model_weight_format", 3), ("aha_hip_debug_fp8_rows", 2),
                        ("aha_hip_quantize_mxfp8", 7), ("aha_hip_gemv_rows_mxfp8", 12)):
        assert hasattr(hip_lib, name), name
        assert len(_lib.SIGNATURES[name][1]) == nargs, name
    # aha_hip_gemv_rows_mxfp8 = aha_hip_gemv_rows with (q, scales) in place of W
    assert _lib.SIGNATURES["aha_hip_gemv_rows_mxfp8"][1][2:] == _lib.SIGNATURES["aha_hip_gemv_rows"][1][1:]
    sig = inspect.signature(model.HipInferenceModel.quantize_weights)
    assert list(sig.parameters) == ["self", "fmt", "lm_head"] and sig.parameters["fmt"].default == "mxfp8" and sig.parameters["lm_head"].default is False
    assert isinstance(model.HipInferenceModel.weight_format, property)
    assert callable(ops.quantize_mxfp8) and callable(ops.gemv_rows_mxfp8)
    src = open(os.path.join(ROOT, "rust", "aha-hip", "src", "lib.rs")).read()
    ext = src[src.index('extern "C" {'):]
    ext = ext[:ext.index("\n    }\n")]
    assert re.search(r"pub fn aha_hip_model_quantize_weights\(m: \*mut AhaModel, format: i32, flags: u32\) -> i32;", ext)
    assert re.search(r"pub fn aha_hip_model_weight_format\(m: \*const AhaModel, format: \*mut i32, flags: \*mut u32\) -> i32;", ext)
    assert re.search(r"pub fn quantize_weights\(&mut self, format: WeightFormat, lm_head: bool\) -> Result<\(\), Error>", src)


def test_weights_fp8_argument_checks_need_no_gpu(hip_lib):
    err = hip_lib.aha_hip_last_error
    assert hip_lib.aha_hip_model_quantize_weights(None, 1, 0) == -1 and b"quantize_weights: null model" in err()
    assert hip_lib.aha_hip_model_weight_format(None, None, None) == -1 and b"null model" in err()
    assert hip_lib.aha_hip_debug_fp8_rows(None, 1) == -1 and b"null model" in err()
    assert hip_lib.aha_hip_quantize_mxfp8(None, 4, 64, None, None, None, None) == -1 and b"quantize_mxfp8: bad arguments" in err()
    buf = (C.c_uint8 * 4096)()
    p = C.addressof(buf)
    assert hip_lib.aha_hip_quantize_mxfp8(p, 4, 48, p, p, None, None) == -1 and b"multiple of 32" in err()       # K % 32
    assert hip_lib.aha_hip_gemv_rows_mxfp8(None, None, None, None, 0, 0, 0, 0, None, None, None, None) == -1
    assert b"gemv_rows_mxfp8: bad arguments" in err()
    assert hip_lib.aha_hip_gemv_rows_mxfp8(p, p, p, p, 33, 32, 64, 0, None, None, None, None) == -1              # R > 32
    assert hip_lib.aha_hip_gemv_rows_mxfp8(p, p, p, p, 1, 32, 40, 0, None, None, None, None) == -1               # K % 32
    assert hip_lib.aha_hip_gemv_rows_mxfp8(p, p, p, p, 1, 32, 64, 3, None, None, None, None) == -1               # logits epilogue without outputs
    from aha_amd.model import HipInferenceModel
    with pytest.raises(ValueError):
        HipInferenceModel.quantize_weights(object(), "int4")


def test_fp8_matvec_kernels_in_the_code_object(kernels, tmp_path):  # noqa: F811
    import glob
    import shutil
    import subprocess
    fam = {n: k for n, k in kernels.items() if isa.family(n) == "gemv_rows_mxfp8_kernel"}
    assert len(fam) == 4, sorted(fam)                   # <CW, NRT> in {1, 2} x {1, 2}
    for n, k in fam.items():
        assert k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0 and k["private_segment_fixed_size"] == 0, (n, k)
        assert k["vgpr_count"] <= 256 and k["max_flat_workgroup_size"] == 256, (n, k)    # launch bounds (256, 2)
    assert any(isa.family(n) == "mxfp8_quantize_kernel" for n in kernels) and any(isa.family(n) == "mxfp8_check_kernel" for n in kernels)
    # global loads only, nothing through scratch, and the same MFMA count as the bf16 kernel's instantiation
    shutil.copy(os.path.join(ROOT, "aha_amd", "csrc", "libaha_hip.so"), tmp_path / "lib.so")
    subprocess.run([f"{isa.LLVM}/llvm-objdump", "--offloading", "lib.so"], cwd=tmp_path, capture_output=True, check=True)
    mfma, bad = {}, {}
    for o in sorted(glob.glob(str(tmp_path / "lib.so.*gfx950"))):
        dis = subprocess.run([f"{isa.LLVM}/llvm-objdump", "-d", "--no-show-raw-insn", o], capture_output=True, text=True, check=True).stdout
        cur = None
        for line in dis.splitlines():
            m = re.match(r"^[0-9a-f]+ <(\S+)>:", line)
            if m:
                cur = m.group(1)
                continue
            if not cur or isa.family(cur) not in ("gemv_rows_mxfp8_kernel", "gemv_rows_kernel"):
                continue
            op = line.split()[0] if line.split() else ""
            if op.startswith("v_mfma"):
                key = (isa.family(cur), tuple(int(x) for x in re.findall(r"Li(\d+)E", cur)[:2]))
                mfma[key] = mfma.get(key, 0) + 1
            if isa.family(cur) == "gemv_rows_mxfp8_kernel" and (op.startswith("flat_load") or op.startswith("scratch_")):
                bad.setdefault(cur, []).append(op)
    assert not bad, bad
    for cw in (1, 2):
        for nrt in (1, 2):
            assert mfma[("gemv_rows_mxfp8_kernel", (cw, nrt))] == mfma[("gemv_rows_kernel", (cw, nrt))] == 8 * cw * nrt
