"""CPU tier: single-sequence decode from MXFP8 weights (gemv_mxfp8_kernel, aha_amd/csrc/kernels_gemv_fp8.hip).

  * the op entries aha_hip_gemv_epi / aha_hip_gemv_mxfp8, the switch aha_hip_debug_fp8_single and the plan query
    aha_hip_debug_plan_gemv_mxfp8 in every layer of the ABI, with their GPU-free argument checks;
  * the kernel's instantiations in the shipped gfx950 code object: the set the launcher can reach and no other, no scratch, the register
    ceilings of the bf16 kernel with as many loads in flight, and -- for every straight-line instantiation -- the prologue under the first
    request: every vector-memory wait between the first non-temporal load and the barrier that ends the prologue is a counted one that
    leaves the R * U * NW weight loads and as many scale-byte loads in flight;
  * one lane's arithmetic restated in numpy: 8 E4M3 bytes and their block's scale byte give, in f32, bit for bit the values the bf16
    kernel reads from W' = the reference quantiser's dequantised matrix.
"""
import ctypes as C
import glob
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
import test_isa_cpu as isa  # noqa: E402  (helpers: family, and its module-scoped `kernels` fixture)
from test_isa_cpu import kernels  # noqa: E402,F401
from test_decode_prologue_waits_cpu import LLVM, vm_waits  # noqa: E402
from test_decode_preload_cpu import kernels as preload_kernels  # noqa: E402,F401  (its fixture, under another name)
from test_weights_fp8_cpu import bf16_bits, edge_matrix  # noqa: E402

STORE, RESIDUAL, SILU_MUL, LOGITS = 0, 1, 2, 3


# ---- the instantiations the launcher can reach (kernels_gemv_fp8.hip launch_epi) -----------------------------------------------------
def shipped():
    """{(R, U, EPI, FAST, PRO)}: U at the plan's cap min(8, 16 / (R * NW)) in all four forms; below it a FAST shape is always straight-line."""
    out = set()
    for epi in (STORE, RESIDUAL, SILU_MUL, LOGITS):
        nw = 2 if epi == SILU_MUL else 1
        for r in ((1, 2) if nw == 2 else (1, 2, 4)):
            cap = min(8, 16 // (r * nw))
            u = 1
            while u <= cap:
                out |= {(r, u, epi, 0, 0), (r, u, epi, 1, 1), (r, u, epi, 1, 2)}
                if u == cap:
                    out.add((r, u, epi, 1, 0))
                u *= 2
    return out


def plan(lib, N, K, epi, norm):
    r, u, g, f = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int32()
    assert lib.aha_hip_debug_plan_gemv_mxfp8(N, K, epi, int(norm), C.byref(r), C.byref(u), C.byref(g), C.byref(f), None) == 0
    return r.value, u.value, g.value, f.value


# ---- 1. every layer of the ABI --------------------------------------------------------------------------------------------------------
def test_single_sequence_fp8_entries_in_every_layer(hip_lib):
    from aha_amd import _lib, model, ops
    import test_host_cpu
    header = open(os.path.join(ROOT, "include", "aha_hip.h")).read()
    assert re.search(r"int aha_hip_gemv_epi\(const void\* W, const void\* x, void\* y, int32_t N, int32_t K, int32_t epi, const void\* norm_w, "
                     r"float eps,\s+const void\* residual, float\* logits, uint32_t\* argmax_out, void\* stream\);", header)
    assert re.search(r"int aha_hip_gemv_mxfp8\(const void\* q, const uint32_t\* scales, const void\* x, void\* y, int32_t N, int32_t K, int32_t epi, "
                     r"const void\* norm_w,\s+float eps, const void\* residual, float\* logits, uint32_t\* argmax_out, void\* stream\);", header)
    assert re.search(r"int aha_hip_debug_fp8_single\(aha_model\* m, int on\);", header)
    assert re.search(r"int aha_hip_debug_plan_gemv_mxfp8\(int32_t N, int32_t K, int32_t epi, int32_t has_norm, int32_t\* R, int32_t\* U, "
                     r"int32_t\* grid, int32_t\* form,\s+int32_t\* by_plan\);", header)
    raw = C.CDLL(_lib.LIB_PATH)
    for name, nargs in (("aha_hip_gemv_epi", 12), ("aha_hip_gemv_mxfp8", 13), ("aha_hip_debug_fp8_single", 2), ("aha_hip_debug_plan_gemv_mxfp8", 9)):
        assert hasattr(raw, name), name
        assert len(_lib.SIGNATURES[name][1]) == nargs, name
    # aha_hip_gemv_mxfp8 = aha_hip_gemv_epi with (q, scales) in place of W
    assert _lib.SIGNATURES["aha_hip_gemv_mxfp8"][1][2:] == _lib.SIGNATURES["aha_hip_gemv_epi"][1][1:]
    # declared == exported == bound, still
    assert set(_lib.SIGNATURES) == set(test_host_cpu._declared_symbols())
    assert callable(ops.gemv_epi) and callable(ops.gemv_mxfp8) and callable(model.HipInferenceModel.debug_fp8_single)
    src = open(os.path.join(ROOT, "rust", "aha-hip", "src", "lib.rs")).read()
    ext = src[src.index('extern "C" {'):]
    ext = ext[:ext.index("\n    }\n")]
    assert re.search(r"pub fn aha_hip_debug_fp8_single\(m: \*mut AhaModel, on: i32\) -> i32;", ext)
    assert re.search(r"pub fn aha_hip_gemv_epi\(\s+w: \*const std::ffi::c_void,", ext)
    assert re.search(r"pub fn aha_hip_gemv_mxfp8\(\s+q: \*const std::ffi::c_void,\s+scales: \*const u32,", ext)
    assert re.search(r"pub fn aha_hip_debug_plan_gemv_mxfp8\(", ext)
    # nothing of the feature reads the environment
    for f in ("kernels_gemv_fp8.hip", "gemv_fp8_body.h"):
        assert "getenv" not in open(os.path.join(ROOT, "aha_amd", "csrc", f)).read(), f


def test_single_sequence_fp8_argument_checks_need_no_gpu(hip_lib):
    err = hip_lib.aha_hip_last_error
    buf = (C.c_uint8 * 4096)()
    p = C.addressof(buf)
    f = C.c_float(1e-6)
    assert hip_lib.aha_hip_debug_fp8_single(None, 1) == -1 and b"debug_fp8_single: null model" in err()
    assert hip_lib.aha_hip_gemv_mxfp8(p, p, p, p, 32, 40, 0, None, f, None, None, None, None) == -1 and b"gemv_mxfp8: K must be a positive multiple of 32" in err()
    assert hip_lib.aha_hip_gemv_mxfp8(p, p, p, p, 32, 32800, 0, None, f, None, None, None, None) == -1 and b"gemv_mxfp8: K must be at most 32768" in err()
    assert hip_lib.aha_hip_gemv_mxfp8(p, None, p, p, 32, 64, 0, None, f, None, None, None, None) == -1 and b"gemv_mxfp8: null scales" in err()
    assert hip_lib.aha_hip_gemv_mxfp8(None, p, p, p, 32, 64, 0, None, f, None, None, None, None) == -1 and b"null matrix or x" in err()
    assert hip_lib.aha_hip_gemv_mxfp8(p, p, p, None, 32, 64, 0, None, f, None, None, None, None) == -1 and b"null y" in err()
    assert hip_lib.aha_hip_gemv_mxfp8(p, p, p, p, 32, 64, 1, None, f, None, None, None, None) == -1 and b"needs a residual" in err()
    assert hip_lib.aha_hip_gemv_mxfp8(p, p, p, p, 48, 64, 2, None, f, None, None, None, None) == -1 and b"N % 32" in err()
    assert hip_lib.aha_hip_gemv_mxfp8(p, p, p, None, 32, 64, 3, None, f, None, None, None, None) == -1 and b"logits and argmax_out" in err()
    assert hip_lib.aha_hip_gemv_mxfp8(p, p, p, p, 32, 64, 4, None, f, None, None, None, None) == -1 and b"epi must be 0..3" in err()
    assert hip_lib.aha_hip_gemv_epi(p, p, p, 32, 36, 0, None, f, None, None, None, None) == -1 and b"gemv_epi: K must be a positive multiple of 8" in err()
    assert hip_lib.aha_hip_gemv_epi(p, p, p, 32, 32776, 0, None, f, None, None, None, None) == -1 and b"at most 32768" in err()
    r = C.c_int32()
    assert hip_lib.aha_hip_debug_plan_gemv_mxfp8(64, 40, 0, 0, C.byref(r), C.byref(r), C.byref(r), None, None) == -1 and b"debug_plan_gemv_mxfp8" in err()
    assert hip_lib.aha_hip_debug_plan_gemv_mxfp8(64, 64, 0, 0, None, C.byref(r), C.byref(r), None, None) == -1


# ---- 2. the plan ----------------------------------------------------------------------------------------------------------------------
# (name, N matrix rows, K, epi, norm) of the decode step: Qwen3-8B (H 4096, I 12288, 32 / 8 heads) and Qwen3-0.6B (H 1024, I 3072, 16 / 8)
DECODE_SHAPES = [("8b qkv", 6144, 4096, STORE, True), ("8b o_proj", 4096, 4096, RESIDUAL, False), ("8b gate_up", 24576, 4096, SILU_MUL, True),
                 ("8b down", 4096, 12288, RESIDUAL, False), ("8b lm_head", 151936, 4096, LOGITS, True),
                 ("0.6b qkv", 4096, 1024, STORE, True), ("0.6b o_proj", 1024, 2048, RESIDUAL, False), ("0.6b gate_up", 6144, 1024, SILU_MUL, True),
                 ("0.6b down", 1024, 3072, RESIDUAL, False), ("0.6b lm_head", 151936, 1024, LOGITS, True)]


def test_plan_names_a_shipped_instantiation_and_a_grid_within_the_tiles(hip_lib):
    have = shipped()
    g = np.random.default_rng(0)
    shapes = [(n, k, e, nm) for _, n, k, e, nm in DECODE_SHAPES]
    for _ in range(400):
        e = int(g.integers(0, 4))
        n = int(g.integers(1, 40000))
        n = max(32, n // 32 * 32) if e == SILU_MUL else n
        shapes.append((n, int(g.integers(1, 1025)) * 32, e, bool(g.integers(0, 2))))
    for n, k, e, nm in shapes:
        r, u, grid, form = plan(hip_lib, n, k, e, nm)
        rows = n // 2 if e == SILU_MUL else n
        assert (r, u, e, int(form != 0), max(form - 1, 0)) in have, (n, k, e, nm, r, u, form)
        assert 1 <= grid <= min(768, -(-rows // (4 * r))), (n, k, e, grid)       # no block without a tile: the first request is unconditional
        assert (form != 0) == (k % (512 * u) == 0)
        assert (form >= 2) == (form != 0 and k <= (8192 if nm else 16384)) and (form == 3) == (form >= 2 and nm)
    # which matrices a model's step takes from the copies (profiles/weights_fp8_single.md): every 8B one, of 0.6B's only the lm_head
    from aha_amd import ops
    assert [ops.gemv_mxfp8_by_plan(n, k, e) for _, n, k, e, _ in DECODE_SHAPES] == [True] * 5 + [False] * 4 + [True]
    # a large matrix whose launch would take the general form (K no multiple of 512 * U) was never measured, and the one measured
    # general-form launch lost: it stays on bf16.  down_proj at I = 9728 (19 chunks at U = 8) against I = 8192
    assert not ops.gemv_mxfp8_by_plan(4096, 9728, RESIDUAL) and ops.gemv_mxfp8_by_plan(4096, 8192, RESIDUAL)
    assert not ops.gemv_mxfp8_by_plan(4095, 4096, RESIDUAL)      # below 2^24 elements
    # the 8B decode step keeps 16 half-width loads per buffer in flight on every matrix
    for name, n, k, e, nm in DECODE_SHAPES[:5]:
        r, u, _, form = plan(hip_lib, n, k, e, nm)
        assert r * u * (2 if e == SILU_MUL else 1) == 16 and form != 0, name


# ---- 3. the code object ---------------------------------------------------------------------------------------------------------------
def test_instantiations_in_the_code_object(kernels):  # noqa: F811
    fam = {n: k for n, k in kernels.items() if isa.family(n) == "gemv_mxfp8_kernel"}
    got = set()
    for n, k in fam.items():
        m = re.search(r"gemv_mxfp8_kernelILi(\d+)ELi(\d+)ELi(\d+)ELb(\d)ELi(\d)EE", n)
        assert m, n
        got.add(tuple(int(x) for x in m.groups()))
        assert k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0 and k["private_segment_fixed_size"] == 0, (n, k)
        assert k["max_flat_workgroup_size"] == 256 and k["group_segment_fixed_size"] == 0, (n, k)     # launch bounds 256; LDS is dynamic
    assert got == shipped(), (sorted(got - shipped()), sorted(shipped() - got))
    assert not any("gemv_kernelI" in n for n in fam)      # the bf16 kernel's scans match by that substring


def test_register_ceilings_of_the_decode_shapes(hip_lib, kernels):  # noqa: F811
    """Not above the bf16 instantiation with as many loads in flight (tests/test_decode_prologue_waits_cpu.py test_matvec_register_count):
    127 up to 8 loads, 166 gate+up / 170 otherwise at 16."""
    vg = {}
    for n, k in kernels.items():
        m = re.search(r"gemv_mxfp8_kernelILi(\d+)ELi(\d+)ELi(\d+)ELb(\d)ELi(\d)EE", n)
        if m:
            vg[tuple(int(x) for x in m.groups())] = k["vgpr_count"]
    for name, n, k, e, nm in DECODE_SHAPES:
        r, u, _, form = plan(hip_lib, n, k, e, nm)
        loads = r * u * (2 if e == SILU_MUL else 1)
        assert loads <= 16, name
        ceiling = 127 if loads <= 8 else 166 if e == SILU_MUL else 170
        assert vg[(r, u, e, int(form != 0), max(form - 1, 0))] <= ceiling, (name, r, u, form, vg[(r, u, e, int(form != 0), max(form - 1, 0))])


def test_leading_arguments_are_preloaded(preload_kernels):  # noqa: F811
    """q, scales, x, norm_w, y, the residual vector, N and K: 14 dwords in user SGPRs at wave launch, as the bf16 matvec's."""
    fam = {n: k for n, k in preload_kernels.items() if "gemv_mxfp8_kernel" in n}
    assert len(fam) == len(shipped())
    assert all(k["kernarg_preload_length"] >= 14 for k in fam.values()), {n: k["kernarg_preload_length"] for n, k in fam.items() if k["kernarg_preload_length"] < 14}


@pytest.fixture(scope="module")
def straight_line_text(tmp_path_factory):
    """{(R, U, EPI, PRO): program text} of the straight-line instantiations, extracted as tests/test_decode_prologue_waits_cpu.py does."""
    if not (os.path.exists(f"{LLVM}/llvm-objdump") and os.path.exists(f"{LLVM}/llvm-readelf")):
        pytest.skip("ROCm llvm tools not found")
    from aha_amd import build
    build.build()
    d = tmp_path_factory.mktemp("codeobj_fp8")
    shutil.copy(os.path.join(ROOT, "aha_amd", "csrc", "libaha_hip.so"), d / "lib.so")
    subprocess.run([f"{LLVM}/llvm-objdump", "--offloading", "lib.so"], cwd=d, capture_output=True, check=True)
    out = {}
    for o in sorted(glob.glob(str(d / "lib.so.*gfx950"))):
        notes = subprocess.run([f"{LLVM}/llvm-readelf", "--notes", o], capture_output=True, text=True, check=True).stdout
        if "gemv_mxfp8_kernel" not in notes:
            continue
        dis = subprocess.run([f"{LLVM}/llvm-objdump", "-d", "--no-show-raw-insn", o], capture_output=True, text=True, check=True).stdout
        cur = None
        for line in dis.splitlines():
            m = re.match(r"^[0-9a-f]+ <(\S+)>:", line)
            if m:
                k = re.search(r"gemv_mxfp8_kernelILi(\d+)ELi(\d+)ELi(\d+)ELb1ELi([12])EE", m.group(1))
                cur = tuple(int(x) for x in k.groups()) if k else None
                if cur:
                    assert cur not in out, cur
                    out[cur] = []
                continue
            t = line.strip().split("//")[0].strip()
            if cur and t:
                out[cur].append(t)
    return out


def is_nt_load(t):
    return t.startswith("global_load_") and t.split()[-1] == "nt"


def test_every_straight_line_prologue_runs_under_the_first_request(straight_line_text):
    want = {(r, u, e, pro) for (r, u, e, fast, pro) in shipped() if pro}
    assert set(straight_line_text) == want
    for (r, u, e, pro), text in sorted(straight_line_text.items()):
        loads = r * u * (2 if e == SILU_MUL else 1)
        first = next(i for i, t in enumerate(text) if is_nt_load(t))
        ends = [i for i, t in enumerate(text) if t.startswith("s_barrier") and i > first]
        end = ends[(2 if pro == 2 else 1) - 1]          # the RMSNorm's reduction adds a barrier
        issued, seen, kinds = 0, [], {}
        for i in range(first, end):
            t = text[i]
            if is_nt_load(t):
                issued += 1
                kinds[t.split()[0]] = kinds.get(t.split()[0], 0) + 1
            if t.startswith("s_cbranch") or t.startswith("s_branch"):
                assert int(t.split()[1]) < 0x8000, f"backward branch in the prologue of {(r, u, e, pro)}: {t}"
            m = re.search(r"vmcnt\((\d+)\)", t) if t.startswith("s_waitcnt") else None
            if m:
                seen.append(int(m.group(1)))
                assert int(m.group(1)) >= issued, f"{(r, u, e, pro)}: `{t}` with {issued} nt loads issued: the wait drains the first request"
        # the whole first request and only it: 8-byte weight loads and as many scale bytes
        assert kinds == {"global_load_dwordx2": loads, "global_load_ubyte": loads}, ((r, u, e, pro), kinds)
        assert seen, f"{(r, u, e, pro)}: no wait at all in front of the barrier: the scan does not see the staging"
        assert [n for i, n in vm_waits(text) if i < first] == [], f"{(r, u, e, pro)}: a vector-memory wait in front of the first weight request"
        # what the conversion compiles to: the scale folded in by the hardware, the high half by op_sel
        assert any(t.startswith("v_cvt_scalef32_pk_f32_fp8") for t in text) and any(t.startswith("v_cvt_scalef32_pk_f32_fp8") and "op_sel:[1,0,0]" in t for t in text)


# ---- 4. one lane's arithmetic ---------------------------------------------------------------------------------------------------------
def e4m3_f32(b):
    """OCP e4m3fn bytes -> f32, written out: sign, 4 exponent bits (bias 7), 3 mantissa bits, subnormals man * 2^-9."""
    b = np.asarray(b, dtype=np.uint32)
    ex, man = (b >> 3) & 0xf, b & 7
    mag = np.where(ex == 0, man.astype(np.float32) * np.float32(2.0 ** -9),
                   ((ex + 120) << 23 | man << 20).astype(np.uint32).view(np.float32))
    return np.where(b & 0x80, -mag, mag).astype(np.float32)


def lane_operands(q8, scale_byte):
    """What consume() hands to its fmas: the 8 bytes times 2^(scale - 127) in f32 (v_cvt_scalef32_pk_f32_fp8: exact)."""
    sf = np.array([int(scale_byte) << 23], dtype=np.uint32).view(np.float32)[0]
    with np.errstate(under="raise", over="raise"):
        return (e4m3_f32(q8) * sf).astype(np.float32)


def fma_chain(x8, w8, acc=np.float32(0)):
    s = np.float64(acc)
    for a, b in zip(x8, w8):
        s = np.float64(np.float32(np.float64(a) * np.float64(b) + s))      # the product of two f32 is exact in f64
    return np.float32(s)


def test_lane_arithmetic_equals_the_bf16_kernel_operands_bit_for_bit():
    from aha_amd import quant
    W = edge_matrix()
    q, s, wr = quant.quantize_mxfp8(W)
    want = (bf16_bits(wr).numpy().astype(np.uint16).astype(np.uint32) << 16)          # lo_bf / hi_bf of W'
    qn, sn = q.numpy(), s.numpy()
    g = np.random.default_rng(1)
    x = g.standard_normal(W.shape[1]).astype(np.float32)
    seen_sub = seen_neg0 = 0
    for row in range(W.shape[0]):
        for k0 in range(0, W.shape[1], 8):                # a lane's 8 k of one chunk: inside one MX block
            ops8 = lane_operands(qn[row, k0:k0 + 8], sn[row, k0 // 32])
            assert np.array_equal(ops8.view(np.uint32), want[row, k0:k0 + 8]), (row, k0)
            a = fma_chain(x[k0:k0 + 8], ops8)
            b = fma_chain(x[k0:k0 + 8], want[row, k0:k0 + 8].view(np.float32))
            assert a.view(np.uint32) == b.view(np.uint32)
            seen_sub += int(((qn[row, k0:k0 + 8] & 0x78) == 0).sum() and ((qn[row, k0:k0 + 8] & 0x7f) != 0).sum())
            seen_neg0 += int((qn[row, k0:k0 + 8] == 0x80).sum())
    assert seen_sub > 0 and seen_neg0 >= 2 and int(sn.min()) == 10          # subnormal codes, -0, the smallest block exponent
    # every code (but the two NaNs) at the smallest, the middle and the largest block exponent, against the reference dequantiser
    # (at e = 120 a finite bf16 weight gives |q| <= 240 = code 0x77: 256 * 2^120 is past bf16, and the quantiser refuses such a matrix)
    for sb in (10, 127, 247):
        codes = np.array([c for c in range(256) if c & 0x7f != 0x7f and (sb < 247 or c & 0x7f <= 0x77)], dtype=np.uint8)
        qq = torch.from_numpy(np.resize(codes, 256).reshape(1, 256).copy())
        ss = torch.full((1, 8), sb, dtype=torch.uint8)
        ref = bf16_bits(quant.dequantize_mxfp8(qq, ss)).numpy().astype(np.uint16).astype(np.uint32) << 16
        got = lane_operands(qq.numpy()[0], sb)
        assert np.array_equal(got.view(np.uint32), ref[0]), sb
        assert np.isfinite(got).all() and (np.abs(got[got != 0]) >= np.float32(2.0 ** -126)).all()   # never an f32 subnormal
    assert lane_operands(np.array([0x00, 0x80], dtype=np.uint8), 10).view(np.uint32).tolist() == [0, 0x80000000]
