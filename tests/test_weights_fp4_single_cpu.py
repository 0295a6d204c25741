"""CPU tier: single-sequence decode from MXFP4 weights (gemv_mxfp4_kernel, aha_amd/csrc/kernels_gemv_fp4.hip), the twin of
tests/test_weights_fp8_single_cpu.py, whose helpers it uses.

  * the op entry aha_hip_gemv_mxfp4, the switch aha_hip_debug_fp4_single and the plan query aha_hip_debug_plan_gemv_mxfp4 in every layer
    of the ABI, with their GPU-free argument checks;
  * the kernel's instantiations in the shipped gfx950 code object: the set the launcher can reach and no other, no scratch, at most 170
    VGPRs on the decode shapes (three blocks of four waves per CU), and -- for every straight-line instantiation -- the prologue under
    the first request: R * U * NW dword loads and as many scale bytes, all in flight at every wait in front of the prologue's barrier;
  * one lane's arithmetic restated in numpy: 4 bytes of E2M1 codes and their block's scale byte give, in f32, bit for bit the values the
    bf16 kernel reads from W' = the reference quantiser's dequantised matrix, -0.0 for the code 0x8 included.
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
import test_isa_cpu as isa  # noqa: E402
from test_isa_cpu import kernels  # noqa: E402,F401
from test_decode_prologue_waits_cpu import LLVM, vm_waits  # noqa: E402
from test_decode_preload_cpu import kernels as preload_kernels  # noqa: E402,F401  (its fixture, under another name)
from test_weights_fp4_cpu import bf16_bits, edge_matrix  # noqa: E402
import test_weights_fp8_single_cpu as fp8  # noqa: E402
from test_weights_fp8_single_cpu import DECODE_SHAPES, fma_chain, is_nt_load  # noqa: E402

STORE, RESIDUAL, SILU_MUL, LOGITS = 0, 1, 2, 3
NAME = r"gemv_mxfp4_kernelILi(\d+)ELi(\d+)ELi(\d+)ELb(\d)ELi(\d)EE"


def shipped():
    """{(R, U, EPI, FAST, PRO)}: the direct form keeps the FP8 plan's 16 loads per buffer, so the launcher reaches the same set."""
    return fp8.shipped()


def plan(lib, N, K, epi, norm):
    r, u, g, f = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int32()
    assert lib.aha_hip_debug_plan_gemv_mxfp4(N, K, epi, int(norm), C.byref(r), C.byref(u), C.byref(g), C.byref(f), None) == 0
    return r.value, u.value, g.value, f.value


# ---- 1. every layer of the ABI --------------------------------------------------------------------------------------------------------
def test_single_sequence_fp4_entries_in_every_layer(hip_lib):
    from aha_amd import _lib, model, ops
    import test_host_cpu
    header = open(os.path.join(ROOT, "include", "aha_hip.h")).read()
    assert re.search(r"int aha_hip_gemv_mxfp4\(const void\* q, const uint32_t\* scales, const void\* x, void\* y, int32_t N, int32_t K, int32_t epi, "
                     r"const void\* norm_w,\s+float eps, const void\* residual, float\* logits, uint32_t\* argmax_out, void\* stream\);", header)
    assert re.search(r"int aha_hip_debug_fp4_single\(aha_model\* m, int on\);", header)
    assert re.search(r"int aha_hip_debug_plan_gemv_mxfp4\(int32_t N, int32_t K, int32_t epi, int32_t has_norm, int32_t\* R, int32_t\* U, "
                     r"int32_t\* grid, int32_t\* form,\s+int32_t\* by_plan\);", header)
    raw = C.CDLL(_lib.LIB_PATH)
    for name, nargs in (("aha_hip_gemv_mxfp4", 13), ("aha_hip_debug_fp4_single", 2), ("aha_hip_debug_plan_gemv_mxfp4", 9)):
        assert hasattr(raw, name), name
        assert len(_lib.SIGNATURES[name][1]) == nargs, name
    # the same signatures as the FP8 entries
    for a, b in (("aha_hip_gemv_mxfp4", "aha_hip_gemv_mxfp8"), ("aha_hip_debug_fp4_single", "aha_hip_debug_fp8_single"),
                 ("aha_hip_debug_plan_gemv_mxfp4", "aha_hip_debug_plan_gemv_mxfp8")):
        assert _lib.SIGNATURES[a] == _lib.SIGNATURES[b], a
    # declared == exported == bound, still
    assert set(_lib.SIGNATURES) == set(test_host_cpu._declared_symbols())
    assert callable(ops.gemv_mxfp4) and callable(ops.plan_gemv_mxfp4) and callable(ops.gemv_mxfp4_by_plan)
    assert callable(model.HipInferenceModel.debug_fp4_single)
    src = open(os.path.join(ROOT, "rust", "aha-hip", "src", "lib.rs")).read()
    ext = src[src.index('extern "C" {'):]
    ext = ext[:ext.index("\n    }\n")]
    assert re.search(r"pub fn aha_hip_debug_fp4_single\(m: \*mut AhaModel, on: i32\) -> i32;", ext)
    assert re.search(r"pub fn aha_hip_gemv_mxfp4\(\s+q: \*const std::ffi::c_void,\s+scales: \*const u32,", ext)
    assert re.search(r"pub fn aha_hip_debug_plan_gemv_mxfp4\(", ext)
    assert re.search(r"pub fn debug_fp4_single\(&mut self, on: i32\) -> Result<\(\), Error> \{\s+check\(unsafe \{ sys::aha_hip_debug_fp4_single\(self\.model, on\) \}\)", src)
    assert "launch_gemv_mxfp4" in open(os.path.join(ROOT, "aha_amd", "csrc", "kernels.h")).read()
    # nothing of the feature reads the environment
    for f in ("kernels_gemv_fp4.hip", "kernels_gemv_fp8.hip", "gemv_fp8_body.h", "gemv_fp8_launch.h"):
        assert "getenv" not in open(os.path.join(ROOT, "aha_amd", "csrc", f)).read(), f
    # built like the FP8 matvec
    from aha_amd import build
    assert "kernels_gemv_fp4.hip" in build.SOURCES and build.FLAGS_LIKE["kernels_gemv_fp4.hip"] == build.FLAGS_LIKE["kernels_gemv_fp8.hip"]


def test_single_sequence_fp4_argument_checks_need_no_gpu(hip_lib):
    err = hip_lib.aha_hip_last_error
    buf = (C.c_uint8 * 4096)()
    p = C.addressof(buf)
    f = C.c_float(1e-6)
    g = hip_lib.aha_hip_gemv_mxfp4
    assert hip_lib.aha_hip_debug_fp4_single(None, 1) == -1 and b"debug_fp4_single: null model" in err()
    assert g(p, p, p, p, 32, 40, 0, None, f, None, None, None, None) == -1 and b"gemv_mxfp4: K must be a positive multiple of 32" in err()
    assert g(p, p, p, p, 32, 0, 0, None, f, None, None, None, None) == -1 and b"gemv_mxfp4: K must be a positive multiple of 32" in err()
    assert g(p, p, p, p, 32, 32800, 0, None, f, None, None, None, None) == -1 and b"gemv_mxfp4: K must be at most 32768" in err()
    assert g(p, None, p, p, 32, 64, 0, None, f, None, None, None, None) == -1 and b"gemv_mxfp4: null scales" in err()
    assert g(None, p, p, p, 32, 64, 0, None, f, None, None, None, None) == -1 and b"gemv_mxfp4: null matrix or x" in err()
    assert g(p, p, None, p, 32, 64, 0, None, f, None, None, None, None) == -1 and b"gemv_mxfp4: null matrix or x" in err()
    assert g(p, p, p, None, 32, 64, 0, None, f, None, None, None, None) == -1 and b"gemv_mxfp4: null y" in err()
    assert g(p, p, p, p, 32, 64, 1, None, f, None, None, None, None) == -1 and b"gemv_mxfp4: epi 1 needs a residual" in err()
    assert g(p, p, p, p, 48, 64, 2, None, f, None, None, None, None) == -1 and b"gemv_mxfp4: epi 2 needs N % 32 == 0" in err()
    assert g(p, p, p, None, 32, 64, 3, None, f, None, None, None, None) == -1 and b"gemv_mxfp4: epi 3 needs logits and argmax_out" in err()
    assert g(p, p, p, p, 32, 64, 3, None, f, None, p, None, None) == -1 and b"gemv_mxfp4: epi 3 needs logits and argmax_out" in err()
    assert g(p, p, p, p, 32, 64, 4, None, f, None, None, None, None) == -1 and b"gemv_mxfp4: epi must be 0..3" in err()
    assert g(p, p, p, p, 32, 64, -1, None, f, None, None, None, None) == -1 and b"gemv_mxfp4: epi must be 0..3" in err()
    r = C.c_int32()
    assert hip_lib.aha_hip_debug_plan_gemv_mxfp4(64, 40, 0, 0, C.byref(r), C.byref(r), C.byref(r), None, None) == -1 and b"debug_plan_gemv_mxfp4" in err()
    assert hip_lib.aha_hip_debug_plan_gemv_mxfp4(64, 64, 0, 0, None, C.byref(r), C.byref(r), None, None) == -1 and b"debug_plan_gemv_mxfp4" in err()
    assert hip_lib.aha_hip_debug_plan_gemv_mxfp4(48, 64, 2, 0, C.byref(r), C.byref(r), C.byref(r), None, None) == -1


# ---- 2. the plan ----------------------------------------------------------------------------------------------------------------------
def by_plan_in_profile():
    """The decision section of profiles/weights_fp4_single.md: its line `by plan: name, name, ...` (or `by plan: none`) over DECODE_SHAPES."""
    text = open(os.path.join(ROOT, "profiles", "weights_fp4_single.md")).read()
    m = re.search(r"^## Decision\n(.*?)(?=^## |\Z)", text, re.S | re.M)
    assert m, "profiles/weights_fp4_single.md has no Decision section"
    line = re.search(r"^by plan: (.*)$", m.group(1), re.M)
    assert line, "the Decision section names no `by plan:` list"
    names = [n.strip() for n in line.group(1).split(",")]
    names = [] if names == ["none"] else names
    known = [n for n, *_ in DECODE_SHAPES]
    assert all(n in known for n in names), names
    return [n in names for n in known]


def test_plan_names_a_shipped_instantiation_and_a_grid_within_the_tiles(hip_lib):
    from aha_amd import ops
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
        assert (r, u, grid, form) == ops.plan_gemv_mxfp4(n, k, e, nm)
        rows = n // 2 if e == SILU_MUL else n
        assert (r, u, e, int(form != 0), max(form - 1, 0)) in have, (n, k, e, nm, r, u, form)
        assert 1 <= grid <= min(768, -(-rows // (4 * r))), (n, k, e, grid)       # no block without a tile: the first request is unconditional
        assert u & (u - 1) == 0 and (r == 1 or -(-rows // (4 * r)) >= 512)       # at least 512 tiles unless one row per wave already
        assert (form != 0) == (k % (512 * u) == 0)
        assert (form >= 2) == (form != 0 and k <= (8192 if nm else 16384)) and (form == 3) == (form >= 2 and nm)
        # never by plan: a matrix of at most 1024 x 512 (the suite's small models decode on bf16 unless the switch is 2)
        if n * k <= 1024 * 512:
            assert not ops.gemv_mxfp4_by_plan(n, k, e), (n, k, e)
    for n in (32, 512, 1024):
        for k in (32, 256, 512):
            assert not any(ops.gemv_mxfp4_by_plan(n, k, e) for e in (STORE, RESIDUAL, SILU_MUL, LOGITS)), (n, k)
    # which matrices a model's step takes from the copies: what profiles/weights_fp4_single.md decided from its measurements
    assert [ops.gemv_mxfp4_by_plan(n, k, e) for _, n, k, e, _ in DECODE_SHAPES] == by_plan_in_profile()
    # an unmeasured general-form shape stays on bf16 whatever its size
    assert not ops.gemv_mxfp4_by_plan(4096, 9728, RESIDUAL) and not ops.gemv_mxfp4_by_plan(16416, 1056, LOGITS)


# ---- 3. the code object ---------------------------------------------------------------------------------------------------------------
def test_instantiations_in_the_code_object(kernels):  # noqa: F811
    fam = {n: k for n, k in kernels.items() if "gemv_mxfp4_kernel" in n}
    got = set()
    for n, k in fam.items():
        m = re.search(NAME, n)
        assert m, n
        got.add(tuple(int(x) for x in m.groups()))
        assert isa.family(n) == "gemv_mxfp4_kernel", n
        assert k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0 and k["private_segment_fixed_size"] == 0, (n, k)
        assert k["max_flat_workgroup_size"] == 256 and k["group_segment_fixed_size"] == 0, (n, k)     # launch bounds 256; LDS is dynamic
    assert got == shipped() and len(fam) == len(got), (sorted(got - shipped()), sorted(shipped() - got))
    # the other matvecs' scans match by these substrings
    assert not any("gemv_kernelI" in n or "gemv_mxfp8_kernel" in n for n in fam)


def test_register_ceiling_of_the_decode_shapes(hip_lib, kernels):  # noqa: F811
    """The plan runs 3 blocks of 4 waves per CU: at most 170 VGPRs on every instantiation a decode shape selects."""
    vg = {}
    for n, k in kernels.items():
        m = re.search(NAME, n)
        if m:
            vg[tuple(int(x) for x in m.groups())] = k["vgpr_count"]
    for name, n, k, e, nm in DECODE_SHAPES:
        r, u, _, form = plan(hip_lib, n, k, e, nm)
        assert r * u * (2 if e == SILU_MUL else 1) <= 16, name
        key = (r, u, e, int(form != 0), max(form - 1, 0))
        assert vg[key] <= 170, (name, key, vg[key])


def test_leading_arguments_are_preloaded(preload_kernels):  # noqa: F811
    """q, scales, x, norm_w, y, the residual vector, N and K: 14 dwords in user SGPRs at wave launch, as the FP8 matvec's."""
    fam = {n: k for n, k in preload_kernels.items() if "gemv_mxfp4_kernel" in n}
    assert len(fam) == len(shipped())
    assert all(k["kernarg_preload_length"] >= 14 for k in fam.values()), {n: k["kernarg_preload_length"] for n, k in fam.items() if k["kernarg_preload_length"] < 14}


@pytest.fixture(scope="module")
def straight_line_text(tmp_path_factory):
    """{(R, U, EPI, PRO): program text} of the straight-line instantiations, extracted as tests/test_weights_fp8_single_cpu.py does."""
    if not (os.path.exists(f"{LLVM}/llvm-objdump") and os.path.exists(f"{LLVM}/llvm-readelf")):
        pytest.skip("ROCm llvm tools not found")
    from aha_amd import build
    build.build()
    d = tmp_path_factory.mktemp("codeobj_fp4")
    shutil.copy(os.path.join(ROOT, "aha_amd", "csrc", "libaha_hip.so"), d / "lib.so")
    subprocess.run([f"{LLVM}/llvm-objdump", "--offloading", "lib.so"], cwd=d, capture_output=True, check=True)
    out = {}
    for o in sorted(glob.glob(str(d / "lib.so.*gfx950"))):
        notes = subprocess.run([f"{LLVM}/llvm-readelf", "--notes", o], capture_output=True, text=True, check=True).stdout
        if "gemv_mxfp4_kernel" not in notes:
            continue
        dis = subprocess.run([f"{LLVM}/llvm-objdump", "-d", "--no-show-raw-insn", o], capture_output=True, text=True, check=True).stdout
        cur = None
        for line in dis.splitlines():
            m = re.match(r"^[0-9a-f]+ <(\S+)>:", line)
            if m:
                k = re.search(r"gemv_mxfp4_kernelILi(\d+)ELi(\d+)ELi(\d+)ELb1ELi([12])EE", m.group(1))
                cur = tuple(int(x) for x in k.groups()) if k else None
                if cur:
                    assert cur not in out, cur
                    out[cur] = []
                continue
            t = line.strip().split("//")[0].strip()
            if cur and t:
                out[cur].append(t)
    return out


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
        # the whole first request and only it: one dword of 8 codes per (row, chunk) and as many scale bytes
        assert kinds == {"global_load_dword": loads, "global_load_ubyte": loads}, ((r, u, e, pro), kinds)
        assert seen, f"{(r, u, e, pro)}: no wait at all in front of the barrier: the scan does not see the staging"
        assert [n for i, n in vm_waits(text) if i < first] == [], f"{(r, u, e, pro)}: a vector-memory wait in front of the first weight request"
        # what the conversion compiles to: the scale folded in by the hardware, bytes 1..3 of the dword by op_sel
        cvt = [t for t in text if t.startswith("v_cvt_scalef32_pk_f32_fp4")]
        assert any("op_sel" not in t for t in cvt) and any("op_sel" in t for t in cvt), (r, u, e, pro)
        assert not any(t.startswith("v_cvt_scalef32_pk_f32_fp8") for t in text)


# ---- 4. one lane's arithmetic ---------------------------------------------------------------------------------------------------------
E2M1 = np.array([0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0], dtype=np.float32)


def lane_operands(q4, scale_byte):
    """What consume() hands to its fmas: the 8 codes of 4 bytes (the even k in bits 0..3) times 2^(scale - 127) in f32
    (v_cvt_scalef32_pk_f32_fp4 on bytes 0..3: exact, the sign kept on a zero)."""
    q4 = np.asarray(q4, dtype=np.uint8)
    assert q4.shape == (4,)
    codes = np.stack((q4 & 0xf, q4 >> 4), axis=-1).reshape(8)
    sf = np.array([int(scale_byte) << 23], dtype=np.uint32).view(np.float32)[0]
    with np.errstate(under="raise", over="raise"):
        mag = (E2M1[codes & 7] * sf).astype(np.float32)
    return np.where(codes & 8, -mag, mag).astype(np.float32)


def test_lane_arithmetic_equals_the_bf16_kernel_operands_bit_for_bit():
    from aha_amd import quant
    W = edge_matrix()
    q, s, wr = quant.quantize_mxfp4(W)
    want = (bf16_bits(wr).numpy().astype(np.uint16).astype(np.uint32) << 16)          # lo_bf / hi_bf of W'
    qn, sn = q.numpy(), s.numpy()
    g = np.random.default_rng(1)
    x = g.standard_normal(W.shape[1]).astype(np.float32)
    seen_neg0 = 0
    for row in range(W.shape[0]):
        for k0 in range(0, W.shape[1], 8):                # a lane's 8 k of one chunk: 4 bytes inside one MX block
            ops8 = lane_operands(qn[row, k0 // 2:k0 // 2 + 4], sn[row, k0 // 32])
            assert np.array_equal(ops8.view(np.uint32), want[row, k0:k0 + 8]), (row, k0)
            a = fma_chain(x[k0:k0 + 8], ops8)
            b = fma_chain(x[k0:k0 + 8], want[row, k0:k0 + 8].view(np.float32))
            assert a.view(np.uint32) == b.view(np.uint32)
            seen_neg0 += int((ops8.view(np.uint32) == 0x80000000).sum())
            assert np.isfinite(ops8).all() and (np.abs(ops8[ops8 != 0]) >= np.float32(2.0 ** -126)).all()     # never an f32 subnormal
    assert seen_neg0 >= 1                                  # the matrix holds the code 0x8
    # all 16 codes at the smallest, the middle and the largest block exponent, against the reference dequantiser
    for sb in (2, 127, 252):
        qq = torch.from_numpy(np.resize(np.array([lo | hi << 4 for lo, hi in zip(range(0, 16, 2), range(1, 16, 2))], dtype=np.uint8), 16).reshape(1, 16).copy())
        ss = torch.full((1, 1), sb, dtype=torch.uint8)
        ref = bf16_bits(quant.dequantize_mxfp4(qq, ss)).numpy().astype(np.uint16).astype(np.uint32) << 16
        got = np.concatenate([lane_operands(qq.numpy()[0, i:i + 4], sb) for i in range(0, 16, 4)])
        assert sorted(set(quant.unpack_nibbles(qq)[0, :16].tolist())) == list(range(16))
        assert np.array_equal(got.view(np.uint32), ref[0]), sb
        assert np.isfinite(got).all() and (np.abs(got[got != 0]) >= np.float32(2.0 ** -126)).all()
    # +0 / -0
    for sb in (2, 127, 252):
        assert lane_operands(np.array([0x80, 0x08, 0x00, 0x88], dtype=np.uint8), sb).view(np.uint32).tolist() == \
            [0, 0x80000000, 0x80000000, 0, 0, 0, 0x80000000, 0x80000000]
