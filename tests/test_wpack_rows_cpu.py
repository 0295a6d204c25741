"""CPU tier: exception rows of the exact 13-bit weight copies (aha_amd/quant.py check_pk13_rows / pack_pk13_rows / unpack_pk13_rows,
gemv_kernel_rows_pk13 in aha_amd/csrc/kernels_gemv_pk13.hip).

  * the restatement: the rows found equal a brute-force scan; pack -> unpack is W everywhere but at the flagged weights, and W everywhere
    once the flagged rows are taken from W; 16 rows are accepted, 17 refused; Inf / NaN are refused;
  * the new entries in the header, the ctypes table and ops, and their argument checks, which need no GPU;
  * the twin kernel in the shipped gfx950 code object: every (R, EPI, PRO) the launcher can pick, under a name the plain kernel's scans
    do not match; no scratch, no spills; the plain kernel's register budget and at most 168 VGPRs on the R = 2 form (three waves per SIMD);
    the straight-line prologues leave the first buffer in flight exactly as tests/test_wpack_isa_cpu.py asks of the plain kernel; the
    loads of the exception rows (the only plain global 16-byte loads behind the prologue) sit behind the prologue's last barrier.
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
from test_decode_prologue_waits_cpu import LLVM, vm_waits  # noqa: E402
from test_wpack_cpu import SILU_MUL, bits_of, edge_weights, from_bits, shipped  # noqa: E402
from test_wpack_isa_cpu import is_nt_load  # noqa: E402

from aha_amd import quant  # noqa: E402

BELOW = 0x0d80          # 2^-100: finite, far below the window of weights of scale 0.02


def planted(N=40, K=8192, where=((0, 0), (7, 4097), (7, 8191), (39, 600)), seed=5):
    W = edge_weights(N, K, seed=seed)
    b = bits_of(W).copy()
    for i, (r, c) in enumerate(where):
        b[r, c] = BELOW | (0x8000 if i & 1 else 0)
    return from_bits(b)


# ---- 1. the restatement ---------------------------------------------------------------------------------------------------------------
def test_rows_found_equal_a_brute_force_scan():
    W = planted()
    bh, bad = quant.check_pk13(W)
    assert bad == 4
    b = bits_of(W)
    brute = [r for r in range(W.shape[0])
             if any((int(v) & 0x7f80) != 0x7f80 and ((int(v) >> 8) & 0x7f) != 0 and ((int(v) >> 8) & 0x7f) <= bh for v in b[r])]
    assert quant.check_pk13_rows(W) == (bh, 0, brute) and brute == [0, 7, 39]
    # a matrix inside the window: no rows, and the old check agrees
    W0 = edge_weights(4, 4096, seed=6)
    assert quant.check_pk13_rows(W0) == (quant.check_pk13(W0)[0], 0, [])


def test_pack_then_unpack_is_w_everywhere_but_at_the_flagged_weights():
    W = planted()
    bh, nonfinite, rows = quant.check_pk13_rows(W)
    P = quant.pack_pk13_rows(W, bh)
    assert P.shape == (40, 2, 6656) and P.dtype == torch.uint8
    got, want = bits_of(quant.unpack_pk13(P, bh)), bits_of(W)
    diff = {(int(r), int(c)) for r, c in np.argwhere(got != want)}
    assert diff == {(0, 0), (7, 4097), (7, 8191), (39, 600)}
    # what the matvec computes with: the flagged rows from W
    assert np.array_equal(bits_of(quant.unpack_pk13_rows(P, bh, W, rows)), want)
    # outside the flagged weights the bytes are pack_pk13's own: a unit without one is untouched
    Pold = quant.pack_pk13(W, bh)
    same = torch.ones(40, 2, dtype=torch.bool)
    for r, c in diff:
        same[r, c // 4096] = False
    assert torch.equal(P[same], Pold[same])


def test_sixteen_rows_are_accepted_and_seventeen_refused():
    assert quant.PK13_MAX_ROWS == 16
    where16 = tuple((2 * i + 1, 37 * i) for i in range(16))
    W = planted(40, 4096, where16)
    bh, nonfinite, rows = quant.check_pk13_rows(W)
    assert rows == [2 * i + 1 for i in range(16)] and quant.packable_pk13_rows(nonfinite, rows)
    W = planted(40, 4096, where16 + ((1, 4000), (3, 9)))          # more weights, the same rows
    assert quant.check_pk13_rows(W)[2] == rows and quant.packable_pk13_rows(0, rows)
    W = planted(40, 4096, where16 + ((38, 5),))
    bh, nonfinite, rows = quant.check_pk13_rows(W)
    assert len(rows) == 17 and nonfinite == 0 and not quant.packable_pk13_rows(nonfinite, rows)


def test_inf_and_nan_are_refused():
    for v in (0x7f80, 0xff80, 0x7fc0, 0xffff):
        W = planted(8, 4096, ((2, 2),))
        b = bits_of(W).copy()
        b[5, 100] = v
        bh, nonfinite, rows = quant.check_pk13_rows(from_bits(b))
        assert nonfinite == 1 and rows == [2] and not quant.packable_pk13_rows(nonfinite, rows)
        assert bh == quant.check_pk13(W)[0]          # a non-finite value does not move the base


# ---- 2. the entries ---------------------------------------------------------------------------------------------------------------------
def test_entries_in_every_layer_and_argument_checks_need_no_gpu(hip_lib):
    from aha_amd import _lib, ops
    import test_host_cpu
    header = open(os.path.join(ROOT, "include", "aha_hip.h")).read()
    for decl in (r"int aha_hip_pack_pk13_rows\(const void\* W, int32_t N, int32_t K, void\* out, int32_t\* bh_out, int32_t\* rows_out, int32_t cap, "
                 r"int32_t\* nrows_out,\s+int64_t\* below_out, int64_t\* nonfinite_out, void\* stream\);",
                 r"int aha_hip_gemv_pk13_rows\(const void\* packed, int32_t bh, const void\* W, const int32_t\* rows, int32_t nrows, const void\* x,",
                 # the old entries keep their contracts
                 r"int aha_hip_pack_pk13\(const void\* W, int32_t N, int32_t K, void\* out, int32_t\* bh_out, int64_t\* bad_out, void\* stream\);",
                 r"int aha_hip_gemv_pk13\(const void\* packed, int32_t bh, const void\* x,"):
        assert re.search(decl, header), decl
    raw = C.CDLL(_lib.LIB_PATH)
    for name, nargs in (("aha_hip_pack_pk13_rows", 11), ("aha_hip_gemv_pk13_rows", 16), ("aha_hip_pack_pk13", 7), ("aha_hip_gemv_pk13", 13)):
        assert hasattr(raw, name) and len(_lib.SIGNATURES[name][1]) == nargs, name
    assert set(_lib.SIGNATURES) == set(test_host_cpu._declared_symbols())
    assert all(callable(f) for f in (ops.pack_pk13_rows, ops.gemv_pk13_rows, quant.check_pk13_rows, quant.pack_pk13_rows, quant.unpack_pk13_rows))
    err = hip_lib.aha_hip_last_error
    buf = (C.c_uint8 * 4096)()
    p = C.addressof(buf)
    f = C.c_float(1e-6)
    bh, n, below, nonf = C.c_int32(), C.c_int32(), C.c_int64(), C.c_int64()
    rows = (C.c_int32 * 16)(*range(16))
    pack = hip_lib.aha_hip_pack_pk13_rows
    assert pack(p, 4, 2048, p, C.byref(bh), rows, 16, C.byref(n), C.byref(below), C.byref(nonf), None) == -1 and b"pack_pk13_rows" in err()
    assert pack(p, 4, 4096, p, C.byref(bh), rows, 17, C.byref(n), C.byref(below), C.byref(nonf), None) == -1 and b"cap 0..16" in err()
    assert pack(None, 4, 4096, p, C.byref(bh), rows, 16, C.byref(n), C.byref(below), C.byref(nonf), None) == -1 and b"pack_pk13_rows" in err()
    gemv = hip_lib.aha_hip_gemv_pk13_rows
    assert gemv(p, 40, p, rows, 1, p, p, 32, 4104, 0, None, f, None, None, None, None) == -1 and b"gemv_pk13_rows: K must be a multiple of 4096" in err()
    assert gemv(p, 113, p, rows, 1, p, p, 32, 4096, 0, None, f, None, None, None, None) == -1 and b"bh must be 0..112" in err()
    assert gemv(p, 40, p, rows, 17, p, p, 32, 4096, 0, None, f, None, None, None, None) == -1 and b"nrows must be 0..16" in err()
    assert gemv(p, 40, None, rows, 1, p, p, 32, 4096, 0, None, f, None, None, None, None) == -1 and b"rows need W" in err()
    assert gemv(p, 40, p, None, 1, p, p, 32, 4096, 0, None, f, None, None, None, None) == -1 and b"rows need W" in err()
    rows[3] = 32
    assert gemv(p, 40, p, rows, 4, p, p, 32, 4096, 0, None, f, None, None, None, None) == -1 and b"row 32 is not a row of the matrix" in err()
    rows[3] = -1
    assert gemv(p, 40, p, rows, 4, p, p, 32, 4096, 0, None, f, None, None, None, None) == -1 and b"not a row of the matrix" in err()
    assert gemv(p, 40, p, rows, 1, p, p, 32, 4096, 1, None, f, None, None, None, None) == -1 and b"needs a residual" in err()
    for fn in ("kernels_gemv_pk13.hip", "gemv_pk13_body.h"):
        assert "getenv" not in open(os.path.join(ROOT, "aha_amd", "csrc", fn)).read(), fn


# ---- 3. the code object ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def twins(tmp_path_factory):
    """{(R, EPI, PRO): (name, metadata, program text, {addr, target: per instruction index})} of gemv_kernel_rows_pk13, and the same of
    the plain gemv_kernel_pk13."""
    if not (os.path.exists(f"{LLVM}/llvm-objdump") and os.path.exists(f"{LLVM}/llvm-readelf")):
        pytest.skip("ROCm llvm tools not found")
    from aha_amd import build
    build.build()
    d = tmp_path_factory.mktemp("codeobj_pk13_rows")
    shutil.copy(os.path.join(ROOT, "aha_amd", "csrc", "libaha_hip.so"), d / "lib.so")
    subprocess.run([f"{LLVM}/llvm-objdump", "--offloading", "lib.so"], cwd=d, capture_output=True, check=True)
    out = {"twin": {}, "plain": {}}
    for o in sorted(glob.glob(str(d / "lib.so.*gfx950"))):
        notes = subprocess.run([f"{LLVM}/llvm-readelf", "--notes", o], capture_output=True, text=True, check=True).stdout
        if "gemv_kernel_rows_pk13" not in notes:
            continue
        meta = {}
        for item in re.split(r"\n  - ", notes[notes.index("amdhsa.kernels:"):])[1:]:
            name = re.search(r"^\s*\.name:\s+(\S+)", item, re.M)
            if name:
                meta[name.group(1)] = {k: int(v) for k, v in re.findall(
                    r"^\s{0,4}\.(vgpr_count|sgpr_count|vgpr_spill_count|sgpr_spill_count|private_segment_fixed_size|group_segment_fixed_size|max_flat_workgroup_size):\s+(\d+)\s*$",
                    item, re.M)}
        dis = subprocess.run([f"{LLVM}/llvm-objdump", "-d", "--no-show-raw-insn", o], capture_output=True, text=True, check=True).stdout
        cur = None
        for line in dis.splitlines():
            m = re.match(r"^[0-9a-f]+ <(\S+)>:", line)
            if m:
                cur = None
                for kind, pat in (("twin", r"gemv_kernel_rows_pk13ILi(\d+)ELi(\d+)ELi(\d)EE"), ("plain", r"gemv_kernel_pk13ILi(\d+)ELi(\d+)ELi(\d)EE")):
                    k = re.search(pat, m.group(1))
                    if k:
                        key = tuple(int(x) for x in k.groups())
                        assert key not in out[kind], (kind, key)
                        out[kind][key] = (m.group(1), meta[m.group(1)], [], {"addr": {}, "target": {}, "base": None})
                        cur = out[kind][key]
                continue
            t = line.strip().split("//")[0].strip()
            if cur is not None and t:
                a = re.search(r"// ([0-9A-F]+):", line)
                if a is None:          # padding behind the kernel
                    continue
                here = int(a.group(1), 16)
                if cur[3]["base"] is None:
                    cur[3]["base"] = here
                cur[3]["addr"][len(cur[2])] = here
                to = re.search(r"<[^>+]+\+0x([0-9a-f]+)>\s*$", line) if t.startswith("s_cbranch") or t.startswith("s_branch") else None
                if to:
                    cur[3]["target"][len(cur[2])] = cur[3]["base"] + int(to.group(1), 16)
                cur[2].append(t)
    return out


def test_every_instantiation_the_launcher_can_pick_is_there_under_a_name_of_its_own(twins):
    import test_isa_cpu as isa
    assert set(twins["twin"]) == shipped() == set(twins["plain"])
    for key, (name, meta, text, _) in twins["twin"].items():
        # the plain kernel's scans (tests/test_wpack_cpu.py, tests/test_wpack_isa_cpu.py) select by this substring and pattern
        assert "gemv_kernel_pk13" not in name and not re.search(r"gemv_kernel_pk13ILi\d+ELi\d+ELi\dEE", name), name
        # the matvec class of bench.py and scripts/pmc_summary.py; not the bf16 kernel's own scans
        assert isa.family(name) == "gemv_kernel" and "gemv_kernelI" not in name, name
        assert meta["max_flat_workgroup_size"] == 256 and meta["group_segment_fixed_size"] == 0, (key, meta)


def test_no_scratch_no_spills_and_the_plain_kernels_occupancy(twins):
    for key, (name, meta, text, _) in sorted(twins["twin"].items()):
        assert meta["vgpr_spill_count"] == 0 and meta["sgpr_spill_count"] == 0 and meta["private_segment_fixed_size"] == 0, (key, meta)
        assert not any(t.startswith("scratch_") or t.startswith("buffer_") or t.startswith("flat_load") for t in text), key
        assert meta["vgpr_count"] <= 170, (key, meta)          # the plain kernel's budget (tests/test_wpack_isa_cpu.py)
        if key[0] == 2:
            assert meta["vgpr_count"] <= 168, (key, meta)      # lm_head: three waves per SIMD, all 768 blocks resident
        # 512 VGPRs per SIMD lane in units of 8: the twin runs as many waves per SIMD as the plain kernel of the same form
        waves = lambda v: min(8, 512 // (-(-v // 8) * 8))      # noqa: E731
        assert waves(meta["vgpr_count"]) >= waves(twins["plain"][key][1]["vgpr_count"]), (key, meta, twins["plain"][key][1])
        assert meta["sgpr_count"] <= 102, (key, meta)          # the row list lives in SGPRs and they are not spilled to get there


def test_every_prologue_wait_leaves_the_first_buffer_in_flight(twins):
    """tests/test_wpack_isa_cpu.py's property on the twin's straight-line forms, and the exception rows' loads behind the prologue."""
    for (r, e, pro), (name, meta, text, _) in sorted(twins["twin"].items()):
        if pro == 0:
            continue
        loads = 7 * r * (2 if e == SILU_MUL else 1)
        first = next(i for i, t in enumerate(text) if is_nt_load(t))
        ends = [i for i, t in enumerate(text) if t.startswith("s_barrier") and i > first]
        end = ends[(2 if pro == 2 else 1) - 1]
        issued, seen, kinds = 0, [], {}
        for i in range(first, end):
            t = text[i]
            if is_nt_load(t):
                issued += 1
                kinds[t.split()[0]] = kinds.get(t.split()[0], 0) + 1
            assert not (t.startswith("global_load_") and not is_nt_load(t)), f"{(r, e, pro)}: `{t}` under the first request"
            if t.startswith("s_cbranch") or t.startswith("s_branch"):
                assert int(t.split()[1]) < 0x8000, f"backward branch in the prologue of {(r, e, pro)}: {t}"
            m = re.search(r"vmcnt\((\d+)\)", t) if t.startswith("s_waitcnt") else None
            if m:
                seen.append(int(m.group(1)))
                assert int(m.group(1)) >= issued, f"{(r, e, pro)}: `{t}` with {issued} nt loads issued: the wait drains the first request"
        assert kinds == {"global_load_dwordx4": loads // 7 * 6, "global_load_dwordx2": loads // 7}, ((r, e, pro), kinds)
        assert seen and min(seen) >= loads, f"{(r, e, pro)}: waits {seen} in front of the barrier"
        assert [n for i, n in vm_waits(text) if i < first] == [], f"{(r, e, pro)}: a vector-memory wait in front of the first weight request"
        # the exception rows: eight 16-byte loads of W per unit, cached (not nt), behind the prologue's last barrier and nowhere else
        plain_loads = [i for i, t in enumerate(text) if t.startswith("global_load_dwordx4") and not is_nt_load(t) and i > first]
        assert len(plain_loads) == 8 and min(plain_loads) > end, ((r, e, pro), plain_loads, end)


def steady_loop(text, where):
    """(first, last) instruction of the loop with the most non-temporal loads in it: the two refills and the two consumes."""
    addr = {a: i for i, a in where["addr"].items()}
    best = None
    for i, target in where["target"].items():
        if target < where["addr"][i]:          # a backward branch closes a loop
            j = addr[target]
            n = sum(is_nt_load(t) for t in text[j:i])
            if n and (best is None or (n, -(i - j)) > (best[0], -(best[2] - best[1]))):
                best = (n, j, i)
    return best


def test_the_steady_state_loop_waits_as_the_plain_kernel_does(twins):
    """The row-end check costs the steady state no counted wait: inside the loop that refills and consumes both buffers the twin's
    vector-memory waits take the plain kernel's counts and none of them drains the queue."""
    for key, (name, meta, text, where) in sorted(twins["twin"].items()):
        _, _, ptext, pwhere = twins["plain"][key]
        loads = 7 * key[0] * (2 if key[1] == SILU_MUL else 1)
        n, j, i = steady_loop(text, where)
        pn, pj, pi = steady_loop(ptext, pwhere)
        assert n == pn == 2 * loads, (key, n, pn)
        tw = [v for k, v in vm_waits(text) if j <= k < i]
        pw = [v for k, v in vm_waits(ptext) if pj <= k < pi]
        # the same counts (a count met twice in a row waits once), none below the refill in flight
        assert set(tw) == set(pw) and min(tw) == min(pw) >= loads and abs(len(tw) - len(pw)) <= 1, (key, tw, pw)
        # the exception rows' loads are not in it
        assert not any(t.startswith("global_load_dwordx4") and not is_nt_load(t) for t in text[j:i]), key
