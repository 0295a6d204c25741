"""CPU tier: the straight-line instantiations of gemv_kernel_pk13 (aha_amd/csrc/kernels_gemv_pk13.hip) in the shipped gfx950 code object.

For every PRO != 0 instantiation: the prologue runs under the first request -- every vector-memory wait between the first non-temporal load
and the barrier that ends the prologue is a counted one that leaves the buffer's 7 * R * NW weight loads in flight --, nothing touches
scratch, and the kernel stays within 170 VGPRs (12 waves per CU, as the bf16 matvec).
"""
import glob
import os
import re
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_decode_prologue_waits_cpu import LLVM, vm_waits  # noqa: E402
from test_wpack_cpu import SILU_MUL, shipped  # noqa: E402


@pytest.fixture(scope="module")
def straight_line(tmp_path_factory):
    """{(R, EPI, PRO): (metadata, program text)} of the straight-line instantiations."""
    if not (os.path.exists(f"{LLVM}/llvm-objdump") and os.path.exists(f"{LLVM}/llvm-readelf")):
        pytest.skip("ROCm llvm tools not found")
    from aha_amd import build
    build.build()
    d = tmp_path_factory.mktemp("codeobj_pk13")
    shutil.copy(os.path.join(ROOT, "aha_amd", "csrc", "libaha_hip.so"), d / "lib.so")
    subprocess.run([f"{LLVM}/llvm-objdump", "--offloading", "lib.so"], cwd=d, capture_output=True, check=True)
    out = {}
    for o in sorted(glob.glob(str(d / "lib.so.*gfx950"))):
        notes = subprocess.run([f"{LLVM}/llvm-readelf", "--notes", o], capture_output=True, text=True, check=True).stdout
        if "gemv_kernel_pk13" not in notes:
            continue
        meta = {}
        for item in re.split(r"\n  - ", notes[notes.index("amdhsa.kernels:"):])[1:]:
            name = re.search(r"^\s*\.name:\s+(\S+)", item, re.M)
            if name:
                meta[name.group(1)] = {k: int(v) for k, v in re.findall(r"^\s{0,4}\.(vgpr_count|vgpr_spill_count|sgpr_spill_count|private_segment_fixed_size):\s+(\d+)\s*$", item, re.M)}
        dis = subprocess.run([f"{LLVM}/llvm-objdump", "-d", "--no-show-raw-insn", o], capture_output=True, text=True, check=True).stdout
        cur = None
        for line in dis.splitlines():
            m = re.match(r"^[0-9a-f]+ <(\S+)>:", line)
            if m:
                k = re.search(r"gemv_kernel_pk13ILi(\d+)ELi(\d+)ELi([12])EE", m.group(1))
                cur = tuple(int(x) for x in k.groups()) if k else None
                if cur:
                    assert cur not in out, cur
                    out[cur] = (meta[m.group(1)], [])
                continue
            t = line.strip().split("//")[0].strip()
            if cur and t:
                out[cur][1].append(t)
    return out


def is_nt_load(t):
    return t.startswith("global_load_") and t.split()[-1] == "nt"


def test_every_straight_line_instantiation_is_there(straight_line):
    assert set(straight_line) == {k for k in shipped() if k[2]}


def test_no_scratch_and_at_most_170_vgprs(straight_line):
    for key, (meta, text) in sorted(straight_line.items()):
        assert meta["vgpr_spill_count"] == 0 and meta["sgpr_spill_count"] == 0 and meta["private_segment_fixed_size"] == 0, (key, meta)
        assert meta["vgpr_count"] <= 170, (key, meta)
        assert not any(t.startswith("scratch_") or t.startswith("buffer_") for t in text), key


def test_every_prologue_wait_leaves_the_first_buffer_in_flight(straight_line):
    for (r, e, pro), (meta, text) in sorted(straight_line.items()):
        loads = 7 * r * (2 if e == SILU_MUL else 1)
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
                assert int(t.split()[1]) < 0x8000, f"backward branch in the prologue of {(r, e, pro)}: {t}"
            m = re.search(r"vmcnt\((\d+)\)", t) if t.startswith("s_waitcnt") else None
            if m:
                seen.append(int(m.group(1)))
                assert int(m.group(1)) >= issued, f"{(r, e, pro)}: `{t}` with {issued} nt loads issued: the wait drains the first request"
        # the whole first request and only it: six 16-byte pieces and the 8-byte sign piece per (row, unit)
        assert kinds == {"global_load_dwordx4": loads // 7 * 6, "global_load_dwordx2": loads // 7}, ((r, e, pro), kinds)
        assert seen and min(seen) >= loads, f"{(r, e, pro)}: waits {seen} in front of the barrier"
        assert [n for i, n in vm_waits(text) if i < first] == [], f"{(r, e, pro)}: a vector-memory wait in front of the first weight request"
        # the decoding: one packed 16-bit multiply-add per four weights, one byte permute per weight
        assert any(t.startswith("v_pk_mad_u16") for t in text) and any(t.startswith("v_perm_b32") for t in text)
