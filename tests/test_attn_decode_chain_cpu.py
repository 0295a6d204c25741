"""CPU tier: the linear form of the fused decode attention (family attn_decode_fused_kernel: page addresses by arithmetic from two
preloaded kernel arguments) as the compiler emitted it, read from the gfx950 code objects inside the built libaha_hip.so the way
tests/test_decode_preload_cpu.py reads them.

  * the family is one kernel; it still takes at least 12 leading dwords in user SGPRs, has no spill and no scratch, and stays within
    256 VGPRs; the table form is a twin with a family name of its own, held to the same;
  * no wait on a vector-memory return stands in front of the first K/V request: in program text there is no `s_waitcnt` with a
    `vmcnt` field between the kernel's entry and its first `global_load_dwordx4` (the first K fragment: the prologue's own inputs are
    2- and 4-byte loads).  The table form has to have such a wait (the page pointers are loaded): the scan is run on it too, as
    the check that the scan sees what it is meant to see.
"""
import glob
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LLVM = "/opt/rocm/lib/llvm/bin"
KEYS = ("private_segment_fixed_size", "vgpr_spill_count", "sgpr_spill_count", "vgpr_count")
FAMILIES = ("attn_decode_fused_kernel", "attn_decode_fused_table_kernel")


def family(name):
    m = re.search(r"\d+([a-z_0-9]+?_kernel)", name)
    return re.sub(r"^aha\d+", "", m.group(1)) if m else name


@pytest.fixture(scope="module")
def attn(tmp_path_factory):
    """{family: (kernel name, metadata + preload length, program text as a list of instructions)} of the two decode attention kernels."""
    if not (os.path.exists(f"{LLVM}/llvm-objdump") and os.path.exists(f"{LLVM}/llvm-readelf")):
        pytest.skip("ROCm llvm tools not found")
    from aha_amd import build
    build.build()
    d = tmp_path_factory.mktemp("codeobj")
    shutil.copy(os.path.join(ROOT, "aha_amd", "csrc", "libaha_hip.so"), d / "lib.so")
    subprocess.run([f"{LLVM}/llvm-objdump", "--offloading", "lib.so"], cwd=d, capture_output=True, check=True)   # writes lib.so.N.<target>
    objs = sorted(glob.glob(str(d / "lib.so.*gfx950")))
    assert objs, "no gfx950 code object in libaha_hip.so"
    meta, text = {}, {}
    for o in objs:
        notes = subprocess.run([f"{LLVM}/llvm-readelf", "--notes", o], capture_output=True, text=True, check=True).stdout
        if "attn_decode_fused" not in notes:
            continue
        body = notes[notes.index("amdhsa.kernels:"):]
        for item in re.split(r"\n  - ", body)[1:]:
            item = item.split("\namdhsa.")[0]
            name = re.search(r"^\s*\.name:\s+(\S+)", item, re.M)
            if not name or family(name.group(1)) not in FAMILIES:
                continue
            cur = meta.setdefault(name.group(1), {})
            for m in re.finditer(r"^\s{0,4}\.(\w+):\s+(\d+)\s*$", item, re.M):
                if m.group(1) in KEYS:
                    cur[m.group(1)] = int(m.group(2))
        kd = subprocess.run([f"{LLVM}/llvm-objdump", "-D", "-j", ".rodata", o], capture_output=True, text=True, check=True).stdout
        cur = None
        for line in kd.splitlines():
            m = re.match(r"^\.amdhsa_kernel\s+(\S+)", line)
            if m:
                cur = meta.get(m.group(1))
                if cur is not None:
                    cur["kernarg_preload_length"] = 0
                continue
            m = re.match(r"^\s+\.amdhsa_user_sgpr_kernarg_preload_length\s+(\d+)", line)
            if m and cur is not None:
                cur["kernarg_preload_length"] = int(m.group(1))
        dis = subprocess.run([f"{LLVM}/llvm-objdump", "-d", "--no-show-raw-insn", o], capture_output=True, text=True, check=True).stdout
        cur = None
        for line in dis.splitlines():
            m = re.match(r"^[0-9a-f]+ <(\S+)>:", line)
            if m:
                cur = m.group(1) if m.group(1) in meta else None
                continue
            t = line.strip().split("//")[0].strip()
            if cur and t:
                text.setdefault(cur, []).append(t)
    out = {}
    for n, k in meta.items():
        assert family(n) not in out, f"more than one kernel of family {family(n)}"
        assert set(KEYS) | {"kernarg_preload_length"} <= set(k) and text.get(n), (n, k)
        out[family(n)] = (n, k, text[n])
    assert sorted(out) == sorted(FAMILIES), sorted(out)
    return out


@pytest.mark.parametrize("fam", FAMILIES)
def test_preloaded_arguments_no_spill_and_register_budget(attn, fam):
    n, k, _ = attn[fam]
    assert k["kernarg_preload_length"] >= 12, (n, k)
    assert k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0 and k["private_segment_fixed_size"] == 0, (n, k)
    assert k["vgpr_count"] <= 256, (n, k)


def waits_before_first_kv_request(text):
    first = next(i for i, t in enumerate(text) if t.startswith("global_load_dwordx4"))
    return [t for t in text[:first] if t.startswith("s_waitcnt") and "vmcnt" in t]


def test_no_vector_memory_wait_in_front_of_the_first_kv_request(attn):
    _, _, linear = attn["attn_decode_fused_kernel"]
    assert waits_before_first_kv_request(linear) == []
    # the same scan on the table form finds the wait for the page pointers: the scan is not blind
    _, _, table = attn["attn_decode_fused_table_kernel"]
    assert waits_before_first_kv_request(table) != []
