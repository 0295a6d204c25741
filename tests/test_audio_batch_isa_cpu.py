"""CPU tier: the audio tower's batched kernels (the clip-table log-mel pair, the chunk-table conv1 im2col, the slot-table K / V packer) in
the shipped gfx950 code objects pass the audit every shipped kernel passes (tests/test_isa_cpu.py): no register spills, no scratch, no
flat loads and no scratch instructions (flat STORES into KV pages -- page addresses are integers from the page table -- are fine)."""
import glob
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LLVM = "/opt/rocm/lib/llvm/bin"
FAMILIES = ("logmel_power_kernel", "logmel_finalize_kernel", "audio_im2col1_kernel", "kv_pack_generic_kernel")


@pytest.fixture(scope="module")
def code_objects(tmp_path_factory):
    if not (os.path.exists(f"{LLVM}/llvm-objdump") and os.path.exists(f"{LLVM}/llvm-readelf")):
        pytest.skip("ROCm llvm tools not found")
    from aha_amd import build
    build.build()
    d = tmp_path_factory.mktemp("audio_codeobj")
    shutil.copy(os.path.join(ROOT, "aha_amd", "csrc", "libaha_hip.so"), d / "lib.so")
    subprocess.run([f"{LLVM}/llvm-objdump", "--offloading", "lib.so"], cwd=d, capture_output=True, check=True)
    objs = sorted(glob.glob(str(d / "lib.so.*gfx950")))
    assert objs, "no gfx950 code object in libaha_hip.so"
    return objs


def _family(name):
    return next((f for f in FAMILIES if f in name), None)


def test_audio_batch_kernels_have_no_spills_or_scratch(code_objects):
    seen = {}
    for o in code_objects:
        notes = subprocess.run([f"{LLVM}/llvm-readelf", "--notes", o], capture_output=True, text=True, check=True).stdout
        body = notes[notes.index("amdhsa.kernels:"):] if "amdhsa.kernels:" in notes else ""
        for item in re.split(r"\n  - ", body)[1:]:
            item = item.split("\namdhsa.")[0]
            name = re.search(r"^\s*\.name:\s+(\S+)", item, re.M)
            if not name or not _family(name.group(1)):
                continue
            vals = {m.group(1): int(m.group(2)) for m in re.finditer(r"^\s{0,4}\.(\w+):\s+(\d+)\s*$", item, re.M)}
            seen[name.group(1)] = vals
    assert {_family(n) for n in seen} == set(FAMILIES), f"kernels missing from the metadata: {set(FAMILIES) - {_family(n) for n in seen}}"
    bad = {n: v for n, v in seen.items()
           if v.get("vgpr_spill_count", 0) or v.get("sgpr_spill_count", 0) or v.get("private_segment_fixed_size", 0)}
    assert not bad, f"audio kernels with spills / scratch: {bad}"


def test_audio_batch_kernels_have_no_flat_loads(code_objects):
    seen, bad = set(), {}
    for o in code_objects:
        dis = subprocess.run([f"{LLVM}/llvm-objdump", "-d", "--no-show-raw-insn", o], capture_output=True, text=True, check=True).stdout
        cur = None
        for line in dis.splitlines():
            m = re.match(r"^[0-9a-f]+ <(\S+)>:", line)
            if m:
                cur = m.group(1)
                continue
            f = _family(cur) if cur else None
            if not f:
                continue
            seen.add(f)
            op = line.split()[0] if line.split() else ""
            if op.startswith("flat_load") or op.startswith("flat_atomic") or op.startswith("scratch_"):
                bad.setdefault(cur, []).append(op)
    assert seen == set(FAMILIES), f"families not found in the disassembly: {set(FAMILIES) - seen}"
    assert not bad, f"flat loads / scratch in the audio kernels: { {k: v[:3] for k, v in bad.items()} }"
