"""CPU tier: the decode step's kernels take their leading arguments in user SGPRs (gfx950 kernarg preload).  Read from the code objects
inside the built libaha_hip.so: spills and scratch from the AMDGPU metadata notes, the way tests/test_isa_cpu.py reads its keys; the
preload length from the kernel descriptors (the 64-byte `<kernel>.kd` objects in .rodata, which llvm-objdump decodes into .amdhsa_
directives) -- the metadata notes of this toolchain carry no key for it.  `kernarg_preload_length` is the number of kernarg dwords the
wave launch delivers in SGPRs: 0 when the first parameter is a struct by value (passed by reference) or the translation unit was compiled
without the preload flag (aha_amd/build.py EXTRA_FLAGS)."""
import glob
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LLVM = "/opt/rocm/lib/llvm/bin"
KEYS = ("private_segment_fixed_size", "vgpr_spill_count", "sgpr_spill_count")


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    if not (os.path.exists(f"{LLVM}/llvm-objdump") and os.path.exists(f"{LLVM}/llvm-readelf")):
        pytest.skip("ROCm llvm tools not found")
    from aha_amd import build
    build.build()
    d = tmp_path_factory.mktemp("codeobj")
    shutil.copy(os.path.join(ROOT, "aha_amd", "csrc", "libaha_hip.so"), d / "lib.so")
    subprocess.run([f"{LLVM}/llvm-objdump", "--offloading", "lib.so"], cwd=d, capture_output=True, check=True)   # writes lib.so.N.<target>
    objs = sorted(glob.glob(str(d / "lib.so.*gfx950")))
    assert objs, "no gfx950 code object in libaha_hip.so"
    out = {}
    for o in objs:
        notes = subprocess.run([f"{LLVM}/llvm-readelf", "--notes", o], capture_output=True, text=True, check=True).stdout
        body = notes[notes.index("amdhsa.kernels:"):] if "amdhsa.kernels:" in notes else ""
        for item in re.split(r"\n  - ", body)[1:]:
            item = item.split("\namdhsa.")[0]
            name = re.search(r"^\s*\.name:\s+(\S+)", item, re.M)
            if not name:
                continue
            cur = out.setdefault(name.group(1), {})
            for m in re.finditer(r"^\s{0,4}\.(\w+):\s+(\d+)\s*$", item, re.M):
                if m.group(1) in KEYS:
                    cur[m.group(1)] = int(m.group(2))
        kd = subprocess.run([f"{LLVM}/llvm-objdump", "-D", "-j", ".rodata", o], capture_output=True, text=True, check=True).stdout
        cur = None
        for line in kd.splitlines():
            m = re.match(r"^\.amdhsa_kernel\s+(\S+)", line)
            if m:
                cur = out[m.group(1)]
                cur["kernarg_preload_length"] = 0
                continue
            m = re.match(r"^\s+\.amdhsa_user_sgpr_kernarg_preload_length\s+(\d+)", line)
            if m and cur is not None:
                cur["kernarg_preload_length"] = int(m.group(1))
    assert len(out) > 200 and all(set(KEYS) | {"kernarg_preload_length"} <= set(k) for k in out.values()), "kernel records incomplete"
    return out


def family(name):
    m = re.search(r"\d+([a-z_0-9]+?_kernel)", name)
    return re.sub(r"^aha\d+", "", m.group(1)) if m else name


def of_family(kernels, fam):
    return {n: k for n, k in kernels.items() if family(n) == fam}


def test_matvec_and_decode_attention_arguments_are_preloaded(kernels):
    gemv = {n: k for n, k in kernels.items() if "gemv_kernel" in n}
    assert len(gemv) >= 100
    assert all(k["kernarg_preload_length"] >= 12 for k in gemv.values()), {n: k["kernarg_preload_length"] for n, k in gemv.items() if k["kernarg_preload_length"] < 12}
    attn = of_family(kernels, "attn_decode_fused_kernel")
    assert len(attn) == 1
    assert all(k["kernarg_preload_length"] >= 12 for k in attn.values()), attn


def test_step_kernels_are_preloaded(kernels):
    for fam in ("step_tail_kernel", "embed_state_kernel"):
        ks = of_family(kernels, fam)
        assert len(ks) == 1, (fam, list(ks))
        assert all(k["kernarg_preload_length"] > 0 for k in ks.values()), ks


def test_untouched_sources_are_compiled_as_before(kernels):
    """The flag is per source (build.EXTRA_FLAGS): a kernel of another translation unit has no preloaded arguments, whatever its
    signature -- gemm256q_kernel takes a struct, rmsnorm_rows_kernel and argmax_partials_kernel (kernels_elem.hip) plain pointers."""
    from aha_amd import build
    assert sorted(build.EXTRA_FLAGS) == ["kernels_attn.hip", "kernels_gemv.hip", "model.hip"]
    assert not any("preload" in f for f in build.FLAGS)
    for fam in ("gemm256q_kernel", "rmsnorm_rows_kernel", "argmax_partials_kernel"):
        ks = of_family(kernels, fam)
        assert ks, fam
        assert all(k["kernarg_preload_length"] == 0 for k in ks.values()), (fam, ks)


def test_changed_kernels_do_not_spill(kernels):
    changed = {n: k for n, k in kernels.items()
               if "gemv_kernel" in n or family(n) in ("attn_decode_fused_kernel", "attn_decode_fused_traced_kernel", "step_tail_kernel", "embed_state_kernel")}
    assert len(changed) >= 104
    bad = {n: k for n, k in changed.items() if k.get("vgpr_spill_count", 0) or k.get("sgpr_spill_count", 0) or k.get("private_segment_fixed_size", 0)}
    assert not bad, bad
