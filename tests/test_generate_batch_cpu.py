"""CPU tier: batched greedy generation (aha_hip_generate_batch) is wired through every layer -- public header, exported symbol, ctypes
table, Rust shim -- its host-side argument checks need no GPU, and its two kernel families ship in the gfx950 code object without flat
loads, scratch or spills, within the register file."""
import glob
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LLVM = "/opt/rocm/lib/llvm/bin"


def test_generate_batch_symbol_in_every_layer(hip_lib):
    from aha_amd import _lib
    header = open(os.path.join(ROOT, "include", "aha_hip.h")).read()
    assert re.search(r"int aha_hip_generate_batch\(aha_model\* m, const uint32_t\* input_ids, const size_t\* seq_lens, size_t n_seqs,"
                     r"\s+size_t max_new,\s+size_t max_tokens_per_pass, uint32_t\* tokens_out, size_t\* n_out, float\* logits_out\);", header)
    for name, nargs in (("aha_hip_generate_batch", 9), ("aha_hip_gemv_rows", 11), ("aha_hip_attn_decode_batch", 14),
                        ("aha_hip_debug_attn_decode_fused", 12), ("aha_hip_debug_attn_decode_rows", 15), ("aha_hip_debug_spec_accept", 8)):
        assert f"int {name}(" in header, name
        assert hasattr(hip_lib, name), name
        assert len(_lib.SIGNATURES[name][1]) == nargs, name
    src = open(os.path.join(ROOT, "rust", "aha-hip", "src", "lib.rs")).read()
    ext = src[src.index('extern "C" {'):]
    ext = ext[:ext.index("\n    }\n")]
    assert re.search(r"pub fn aha_hip_generate_batch\(\s*m: \*mut AhaModel,\s*ids: \*const u32,\s*seq_lens: \*const usize,\s*n_seqs: usize,"
                     r"\s*max_new: usize,\s*max_tokens_per_pass: usize,\s*tokens_out: \*mut u32,\s*n_out: \*mut usize,\s*logits_out: \*mut f32,?"
                     r"\s*\) -> i32;", ext)
    assert re.search(r"pub fn generate_batch\(&mut self, prompts: &\[&\[u32\]\], max_new: usize, max_tokens_per_pass: usize\)"
                     r" -> Result<Vec<Vec<u32>>, Error>", src)


def test_generate_batch_null_and_empty_arguments_fail_cleanly(hip_lib):
    """Host-side argument checks run before any device work: no GPU needed."""
    assert hip_lib.aha_hip_generate_batch(None, None, None, 0, 0, 0, None, None, None) == -1   # AHA_ERR_INVALID
    assert b"null model" in hip_lib.aha_hip_last_error()
    assert hip_lib.aha_hip_gemv_rows(None, None, None, 0, 0, 0, 0, None, None, None, None) == -1
    assert hip_lib.aha_hip_attn_decode_batch(None, None, None, None, None, None, None, 0, 4, 2, 1e-6, 0.088, None, None) == -1
    assert hip_lib.aha_hip_debug_attn_decode_fused(None, None, None, None, None, 0, 4, 2, 1e-6, 0.088, None, None) == -1


def _code_objects(tmp_path):
    if not (os.path.exists(f"{LLVM}/llvm-objdump") and os.path.exists(f"{LLVM}/llvm-readelf")):
        pytest.skip("ROCm llvm tools not found")
    from aha_amd import build
    build.build()
    shutil.copy(os.path.join(ROOT, "aha_amd", "csrc", "libaha_hip.so"), tmp_path / "lib.so")
    subprocess.run([f"{LLVM}/llvm-objdump", "--offloading", "lib.so"], cwd=tmp_path, capture_output=True, check=True)
    objs = sorted(glob.glob(str(tmp_path / "lib.so.*gfx950")))
    assert objs
    return objs


FAMILIES = ("gemv_rows_kernel", "gemv_rows_merge_kernel", "attn_decode_batch_kernel", "argmax_rows_kernel", "gen_embed_kernel")


def _family(name):
    m = re.search(r"\d+([a-z_0-9]+?_kernel)", name)
    return m.group(1) if m else name


def test_batch_kernels_have_no_flat_loads_scratch_or_spills(tmp_path):
    objs = _code_objects(tmp_path)
    meta = {}
    for o in objs:
        notes = subprocess.run([f"{LLVM}/llvm-readelf", "--notes", o], capture_output=True, text=True, check=True).stdout
        body = notes[notes.index("amdhsa.kernels:"):]
        for item in re.split(r"\n  - ", body)[1:]:
            name = re.search(r"^\s*\.name:\s+(\S+)", item, re.M)
            if name and _family(name.group(1)) in FAMILIES:
                meta[name.group(1)] = {k: int(v) for k, v in re.findall(r"^\s{0,4}\.(\w+):\s+(\d+)\s*$", item, re.M)}
    assert {_family(n) for n in meta} == set(FAMILIES)
    assert len([n for n in meta if _family(n) == "gemv_rows_kernel"]) == 4
    for n, k in meta.items():
        assert k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0 and k["private_segment_fixed_size"] == 0, (n, k)
        assert k["vgpr_count"] <= 256, (n, k)    # two waves per SIMD (launch bounds 256, 2)
    bad, seen = {}, set()
    for o in objs:
        dis = subprocess.run([f"{LLVM}/llvm-objdump", "-d", "--no-show-raw-insn", o], capture_output=True, text=True, check=True).stdout
        cur = None
        for line in dis.splitlines():
            m = re.match(r"^[0-9a-f]+ <(\S+)>:", line)
            if m:
                cur = m.group(1)
                continue
            if not cur or _family(cur) not in ("gemv_rows_kernel", "gemv_rows_merge_kernel", "attn_decode_batch_kernel"):
                continue
            seen.add(_family(cur))
            op = line.split()[0] if line.split() else ""
            if op.startswith("flat_load") or op.startswith("scratch_"):
                bad.setdefault(cur, []).append(op)
    assert len(seen) == 3 and not bad, bad
