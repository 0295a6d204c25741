"""CPU tier: the packed-batch embedding entry point (aha_hip_embed_batch) is wired through every layer -- declared in the public header,
exported by the built library, bound in the ctypes table, declared and wrapped in the Rust shim -- and its pooling kernel ships in the
gfx950 code object."""
import glob
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LLVM = "/opt/rocm/lib/llvm/bin"


def test_embed_batch_symbol_in_every_layer(hip_lib):
    from aha_amd import _lib
    header = open(os.path.join(ROOT, "include", "aha_hip.h")).read()
    assert re.search(r"int aha_hip_embed_batch\(aha_model\* m, const uint32_t\* input_ids, const size_t\* seq_lens, size_t n_seqs,"
                     r"\s+size_t max_tokens_per_pass,\s+float\* out\);", header)
    assert hasattr(hip_lib, "aha_hip_embed_batch")
    restype, args = _lib.SIGNATURES["aha_hip_embed_batch"]
    assert len(args) == 6
    src = open(os.path.join(ROOT, "rust", "aha-hip", "src", "lib.rs")).read()
    ext = src[src.index('extern "C" {'):]
    ext = ext[:ext.index("\n    }\n")]
    assert re.search(r"pub fn aha_hip_embed_batch\(\s*m: \*mut AhaModel,\s*ids: \*const u32,\s*seq_lens: \*const usize,\s*n_seqs: usize,"
                     r"\s*max_tokens_per_pass: usize,\s*out: \*mut f32,?\s*\) -> i32;", ext)
    assert re.search(r"pub fn embed_batch\(&mut self, seqs: &\[&\[u32\]\], max_tokens_per_pass: usize\) -> Result<Vec<f32>, Error>", src)


def test_embed_batch_null_and_empty_arguments_fail_cleanly(hip_lib):
    """Host-side argument checks run before any device work: no GPU needed."""
    assert hip_lib.aha_hip_embed_batch(None, None, None, 0, 0, None) == -1   # AHA_ERR_INVALID
    assert b"null model" in hip_lib.aha_hip_last_error()


def test_pooling_kernel_in_the_code_object(tmp_path):
    if not (os.path.exists(f"{LLVM}/llvm-objdump") and os.path.exists(f"{LLVM}/llvm-readelf")):
        pytest.skip("ROCm llvm tools not found")
    from aha_amd import build
    build.build()
    shutil.copy(os.path.join(ROOT, "aha_amd", "csrc", "libaha_hip.so"), tmp_path / "lib.so")
    subprocess.run([f"{LLVM}/llvm-objdump", "--offloading", "lib.so"], cwd=tmp_path, capture_output=True, check=True)
    objs = sorted(glob.glob(str(tmp_path / "lib.so.*gfx950")))
    assert objs
    notes = "".join(subprocess.run([f"{LLVM}/llvm-readelf", "--notes", o], capture_output=True, text=True, check=True).stdout for o in objs)
    names = re.findall(r"\.name:\s+(\S*embed_pool_kernel\S*)", notes)
    assert names, "embed_pool_kernel is not in the gfx950 code object"
