"""CPU tier of the continuous batching engine (aha_hip_engine_*): the header, the library's exports, the ctypes SIGNATURES and the Rust
shim agree; null or invalid handles, configs, params and ids are refused with AHA_ERR_INVALID before any device work; the code objects of
the kernels the engine changed (the packed prefill attention with a per-segment cache prefix, the batched decode attention with
slot-keyed counters) stay free of spills and scratch."""
import ctypes as C
import glob
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENGINE_FNS = ["aha_hip_engine_create", "aha_hip_engine_destroy", "aha_hip_engine_submit", "aha_hip_engine_cancel", "aha_hip_engine_step",
              "aha_hip_engine_stats", "aha_hip_engine_debug_ctr_base"]


def test_header_exports_signatures_and_rust_agree(hip_lib):
    from aha_amd import _lib
    header = open(os.path.join(ROOT, "include", "aha_hip.h")).read()
    rust = open(os.path.join(ROOT, "rust", "aha-hip", "src", "lib.rs")).read()
    for f in ENGINE_FNS:
        assert re.search(r"\b%s\s*\(" % f, header), f
        assert hasattr(hip_lib, f), f
        assert f in _lib.SIGNATURES, f
        assert re.search(r"pub fn %s\(" % f, rust), f
    f = "aha_hip_debug_attn_prefill_segs"   # the op-level test entry of the packed attention with a cache prefix (no Rust binding)
    assert re.search(r"\b%s\s*\(" % f, header) and hasattr(hip_lib, f) and f in _lib.SIGNATURES
    for name, py in (("aha_engine_config", _lib.EngineConfig), ("aha_engine_event", _lib.EngineEvent), ("aha_engine_stats", _lib.EngineStats)):
        body = header[header.index("typedef struct %s {" % name):]
        body = body[:body.index("} %s;" % name)]
        assert re.findall(r"(\w+);", body) == [n for n, _ in py._fields_], name
    assert C.sizeof(_lib.EngineEvent) == 16 and C.sizeof(_lib.EngineConfig) == 32
    for rs, py in (("AhaEngineConfig", _lib.EngineConfig), ("AhaEngineEvent", _lib.EngineEvent), ("AhaEngineStats", _lib.EngineStats)):
        body = rust[rust.index("pub struct %s {" % rs):]
        body = body[:body.index("}")]
        assert re.findall(r"pub (\w+):", body) == [n for n, _ in py._fields_], rs


def test_null_and_invalid_arguments_are_refused_before_device_work(hip_lib):
    from aha_amd import _lib
    L = hip_lib
    out = C.c_void_p()
    cfg = _lib.EngineConfig(4, 16, 0, 0)
    assert L.aha_hip_engine_create(None, C.byref(cfg), C.byref(out)) == -1
    assert L.aha_hip_engine_create(None, None, C.byref(out)) == -1
    # the config is checked before the model is looked at: every rule, with no model at all
    for bad in ((0, 16, 0, 0), (65, 16, 0, 0), (4, 0, 0, 0), (4, 16, 63, 0), (4, 16, 0, 100), (4, 16, 512, 1024), (4, 1 << 19, 0, 0)):
        assert L.aha_hip_engine_create(None, C.byref(_lib.EngineConfig(*bad)), C.byref(out)) == -1, bad
        assert "bad config" in L.aha_hip_last_error().decode(), bad
    for good in ((1, 1, 64, 64), (64, 16, 0, 0), (8, 16, 2048, 1024)):
        assert L.aha_hip_engine_create(None, C.byref(_lib.EngineConfig(*good)), C.byref(out)) == -1, good
        assert "null model" in L.aha_hip_last_error().decode(), good
    ids = (C.c_uint32 * 3)(1, 2, 3)
    rid = C.c_uint64()
    assert L.aha_hip_engine_submit(None, ids, 3, None, None, 4, C.byref(rid)) == -1
    assert "null engine" in L.aha_hip_last_error().decode()
    bad = _lib.SamplingParams(float("nan"), 1.0, 0, 1.0, 64, 0, 1)
    assert L.aha_hip_engine_submit(None, ids, 3, None, C.byref(bad), 4, C.byref(rid)) == -1
    assert "params" in L.aha_hip_last_error().decode()
    bad_k = _lib.SamplingParams(0.7, 1.0, 0, 1.0, 64, _lib.AHA_SAMPLE_HAS_TOP_K, 1)
    assert L.aha_hip_engine_submit(None, ids, 3, None, C.byref(bad_k), 4, C.byref(rid)) == -1
    assert L.aha_hip_engine_cancel(None, 1) == -1
    n = C.c_size_t()
    evs = (_lib.EngineEvent * 4)()
    assert L.aha_hip_engine_step(None, evs, 4, C.byref(n), None) == -1
    st = _lib.EngineStats()
    assert L.aha_hip_engine_stats(None, C.byref(st)) == -1
    assert L.aha_hip_engine_debug_ctr_base(None, 5) == -1
    L.aha_hip_engine_destroy(None)   # a no-op


LLVM = "/opt/rocm/lib/llvm/bin"


def test_code_objects_of_the_changed_attention_kernels(hip_lib, tmp_path):
    if not (os.path.exists(f"{LLVM}/llvm-objdump") and os.path.exists(f"{LLVM}/llvm-readelf")):
        pytest.skip("ROCm llvm tools not found")
    shutil.copy(os.path.join(ROOT, "aha_amd", "csrc", "libaha_hip.so"), tmp_path / "lib.so")
    subprocess.run([f"{LLVM}/llvm-objdump", "--offloading", "lib.so"], cwd=tmp_path, capture_output=True, check=True)
    seen = {"attn_prefill_kernel": 0, "attn_decode_batch_kernel": 0}
    for o in sorted(glob.glob(str(tmp_path / "lib.so.*gfx950"))):
        notes = subprocess.run([f"{LLVM}/llvm-readelf", "--notes", o], capture_output=True, text=True, check=True).stdout
        body = notes[notes.index("amdhsa.kernels:"):] if "amdhsa.kernels:" in notes else ""
        for item in re.split(r"\n  - ", body)[1:]:
            name = re.search(r"^\s*\.name:\s+(\S+)", item, re.M)
            if not name:
                continue
            fam = [k for k in seen if k in name.group(1)]
            if not fam or ("attn_prefill_kernel" in name.group(1) and "Lb1E" in name.group(1)):   # (debug TRACE instantiations)
                continue
            seen[fam[0]] += 1
            vals = {k: int(v) for k, v in re.findall(r"\.(private_segment_fixed_size|vgpr_spill_count|sgpr_spill_count|vgpr_count):\s+(\d+)", item)}
            assert vals["private_segment_fixed_size"] == 0 and vals["vgpr_spill_count"] == 0 and vals["sgpr_spill_count"] == 0, name.group(1)
            assert vals["vgpr_count"] <= 256, name.group(1)
    assert all(seen.values()), seen
