"""CPU tier: per-token log-probabilities (aha_hip_logprob_rows, aha_hip_generate_batch_logprobs, aha_hip_engine_submit_logprobs,
aha_hip_engine_step_logprobs) are wired through every layer -- declared in the public header, exported by the built library, bound in the
ctypes table, declared in the Rust shim with the same struct layout -- the two kernels of the pass ship in the gfx950 code object, and
the op-level entry rejects bad arguments before it touches a device."""
import ctypes as C
import glob
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LLVM = "/opt/rocm/lib/llvm/bin"
SYMBOLS = ["aha_hip_logprob_rows", "aha_hip_generate_batch_logprobs", "aha_hip_engine_submit_logprobs", "aha_hip_engine_step_logprobs"]
N_ARGS = {"aha_hip_logprob_rows": 8, "aha_hip_generate_batch_logprobs": 13, "aha_hip_engine_submit_logprobs": 8,
          "aha_hip_engine_step_logprobs": 6}


def rust_source():
    return open(os.path.join(ROOT, "rust", "aha-hip", "src", "lib.rs")).read()


def test_logprob_symbols_in_every_layer(hip_lib):
    from aha_amd import _lib
    header = open(os.path.join(ROOT, "include", "aha_hip.h")).read()
    src = rust_source()
    ext = src[src.index('extern "C" {'):]
    ext = ext[:ext.index("\n    }\n")]
    for name in SYMBOLS:
        decl = re.search(r"\nint %s\(([^;]*)\);" % name, header)
        assert decl, f"{name} is not declared in include/aha_hip.h"
        assert len(decl.group(1).split(",")) == N_ARGS[name], name
        assert hasattr(hip_lib, name), f"{name} is not exported"
        restype, args = _lib.SIGNATURES[name]
        assert restype is C.c_int and len(args) == N_ARGS[name], name
        rdecl = re.search(r"pub fn %s\(([^;]*)\) -> i32;" % name, ext)
        assert rdecl, f"{name} is not declared in the Rust shim"
        assert len([a for a in rdecl.group(1).split(",") if a.strip()]) == N_ARGS[name], name
    for wrapper in ("pub fn generate_batch_logprobs(", "pub fn submit_logprobs(", "pub fn step_logprobs("):
        assert wrapper in src, wrapper
    assert re.search(r"#define AHA_MAX_TOP_LOGPROBS 20\b", header)
    # the header states what the numbers mean and what is out of scope
    for phrase in ("temperature 1", "before the repeat penalty", "`echo`", "aha_hip_generate_batch_spec", "ensor-parallel", "logit_bias"):
        assert phrase in header[header.index("per-token log-probabilities"):header.index("int aha_hip_generate_batch_logprobs(")], phrase


def test_token_logprobs_layout_matches_header_and_rust():
    from aha_amd import _lib
    T = _lib.TokenLogprobs
    assert C.sizeof(T) == 168
    assert T.logprob.offset == 0 and T.n_top.offset == 4 and T.top_ids.offset == 8 and T.top_logprobs.offset == 88
    src = rust_source()
    body = re.search(r"#\[repr\(C\)\]\s*(?:#\[derive\([^)]*\)\]\s*)?pub struct AhaTokenLogprobs \{(.*?)\n    \}", src, re.S)
    assert body, "AhaTokenLogprobs is not a #[repr(C)] struct in the Rust shim"
    rust_fields = re.findall(r"pub (\w+): ([^,]+),", body.group(1))
    assert [f for f, _ in rust_fields] == [f[0] for f in T._fields_]
    assert [t.strip() for _, t in rust_fields] == ["f32", "i32", "[u32; AHA_MAX_TOP_LOGPROBS]", "[f32; AHA_MAX_TOP_LOGPROBS]"]
    assert re.search(r"pub const AHA_MAX_TOP_LOGPROBS: usize = 20;", src)
    header = open(os.path.join(ROOT, "include", "aha_hip.h")).read()
    hbody = re.search(r"typedef struct aha_token_logprobs \{(.*?)\} aha_token_logprobs;", header, re.S).group(1)
    hbody = re.sub(r"/\*.*?\*/", "", hbody, flags=re.S)
    assert re.findall(r"\b(\w+)(?:\[AHA_MAX_TOP_LOGPROBS\])?;", hbody) == [f[0] for f in T._fields_]


def test_logprob_kernels_in_the_code_object(tmp_path):
    if not (os.path.exists(f"{LLVM}/llvm-objdump") and os.path.exists(f"{LLVM}/llvm-readelf")):
        pytest.skip("ROCm llvm tools not found")
    from aha_amd import build
    build.build()
    shutil.copy(os.path.join(ROOT, "aha_amd", "csrc", "libaha_hip.so"), tmp_path / "lib.so")
    subprocess.run([f"{LLVM}/llvm-objdump", "--offloading", "lib.so"], cwd=tmp_path, capture_output=True, check=True)
    objs = sorted(glob.glob(str(tmp_path / "lib.so.*gfx950")))
    assert objs
    notes = "".join(subprocess.run([f"{LLVM}/llvm-readelf", "--notes", o], capture_output=True, text=True, check=True).stdout for o in objs)
    for kernel in ("logprob_rows_stage1_kernel", "logprob_rows_stage2_kernel"):
        assert re.findall(r"\.name:\s+(\S*%s\S*)" % kernel, notes), f"{kernel} is not in the gfx950 code object"


def test_logprob_rows_rejects_bad_arguments_before_the_device(hip_lib):
    """R = 0, V = 0, n_top = 21, n_top = -1 and null pointers: AHA_ERR_INVALID from the host-side checks (the pointers are never read as
    device memory, so fake non-null ones do)."""
    AHA_ERR_INVALID = -1
    buf = (C.c_float * 64)()
    p = C.addressof(buf)

    def call(R, V, n_top, logits=p, tokens=p, out=p, ld=None):
        nt = (C.c_int32 * max(len(n_top), 1))(*n_top)
        return hip_lib.aha_hip_logprob_rows(logits, V if ld is None else ld, R, V, tokens, nt, out, None)
    assert call(0, 8, [5]) == AHA_ERR_INVALID
    assert b"logprob_rows" in hip_lib.aha_hip_last_error()
    assert call(1, 0, [5]) == AHA_ERR_INVALID
    assert call(2, 8, [20, 21]) == AHA_ERR_INVALID
    assert b"row 1" in hip_lib.aha_hip_last_error()
    assert call(1, 8, [-1]) == AHA_ERR_INVALID
    assert call(1, 8, [5], ld=7) == AHA_ERR_INVALID
    assert call(1, 8, [5], logits=None) == AHA_ERR_INVALID
    assert call(1, 8, [5], tokens=None) == AHA_ERR_INVALID
    assert call(1, 8, [5], out=None) == AHA_ERR_INVALID
    assert hip_lib.aha_hip_logprob_rows(p, 8, 1, 8, p, None, p, None) == AHA_ERR_INVALID


def test_generation_entries_reject_bad_top_logprobs_before_the_model(hip_lib):
    """The top_logprobs checks come before the model is looked at: a null model never gets that far."""
    AHA_ERR_INVALID = -1
    from aha_amd import _lib
    lp = (_lib.TokenLogprobs * 4)()
    for bad in (21, -2):
        top = (C.c_int32 * 2)(5, bad)
        assert hip_lib.aha_hip_generate_batch_logprobs(None, None, None, 2, None, None, top, 2, 0, None, None, None, lp) == AHA_ERR_INVALID
        msg = hip_lib.aha_hip_last_error()
        assert b"sequence 1" in msg and str(bad).encode() in msg, msg
    top = (C.c_int32 * 2)(5, -1)
    assert hip_lib.aha_hip_generate_batch_logprobs(None, None, None, 2, None, None, top, 2, 0, None, None, None, None) == AHA_ERR_INVALID
    assert b"logprobs_out" in hip_lib.aha_hip_last_error()
    assert hip_lib.aha_hip_generate_batch_logprobs(None, None, None, 2, None, None, None, 2, 0, None, None, None, lp) == AHA_ERR_INVALID
    assert b"top_logprobs" in hip_lib.aha_hip_last_error()
    assert hip_lib.aha_hip_generate_batch_logprobs(None, None, None, 2, None, None, top, 2, 0, None, None, None, lp) == AHA_ERR_INVALID
    assert b"null model" in hip_lib.aha_hip_last_error()
    rid = C.c_uint64()
    for bad in (21, -1):
        assert hip_lib.aha_hip_engine_submit_logprobs(None, None, 0, None, None, 4, bad, C.byref(rid)) == AHA_ERR_INVALID
        assert b"top_logprobs" in hip_lib.aha_hip_last_error()
    assert hip_lib.aha_hip_engine_submit_logprobs(None, None, 0, None, None, 4, 5, C.byref(rid)) == AHA_ERR_INVALID
    assert b"null engine" in hip_lib.aha_hip_last_error()
