"""CPU tier of the group decode attention: its two entries in header, library, ctypes table and Rust shim, and the op entry's refusals
before any device work.  The grouping rule itself is held on the GPU by the bits test (tests/test_attn_group_gpu.py), whose runs are cut
at split changes, at full blocks and into groups of one."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_entries_in_header_library_signatures_and_rust(hip_lib):
    from aha_amd import _lib
    header = open(os.path.join(ROOT, "include", "aha_hip.h")).read()
    rust = open(os.path.join(ROOT, "rust", "aha-hip", "src", "lib.rs")).read()
    for name, nargs in (("aha_hip_attn_decode_group", 14), ("aha_hip_debug_rows_group", 2)):
        decl = re.search(r"\bint %s\(([^;]*)\);" % name, header)
        assert decl and len(decl.group(1).split(",")) == nargs, name
        assert hasattr(hip_lib, name) and len(_lib.SIGNATURES[name][1]) == nargs, name
    assert "pub fn aha_hip_debug_rows_group(m: *mut AhaModel, on: i32) -> i32;" in rust
    assert hip_lib.aha_hip_debug_rows_group(None, 1) == -1 and hip_lib.aha_hip_last_error() == b"debug_rows_group: null model"


def _args(**kw):
    """A call that would be valid if its pointers were: every device pointer a non-null dummy that a refused call never reads."""
    p = C.c_void_p(64)
    a = dict(qkv=p, q_norm_w=p, k_norm_w=p, rope=p, page_ptrs=p, page0=(C.c_int32 * 3)(0, 0, 2), kv_len=(C.c_int32 * 3)(70, 71, 5), rows=3, nh=4,
             kvh=2, eps=1e-6, scale=0.088, o=p, stream=None)
    a.update(kw)
    return list(a.values())


def test_bad_arguments_are_refused_before_device_work(hip_lib):
    """Every case returns AHA_ERR_INVALID on a machine without a GPU: nothing touched the device."""
    group = hip_lib.aha_hip_attn_decode_group
    for ptr in ("qkv", "q_norm_w", "k_norm_w", "rope", "page_ptrs", "page0", "kv_len", "o"):
        assert group(*_args(**{ptr: None})) == -1, ptr
        assert hip_lib.aha_hip_last_error() == b"attn_decode_group: null pointer", ptr
    bad = [dict(rows=0), dict(rows=-2), dict(rows=65536), dict(nh=5), dict(nh=0), dict(kvh=0), dict(nh=34, kvh=2), dict(nh=65, kvh=65),
           dict(kv_len=(C.c_int32 * 3)(70, 0, 5)), dict(kv_len=(C.c_int32 * 3)(70, 71, -1)), dict(page0=(C.c_int32 * 3)(0, -1, 2))]
    for kw in bad:
        assert group(*_args(**kw)) == -1, kw
        assert hip_lib.aha_hip_last_error().startswith(b"attn_decode_group: "), kw
    assert b"row 1" in hip_lib.aha_hip_last_error()
    # the partials of all rows are addressed through one 32-bit offset
    n = 40000
    assert group(*_args(rows=n, nh=64, kvh=64, page0=(C.c_int32 * n)(), kv_len=(C.c_int32 * n)(*([5000] * n)))) == -1
    assert b"below 2^31" in hip_lib.aha_hip_last_error()
