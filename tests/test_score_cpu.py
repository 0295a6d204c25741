"""CPU tier: the scoring entries (aha_hip_score_rows / aha_hip_score_batch, aha_token_score) exist in every layer -- header, library
exports, ctypes table, Rust shim -- with one struct layout, and the host plan of the fused kernel splits the work as DESIGN.md says."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("aha_hip_score_rows", "aha_hip_score_batch")


@pytest.mark.parametrize("name", NAMES)
def test_symbol_in_every_layer(hip_lib, name):
    from aha_amd import _lib
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "aha_hip.h")).read(), flags=re.S)
    rust = open(os.path.join(ROOT, "rust", "aha-hip", "src", "lib.rs")).read()
    assert re.search(r"\bint %s\s*\(" % name, header)
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), name)
    assert name in _lib.SIGNATURES and _lib.SIGNATURES[name][0] is ctypes.c_int
    assert re.search(r"pub fn %s\(" % name, rust)
    nargs = len(re.search(r"\bint %s\s*\(([^)]*)\)" % name, header).group(1).split(","))
    assert len(_lib.SIGNATURES[name][1]) == nargs


def test_token_score_layout():
    from aha_amd import _lib
    T = _lib.TokenScore
    assert ctypes.sizeof(T) == 12
    assert [(n, getattr(T, n).offset) for n, _ in T._fields_] == [("logprob", 0), ("top_id", 4), ("top_logprob", 8)]
    rust = open(os.path.join(ROOT, "rust", "aha-hip", "src", "lib.rs")).read()
    body = rust[rust.index("pub struct AhaTokenScore {"):]
    body = body[:body.index("}")]
    assert "#[repr(C)]" in rust[:rust.index("pub struct AhaTokenScore {")][-80:]
    assert re.findall(r"pub (\w+): (\w+)", body) == [("logprob", "f32"), ("top_id", "u32"), ("top_logprob", "f32")]
    assert "pub fn score_batch(" in rust
