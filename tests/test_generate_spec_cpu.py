"""CPU tier: draft-and-verify greedy decoding (aha_hip_generate_batch_spec) is wired through every layer -- public header, exported
symbols, ctypes table, Rust shim with matching struct fields --, its host-side proposer (aha_hip_spec_propose) equals the Python
definition in aha_amd/speculative.py on hand-written and on random cases, invalid configurations fail before any device work with the
messages the header documents, and its new kernels ship in the gfx950 code object without scratch, spills or flat memory accesses."""
import ctypes as C
import glob
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from aha_amd.speculative import SpecConfig, propose, row_budget

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LLVM = "/opt/rocm/lib/llvm/bin"
AHA_ERR_INVALID = -1


# ---- wiring ----------------------------------------------------------------------------------------------------------------------
def test_spec_symbols_in_every_layer(hip_lib):
    from aha_amd import _lib
    header = open(os.path.join(ROOT, "include", "aha_hip.h")).read()
    src = open(os.path.join(ROOT, "rust", "aha-hip", "src", "lib.rs")).read()
    ext = src[src.index('extern "C" {'):]
    ext = ext[:ext.index("\n    }\n")]
    for name, nargs in (("aha_hip_generate_batch_spec", 15), ("aha_hip_spec_propose", 8)):
        decl = re.search(r"int %s\(([^;]*)\);" % name, header)
        assert decl, name
        assert len(decl.group(1).split(",")) == nargs, name
        assert hasattr(hip_lib, name), name
        assert len(_lib.SIGNATURES[name][1]) == nargs, name
        rust = re.search(r"pub fn %s\(([^;]*)\) -> i32;" % name, ext)
        assert rust, name
        assert len([a for a in rust.group(1).split(",") if a.strip()]) == nargs, name
    assert "pub fn generate_batch_spec(" in src
    # the reference lines each entry realises
    assert "params/chat.rs:105" in header and "params/shared.rs:58-63" in header

    def header_fields(struct):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), header, re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        return re.findall(r"(\w+);", body)

    def rust_fields(struct):
        body = src[src.index("pub struct %s {" % struct):]
        body = body[:body.index("\n    }\n")]
        return re.findall(r"pub (\w+):", body)

    for cstruct, ctype, rstruct in (("aha_spec_config", _lib.SpecConfig, "AhaSpecConfig"), ("aha_spec_stats", _lib.SpecStats, "AhaSpecStats")):
        names = [n for n, _ in ctype._fields_]
        assert header_fields(cstruct) == names == rust_fields(rstruct), cstruct
    assert C.sizeof(_lib.SpecConfig) == 12 and C.sizeof(_lib.SpecStats) == 4 * C.sizeof(C.c_size_t)
    # the Python surface
    from aha_amd.model import HipInferenceModel, Usage
    assert callable(HipInferenceModel.generate_batch_spec)
    u = Usage(1, 0.0, 1, 1.0)
    assert u.accepted_prediction_tokens is None and u.rejected_prediction_tokens is None


# ---- proposer ----------------------------------------------------------------------------------------------------------------------
def c_propose(lib, spec, context, n_prompt, prediction):
    from aha_amd import _lib
    cs = _lib.SpecConfig(spec.max_draft, spec.ngram_min, spec.ngram_max)
    ctx = np.asarray(context, dtype=np.uint32)
    pred = None if prediction is None else np.asarray(list(prediction) + [0], dtype=np.uint32)   # + [0]: a valid pointer for an empty one
    out = np.full(16, 0xFFFFFFFF, dtype=np.uint32)
    n = C.c_size_t(99)
    rc = lib.aha_hip_spec_propose(C.byref(cs), ctx.ctypes.data, ctx.size, n_prompt, None if pred is None else pred.ctypes.data,
                                  0 if prediction is None else len(prediction), out.ctypes.data, C.byref(n))
    assert rc == 0, lib.aha_hip_last_error()
    assert n.value <= spec.max_draft and (out[n.value:] == 0xFFFFFFFF).all()
    return [int(t) for t in out[:n.value]]


# (name, spec, context, n_prompt, prediction, expected draft) -- the expected drafts are worked out by hand from the three rules
GOLDEN = [
    # rule 1: generated [7, 8] == p[0:2] -> p[2:2+3]
    ("aligned prediction", SpecConfig(3, 1, 3), [1, 2, 3, 7, 8], 3, [7, 8, 9, 10, 11, 12], [9, 10, 11]),
    # rule 1 at the end of the prediction: fewer than D left
    ("aligned, tail of the prediction", SpecConfig(4, 1, 3), [1, 2, 3, 7, 8], 3, [7, 8, 9], [9]),
    # rule 1 exhausted (t == |p|), no n-gram of c's tail inside p with a successor, no repeat in c -> nothing
    ("aligned but exhausted, nothing else", SpecConfig(4, 1, 2), [1, 2, 3, 7, 8], 3, [7, 8], []),
    # rule 2: generated [5] != p[0]; k = 2: s = [4, 5] found in p at i = 1 -> p[3:3+2]
    ("n-gram in the prediction", SpecConfig(2, 1, 2), [9, 4, 5], 2, [0, 4, 5, 6, 7, 8], [6, 7]),
    # rule 2 takes the EARLIEST match: s = [5] (k = 1) occurs at i = 1 and i = 3 -> p[2:...]
    ("earliest match in the prediction", SpecConfig(2, 1, 1), [9, 5], 1, [0, 5, 6, 5, 7], [6, 5]),
    # rule 2: a match that ends the prediction (i + k == |p|) has no successor and is skipped; k = 1, s = [7]: only at i = 2 = |p| - 1
    # -> rule 3 on c = [7, 3, 7]: s = [7], latest i < 2 is 0 -> c[1:min(1 + 2, 3)] = [3, 7]
    ("prediction match without a successor falls through", SpecConfig(2, 1, 1), [7, 3, 7], 2, [1, 2, 7], [3, 7]),
    # rule 2 prefers the longer n-gram (generated [3] != p[0:1] = [7]): k = 2, s = [2, 3] at i = 4 -> [9]; the k = 1 match of [3] at i = 1
    # would have given [8]
    ("longer n-gram first", SpecConfig(1, 1, 2), [1, 2, 3], 2, [7, 3, 8, 0, 2, 3, 9], [9]),
    # rule 3: no prediction; k = 2: s = [1, 2] occurs at i = 0 and i = 3 (< n - k = 6) -> LATEST i = 3 -> c[5:min(5 + 4, 8)] = [6, 1, 2]
    ("prompt lookup, latest match, clipped by the context", SpecConfig(4, 1, 2), [1, 2, 5, 1, 2, 6, 1, 2], 8, None, [6, 1, 2]),
    # the same with D = 1: the draft is clipped by D
    ("prompt lookup clipped by D", SpecConfig(1, 1, 2), [1, 2, 5, 1, 2, 6, 1, 2], 8, None, [6]),
    # earliest vs latest on the same data: prediction = the context itself, generated misaligned -> rule 2 takes i = 0 -> p[2:2+2] = [5, 1]
    ("tie: prediction side takes the earliest", SpecConfig(2, 2, 2), [1, 2, 5, 1, 2, 6, 1, 2], 7, [1, 2, 5, 1, 2, 6, 1, 2], [5, 1]),
    # ngram_max larger than the context: k = 8 .. 3 are skipped, k = 1: s = [4], latest i < 1 -> i = 0 -> c[1:2] = [4]
    ("ngram_max larger than the context", SpecConfig(3, 1, 8), [4, 4], 2, None, [4]),
    # a one-token context has nothing to look up
    ("one-token context", SpecConfig(3, 1, 8), [4], 1, None, []),
    # an empty prediction is no prediction: prompt lookup; k = 1, s = [3], latest i < 3 is 1 -> c[2:4] = [9, 3]
    ("empty prediction", SpecConfig(5, 1, 1), [2, 3, 9, 3], 4, [], [9, 3]),
    # a draft clipped by D under rule 1
    ("aligned clipped by D", SpecConfig(2, 1, 3), [1, 7], 1, [7, 8, 9, 10], [8, 9]),
    # D = 15, the longest draft
    ("fifteen", SpecConfig(15, 1, 1), [1, 50], 1, list(range(50, 90)), list(range(51, 66))),
    # speculation off
    ("max_draft 0", SpecConfig(0, 1, 3), [1, 2, 1, 2], 4, [1, 2, 3], []),
    # the prediction's first token is wrong, the rest right: rule 1 fails, k = 1: s = [8] at i = 1 -> [9, 10]
    ("misaligned prediction recovers through its n-grams", SpecConfig(2, 1, 3), [1, 2, 3, 7, 8], 3, [6, 8, 9, 10], [9, 10]),
]


@pytest.mark.parametrize("case", GOLDEN, ids=[g[0] for g in GOLDEN])
def test_proposer_golden_cases(hip_lib, case):
    _, spec, ctx, n_prompt, pred, want = case
    assert propose(spec, ctx, n_prompt, pred) == want
    assert c_propose(hip_lib, spec, ctx, n_prompt, pred) == want


def test_proposer_equals_the_python_definition_on_random_cases(hip_lib):
    rng = np.random.default_rng(20260)
    n_nonempty, rules = 0, set()
    for it in range(4000):
        alpha = int(rng.integers(2, 6))   # small alphabet: matches are frequent
        n = int(rng.integers(1, 40))
        n_prompt = int(rng.integers(0, n + 1))
        ctx = rng.integers(0, alpha, n).tolist()
        lo = int(rng.integers(1, 9))
        spec = SpecConfig(int(rng.integers(0, 16)), lo, int(rng.integers(lo, 9)))
        kind = it % 4
        if kind == 0:
            pred = None
        elif kind == 1:     # aligned with what was generated, then random
            pred = ctx[n_prompt:] + rng.integers(0, alpha, int(rng.integers(0, 12))).tolist()
        elif kind == 2:
            pred = rng.integers(0, alpha, int(rng.integers(0, 30))).tolist()
        else:               # aligned but for one corrupted position
            pred = ctx[n_prompt:] + rng.integers(0, alpha, int(rng.integers(1, 12))).tolist()
            pred[int(rng.integers(0, len(pred)))] = alpha
        want = propose(spec, ctx, n_prompt, pred)
        got = c_propose(hip_lib, spec, ctx, n_prompt, pred)
        assert got == want, (spec, ctx, n_prompt, pred)
        n_nonempty += bool(want)
    assert n_nonempty > 1500   # the cases exercise the rules, they do not all come out empty


def test_row_budget():
    assert [row_budget(n) for n in (1, 31, 32, 33, 64, 65)] == [32, 32, 32, 64, 64, 96]


# ---- invalid configurations: before any device work (no model, no GPU) ---------------------------------------------------------------
def _spec_call(lib, spec, predictions=None, prediction_lens=None):
    return lib.aha_hip_generate_batch_spec(None, None, None, 0, 0, 0, spec, predictions, prediction_lens, None, None, None, None, None, None)


@pytest.mark.parametrize("fields, message", [
    ((-1, 1, 3), b"max_draft must be in 0..15"),
    ((16, 1, 3), b"max_draft must be in 0..15"),
    ((4, 0, 3), b"n-gram bounds must satisfy 1 <= ngram_min <= ngram_max <= 8"),
    ((4, 3, 2), b"n-gram bounds must satisfy 1 <= ngram_min <= ngram_max <= 8"),
    ((4, 1, 9), b"n-gram bounds must satisfy 1 <= ngram_min <= ngram_max <= 8"),
])
def test_invalid_configs(hip_lib, fields, message):
    from aha_amd import _lib
    cs = _lib.SpecConfig(*fields)
    assert _spec_call(hip_lib, C.byref(cs)) == AHA_ERR_INVALID
    assert message in hip_lib.aha_hip_last_error() and b"generate_batch_spec" in hip_lib.aha_hip_last_error()
    out, n = np.zeros(16, np.uint32), C.c_size_t(0)
    ctx = np.asarray([1, 2], np.uint32)
    assert hip_lib.aha_hip_spec_propose(C.byref(cs), ctx.ctypes.data, 2, 2, None, 0, out.ctypes.data, C.byref(n)) == AHA_ERR_INVALID
    assert message in hip_lib.aha_hip_last_error()


def test_invalid_arguments(hip_lib):
    from aha_amd import _lib
    good = _lib.SpecConfig(4, 1, 3)
    assert _spec_call(hip_lib, None) == AHA_ERR_INVALID
    assert b"null spec" in hip_lib.aha_hip_last_error()
    some = np.asarray([1, 2, 3], np.uint32)
    lens = np.asarray([3], np.uint64)
    for p, l in ((some.ctypes.data, None), (None, lens.ctypes.data)):
        assert _spec_call(hip_lib, C.byref(good), p, l) == AHA_ERR_INVALID
        assert b"predictions and prediction_lens must both be set or both be null" in hip_lib.aha_hip_last_error()
    # a valid config gets as far as the model check
    assert _spec_call(hip_lib, C.byref(good)) == AHA_ERR_INVALID
    assert b"null model" in hip_lib.aha_hip_last_error()
    assert _spec_call(hip_lib, C.byref(good), some.ctypes.data, lens.ctypes.data) == AHA_ERR_INVALID
    assert b"null model" in hip_lib.aha_hip_last_error()
    # the proposer's own arguments
    out, n = np.zeros(16, np.uint32), C.c_size_t(0)
    assert hip_lib.aha_hip_spec_propose(C.byref(good), None, 0, 0, None, 0, out.ctypes.data, C.byref(n)) == AHA_ERR_INVALID
    assert hip_lib.aha_hip_spec_propose(C.byref(good), some.ctypes.data, 3, 4, None, 0, out.ctypes.data, C.byref(n)) == AHA_ERR_INVALID
    assert b"n_prompt > n_context" in hip_lib.aha_hip_last_error()
    assert hip_lib.aha_hip_spec_propose(None, some.ctypes.data, 3, 3, None, 0, out.ctypes.data, C.byref(n)) == AHA_ERR_INVALID
    with pytest.raises(ValueError):
        propose(SpecConfig(16, 1, 3), [1, 2], 2)
    with pytest.raises(ValueError):
        propose(SpecConfig(4, 2, 1), [1, 2], 2)


# ---- ISA ---------------------------------------------------------------------------------------------------------------------------
NEW_FAMILIES = ("kv_append_rows_kernel", "spec_accept_rows_kernel", "attn_decode_rows_kernel")


def _family(name):
    m = re.search(r"\d+([a-z_0-9]+?_kernel)", name)
    return m.group(1) if m else name


def test_spec_kernels_have_no_scratch_spills_or_flat_accesses(tmp_path):
    if not (os.path.exists(f"{LLVM}/llvm-objdump") and os.path.exists(f"{LLVM}/llvm-readelf")):
        pytest.skip("ROCm llvm tools not found")
    from aha_amd import build
    build.build()
    shutil.copy(os.path.join(ROOT, "aha_amd", "csrc", "libaha_hip.so"), tmp_path / "lib.so")
    subprocess.run([f"{LLVM}/llvm-objdump", "--offloading", "lib.so"], cwd=tmp_path, capture_output=True, check=True)
    objs = sorted(glob.glob(str(tmp_path / "lib.so.*gfx950")))
    assert objs
    meta, ops = {}, {}
    for o in objs:
        notes = subprocess.run([f"{LLVM}/llvm-readelf", "--notes", o], capture_output=True, text=True, check=True).stdout
        body = notes[notes.index("amdhsa.kernels:"):] if "amdhsa.kernels:" in notes else ""
        for item in re.split(r"\n  - ", body)[1:]:
            name = re.search(r"^\s*\.name:\s+(\S+)", item, re.M)
            if name and _family(name.group(1)) in NEW_FAMILIES:
                meta[name.group(1)] = {k: int(v) for k, v in re.findall(r"^\s{0,4}\.(\w+):\s+(\d+)\s*$", item, re.M)}
        dis = subprocess.run([f"{LLVM}/llvm-objdump", "-d", "--no-show-raw-insn", o], capture_output=True, text=True, check=True).stdout
        cur = None
        for line in dis.splitlines():
            m = re.match(r"^[0-9a-f]+ <(\S+)>:", line)
            if m:
                cur = m.group(1)
                continue
            if cur and _family(cur) in NEW_FAMILIES and line.split():
                ops.setdefault(cur, []).append(line.split()[0])
    assert sorted(_family(n) for n in meta) == sorted(NEW_FAMILIES), list(meta)
    assert sorted(_family(n) for n in ops) == sorted(NEW_FAMILIES), list(ops)
    for n, k in meta.items():
        assert k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0 and k["private_segment_fixed_size"] == 0, (n, k)
        assert k["vgpr_count"] <= 256, (n, k)
    for n, o in ops.items():
        bad = [x for x in o if x.startswith("scratch_") or x.startswith("flat_load") or
               (x.startswith("flat_") and _family(n) != "attn_decode_rows_kernel")]
        assert not bad, (n, bad[:5])
        stores = [x for x in o if x.startswith("global_store") or x.startswith("buffer_store")]
        assert stores, n   # the kernels write through the global address space
    # one wave per (row, kv head) / per 64 sequences
    assert all(k["max_flat_workgroup_size"] == 64 for n, k in meta.items() if _family(n) != "attn_decode_rows_kernel")
    # the attention launch of a draft-and-verify step is the batch attention without its append: it stores less, it is not longer
    rows = next(o for n, o in ops.items() if _family(n) == "attn_decode_rows_kernel")
    assert sum(x.startswith("v_mfma") for x in rows) == 64
