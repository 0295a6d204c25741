"""CPU tier: logit_bias, presence_penalty and frequency_penalty (aha_logit_adjust) are wired through every layer -- header, exports,
ctypes table, Rust shim, struct layout -- and the host sampler (aha_hip_sampler_set_adjust / _plan / _pick / _adjust_list) follows the
definition of include/aha_hip.h, restated here in numpy:

  y = x after the repeat penalty; c_i = occurrences of i in ALL generated tokens; for every id with b_i != 0 or c_i > 0
  a_i = f32(f64(b_i) - f64(frequency) * c_i - f64(presence) * [c_i > 0]); z_i = y_i + a_i in f32; the sampler runs on z.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

from test_generate_sampled_cpu import CppSampler

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_ARGS = {"aha_hip_generate_batch_adjusted": 14, "aha_hip_engine_submit_adjusted": 9, "aha_hip_sample_rows_adjusted": 16,
          "aha_hip_sampler_set_adjust": 2, "aha_hip_sampler_adjust_list": 8}
NINF = float("-inf")


def test_adjust_symbols_in_every_layer(hip_lib):
    from aha_amd import _lib
    header = open(os.path.join(ROOT, "include", "aha_hip.h")).read()
    src = open(os.path.join(ROOT, "rust", "aha-hip", "src", "lib.rs")).read()
    ext = src[src.index('extern "C" {'):]
    ext = ext[:ext.index("\n    }\n")]
    for name, n in N_ARGS.items():
        decl = re.search(r"\nint %s\(([^;]*)\);" % name, header)
        assert decl, f"{name} is not declared in include/aha_hip.h"
        assert len(decl.group(1).split(",")) == n, name
        assert hasattr(hip_lib, name), f"{name} is not exported"
        restype, args = _lib.SIGNATURES[name]
        assert restype is C.c_int and len(args) == n, name
        rdecl = re.search(r"pub fn %s\(([^;]*)\) -> i32;" % name, ext)
        assert rdecl, f"{name} is not declared in the Rust shim"
        assert len([a for a in rdecl.group(1).split(",") if a.strip()]) == n, name
    for wrapper in ("pub fn generate_batch_adjusted(", "pub fn submit_adjusted(", "pub struct LogitAdjust"):
        assert wrapper in src, wrapper
    assert re.search(r"#define AHA_MAX_LOGIT_BIAS 1024\b", header) and _lib.AHA_MAX_LOGIT_BIAS == 1024
    assert "pub const AHA_MAX_LOGIT_BIAS: usize = 1024;" in src
    # the header states the definition and what is out of scope
    sec = header[header.index("logit_bias, presence_penalty, frequency_penalty"):header.index("int aha_hip_sampler_adjust_list(")]
    for phrase in ("not windowed", "rounded once", "one f32 add", "from the raw x", "aha_hip_sample_candidates", "aha_hip_generate_batch_spec",
                   "allowed-token masks", "grammars", "context walk"):
        assert phrase in sec, phrase


def test_logit_adjust_layout_matches_header_and_rust():
    from aha_amd import _lib
    T = _lib.LogitAdjust
    assert C.sizeof(T) == 32
    assert [getattr(T, f).offset for f, _ in T._fields_] == [0, 4, 8, 16, 24]
    header = open(os.path.join(ROOT, "include", "aha_hip.h")).read()
    hbody = re.search(r"typedef struct aha_logit_adjust \{(.*?)\} aha_logit_adjust;", header, re.S).group(1)
    hfields = re.findall(r"^\s+[\w ]+?\*?\s*\*?(\w+);", hbody, re.M)
    assert hfields == [f for f, _ in T._fields_]
    src = open(os.path.join(ROOT, "rust", "aha-hip", "src", "lib.rs")).read()
    body = re.search(r"#\[repr\(C\)\]\s*(?:#\[derive\([^)]*\)\]\s*)?pub struct AhaLogitAdjust \{(.*?)\n    \}", src, re.S)
    assert body, "AhaLogitAdjust is not a #[repr(C)] struct in the Rust shim"
    rust_fields = re.findall(r"pub (\w+): ([^,]+),", body.group(1))
    assert [f for f, _ in rust_fields] == hfields
    assert [t.strip() for _, t in rust_fields] == ["f32", "f32", "*const u32", "*const f32", "usize"]


def test_sampling_params_positional_construction_is_unchanged():
    from aha_amd import sampling as hs
    sp = hs.SamplingParams(0.7, 0.9, 20, 1.1, 32, 5)
    assert (sp.temperature, sp.top_p, sp.top_k, sp.repeat_penalty, sp.repeat_last_n, sp.seed) == (0.7, 0.9, 20, 1.1, 32, 5)
    assert (sp.presence_penalty, sp.frequency_penalty, sp.logit_bias) == (0.0, 0.0, None) and not sp.adjust_active
    c = sp.to_c()
    assert (c.top_k, c.repeat_last_n, c.seed) == (20, 32, 5)
    adj, keep = hs.SamplingParams(presence_penalty=0.5, logit_bias={7: -1.5, 3: NINF}).adjust_to_c()
    assert adj.n_bias == 2 and adj.presence_penalty == 0.5 and adj.frequency_penalty == 0.0
    assert {int(adj.bias_ids[i]): float(adj.bias_vals[i]) for i in range(2)} == {7: -1.5, 3: NINF}
    assert hs.SamplingParams(logit_bias={1: 2.0}).adjust_active and hs.SamplingParams(frequency_penalty=0.1).adjust_active
    assert hs.SamplingParams().adjust_to_c()[0].n_bias == 0


# ---- the host sampler ------------------------------------------------------------------------------------------------------------
def make_adjust(presence=0.0, frequency=0.0, bias=None, n_bias=None, null_arrays=False):
    from aha_amd import _lib
    bias = bias or []
    ids = np.asarray([i for i, _ in bias], dtype=np.uint32)
    vals = np.asarray([b for _, b in bias], dtype=np.float32)
    n = len(bias) if n_bias is None else n_bias
    a = _lib.LogitAdjust(presence, frequency, None if null_arrays or not ids.size else ids.ctypes.data_as(C.POINTER(C.c_uint32)),
                         None if null_arrays or not vals.size else vals.ctypes.data_as(C.POINTER(C.c_float)), n)
    return a, (ids, vals)


def set_adjust(lib, cpp, **kw):
    a, keep = make_adjust(**kw)
    return lib.aha_hip_sampler_set_adjust(cpp.h, C.byref(a))


def adjust_list(lib, cpp, V, gen, cap=None):
    g = np.ascontiguousarray(gen, dtype=np.uint32)
    cap = 2048 if cap is None else cap
    ids, vals, n = np.zeros(max(cap, 1), np.uint32), np.zeros(max(cap, 1), np.float32), C.c_size_t()
    rc = lib.aha_hip_sampler_adjust_list(cpp.h, V, g.ctypes.data if g.size else None, g.size, ids.ctypes.data, vals.ctypes.data, cap, C.byref(n))
    return rc, ids[:n.value].copy() if rc == 0 else None, vals[:n.value].copy() if rc == 0 else None, n.value


def test_set_adjust_argument_errors(hip_lib):
    from aha_amd import sampling as hs
    cpp = CppSampler(hip_lib, hs.SamplingParams().to_c())
    try:
        bad = [dict(presence=float("nan")), dict(presence=float("inf")), dict(frequency=float("nan")), dict(frequency=NINF),
               dict(bias=[(i, 1.0) for i in range(1025)]), dict(bias=[(1, 1.0)], null_arrays=True), dict(bias=[(4, 1.0), (9, 0.5), (4, 2.0)]),
               dict(bias=[(2, float("nan"))]), dict(bias=[(2, float("inf"))])]
        for kw in bad:
            assert set_adjust(hip_lib, cpp, **kw) == -1, kw
            assert b"sampler_set_adjust" in hip_lib.aha_hip_last_error(), kw
            assert cpp.plan(300, 5)[0] == 0, kw                      # a refused adjust leaves the sampler as it was
        assert hip_lib.aha_hip_sampler_set_adjust(None, None) == -1
        assert set_adjust(hip_lib, cpp, bias=[(i, -1.0) for i in range(1024)]) == 0      # the limit itself
        assert set_adjust(hip_lib, cpp, bias=[(3, NINF), (1, 0.0)]) == 0
        rc, ids, vals, n = adjust_list(hip_lib, cpp, 300, [])
        assert rc == 0 and ids.tolist() == [3] and vals.tolist() == [NINF]               # a zero bias is no addend
        assert hip_lib.aha_hip_sampler_set_adjust(cpp.h, None) == 0 and cpp.plan(300, 5)[0] == 0
    finally:
        cpp.close()


def test_plan_asks_for_one_candidate_while_an_addend_is_live(hip_lib):
    from aha_amd import sampling as hs
    cpp = CppSampler(hip_lib, hs.SamplingParams().to_c())            # ArgMax, no repeat penalty
    try:
        assert cpp.plan(300, 0)[0] == 0 and cpp.plan(300, 9)[0] == 0
        assert set_adjust(hip_lib, cpp, presence=0.5) == 0
        assert cpp.plan(300, 0)[0] == 0                                # nothing generated, no bias: no addend yet
        assert cpp.plan(300, 1) == (1, 0.0, 1.0, 0)
        assert set_adjust(hip_lib, cpp, bias=[(5, 2.0)]) == 0
        assert cpp.plan(300, 0)[0] == 1
        assert set_adjust(hip_lib, cpp, bias=[(5, 0.0)]) == 0         # only a zero bias: no addend before a token exists
        assert cpp.plan(300, 0)[0] == 0
        assert set_adjust(hip_lib, cpp) == 0                          # inactive again
        assert cpp.plan(300, 0)[0] == 0 and cpp.plan(300, 9)[0] == 0
    finally:
        cpp.close()
    cpp = CppSampler(hip_lib, hs.SamplingParams(0.7, top_k=20).to_c())   # a sampled row keeps its own k
    try:
        assert set_adjust(hip_lib, cpp, frequency=1.0, bias=[(5, 2.0)]) == 0
        assert cpp.plan(300, 3)[0] == 20
    finally:
        cpp.close()


def addends(presence, frequency, bias, gen, V):
    """Step 2 of the definition: sorted ids and f32 addends."""
    b = {i: np.float32(v) for i, v in bias if np.float32(v) != 0}
    c = {}
    for t in gen:
        if t < V:
            c[t] = c.get(t, 0) + 1
    ids = sorted(set(b) | set(c))
    out = []
    for i in ids:
        a = np.float64(b.get(i, np.float32(0)))
        if i in c:
            a = a - np.float64(np.float32(frequency)) * np.float64(c[i]) - np.float64(np.float32(presence))
        out.append(np.float32(a))
    return np.asarray(ids, dtype=np.int64), np.asarray(out, dtype=np.float32)


def numpy_pick(lp, pen, last_n, x, gen, adj):
    """Steps 1-4 on a full vector: the oracle's penalty, the f32 add, then sampling.py's softmax / top-k / top-p and the draw."""
    from oracle import sampling as osamp
    from aha_amd import sampling as hs
    V = x.shape[0]
    p_eff, pctx = hs.penalty_context(pen, last_n, gen)
    y = osamp.apply_repeat_penalty(x, p_eff, pctx) if p_eff != 1.0 else x.copy()
    y = np.asarray(y, dtype=np.float32).copy()
    ids, a = addends(adj["presence"], adj["frequency"], adj["bias"], gen, V)
    with np.errstate(invalid="ignore"):
        y[ids] = y[ids] + a
    if lp.sampling.kind == "ArgMax":
        return int(np.argmax(y)), (ids, a)
    w, keep = lp.weights_from_logits(y)
    pos = lp.draw(w)
    return (pos if keep is None else int(keep[pos])), (ids, a)


SAMPLERS = [dict(), dict(temperature=0.0, repeat_penalty=1.3, repeat_last_n=5), dict(temperature=1.1), dict(temperature=0.8, top_k=20),
            dict(temperature=0.9, top_k=20, repeat_penalty=1.2, repeat_last_n=8), dict(temperature=1.0, top_p=0.9),
            dict(temperature=0.6, top_p=0.95, top_k=20), dict(temperature=0.7, top_p=0.5, top_k=40, repeat_penalty=0.8)]
ADJUSTS = [dict(presence=0.0, frequency=0.0, bias=[(7, 1.5), (299, -2.0), (0, NINF), (150, 100.0)]),
           dict(presence=0.75, frequency=0.0, bias=[]), dict(presence=0.0, frequency=2.0, bias=[]),
           dict(presence=-0.5, frequency=0.3, bias=[(11, 0.25), (12, NINF), (13, -0.125), (200, 3.0)])]


@pytest.mark.parametrize("si", range(len(SAMPLERS)))
def test_pick_on_full_vectors_follows_the_definition(hip_lib, si):
    from aha_amd import sampling as hs
    V, steps = 300, 40
    for ai, adj in enumerate(ADJUSTS):
        g = np.random.default_rng(100 * si + ai)
        sp = hs.SamplingParams(**SAMPLERS[si], seed=77 + ai)
        lp = hs.get_logit_processor(sp.temperature, sp.top_p, sp.top_k, sp.seed)
        plain_lp = hs.get_logit_processor(sp.temperature, sp.top_p, sp.top_k, sp.seed)
        pen = 1.0 if sp.repeat_penalty is None else sp.repeat_penalty
        cpp, plain = CppSampler(hip_lib, sp.to_c()), CppSampler(hip_lib, sp.to_c())
        try:
            assert set_adjust(hip_lib, cpp, **adj) == 0
            gen, differs = [], False
            for step in range(steps):
                # few distinct leaders, so that tokens repeat and the counts grow past 1
                x = (g.normal(0, 1.0, V) + 4.0 * (np.arange(V) % 37 == 0)).astype(np.float32)
                want, (ids, a) = numpy_pick(lp, pen, sp.repeat_last_n, x, gen, adj)
                rc, lids, lvals, n = adjust_list(hip_lib, cpp, V, gen)
                assert rc == 0 and np.array_equal(lids, ids) and np.array_equal(lvals.view(np.uint32), a.view(np.uint32)), (si, ai, step)
                got = cpp.pick(None, x, V, gen)
                assert got == want, (si, ai, step, got, want)
                # RNG words: those of the same sampler without an adjust
                plain_tok = plain.pick(None, x, V, gen)
                assert cpp.words() == plain.words(), (si, ai, step)
                differs |= plain_tok != got
                gen.append(got)
            assert differs, (si, ai)                                  # the adjust changed at least one pick
            assert max(np.bincount(gen)) > 1 or adj["bias"], (si, ai)
        finally:
            cpp.close()
            plain.close()
            del plain_lp


def test_an_inactive_adjust_is_no_adjust(hip_lib):
    from aha_amd import sampling as hs
    V = 300
    for kw in SAMPLERS:
        sp = hs.SamplingParams(**kw, seed=5)
        a, b = CppSampler(hip_lib, sp.to_c()), CppSampler(hip_lib, sp.to_c())
        try:
            assert set_adjust(hip_lib, a) == 0
            g = np.random.default_rng(3)
            gen = []
            for step in range(20):
                x = g.normal(0, 2.0, V).astype(np.float32)
                assert a.plan(V, len(gen)) == b.plan(V, len(gen))
                ta, tb = a.pick(None, x, V, gen), b.pick(None, x, V, gen)
                assert ta == tb and a.words() == b.words()
                gen.append(ta)
            assert adjust_list(hip_lib, a, V, gen)[3] == 0
        finally:
            a.close()
            b.close()


def test_adjust_list_counts_and_capacity(hip_lib):
    from aha_amd import sampling as hs
    cpp = CppSampler(hip_lib, hs.SamplingParams().to_c())
    try:
        assert set_adjust(hip_lib, cpp, presence=0.5, frequency=0.25, bias=[(9, 1.0), (2, -3.0)]) == 0
        gen = [5, 9, 5, 400, 5, 1]                                    # 400 >= V: ignored
        rc, ids, vals, n = adjust_list(hip_lib, cpp, 300, gen)
        assert rc == 0 and ids.tolist() == [1, 2, 5, 9]
        assert vals.tolist() == [np.float32(-0.75), np.float32(-3.0), np.float32(-1.25), np.float32(1.0 - 0.25 - 0.5)]
        rc, _, _, n = adjust_list(hip_lib, cpp, 300, gen, cap=3)
        assert rc == -1 and n == 4                                    # too small: the needed length is reported
        rc, ids, vals, n = adjust_list(hip_lib, cpp, 300, gen[:2])    # a shorter history: the counts start over
        assert rc == 0 and ids.tolist() == [2, 5, 9] and vals.tolist() == [np.float32(-3.0), np.float32(-0.75), np.float32(0.25)]
    finally:
        cpp.close()


def test_product_mirror_applies_the_addends():
    from aha_amd import sampling as hs
    ids, vals = hs.logit_addends(0.5, 0.25, {9: 1.0, 2: -3.0, 4: 0.0, 700: 1.0}, [5, 9, 5, 400, 5, 1], 300)
    want_ids, want = addends(0.5, 0.25, [(9, 1.0), (2, -3.0)], [5, 9, 5, 400, 5, 1], 300)
    assert np.array_equal(ids.astype(np.int64), want_ids) and np.array_equal(vals.view(np.uint32), want.view(np.uint32))
    ctx = hs.SamplingParams(presence_penalty=0.5, logit_bias={3: NINF}).context(4, 8)
    assert ctx.presence_penalty == 0.5 and ctx.logit_bias == {3: NINF}
