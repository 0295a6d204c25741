"""CPU tier: batched sampled generation (aha_hip_generate_batch_sampled) is wired through every layer -- public header, exported symbols,
ctypes table and struct mirror, Rust shim -- its argument checks run before any device work, the C++ sampler (aha_hip_sampler_*) picks
the tokens of the Python specification (aha_amd/sampling.py) and consumes its RNG stream alike, and the batched candidate kernels ship in
the gfx950 code object without flat loads, scratch or spills."""
import ctypes as C
import glob
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LLVM = "/opt/rocm/lib/llvm/bin"
NEW = {"aha_hip_generate_batch_sampled": 10, "aha_hip_sample_rows": 13, "aha_hip_sampler_create": 2, "aha_hip_sampler_destroy": 1,
       "aha_hip_sampler_plan": 7, "aha_hip_sampler_pick": 11, "aha_hip_sampler_rng_words": 1}


def test_generate_sampled_symbols_in_every_layer(hip_lib):
    from aha_amd import _lib
    header = open(os.path.join(ROOT, "include", "aha_hip.h")).read()
    assert re.search(r"typedef struct aha_sampling_params \{\s*float temperature;\s*float top_p;\s*int32_t top_k;\s*float repeat_penalty;"
                     r"\s*int32_t repeat_last_n;\s*uint32_t flags;\s*uint64_t seed;\s*\} aha_sampling_params;", header)
    assert re.search(r"int aha_hip_generate_batch_sampled\(aha_model\* m, const uint32_t\* input_ids, const size_t\* seq_lens, size_t n_seqs,"
                     r"\s+const aha_sampling_params\* params, size_t max_new, size_t max_tokens_per_pass,"
                     r"\s+uint32_t\* tokens_out, size_t\* n_out, float\* step_logits_out\);", header)
    for name, nargs in NEW.items():
        assert re.search(rf"\b{name}\(", header), name
        assert hasattr(hip_lib, name), name
        assert len(_lib.SIGNATURES[name][1]) == nargs, name
    # the ctypes mirror: aha_sampling_params is 5 four-byte fields, a flags word and a u64 seed
    assert [f[0] for f in _lib.SamplingParams._fields_] == ["temperature", "top_p", "top_k", "repeat_penalty", "repeat_last_n", "flags", "seed"]
    assert C.sizeof(_lib.SamplingParams) == 32 and _lib.SamplingParams.seed.offset == 24
    src = open(os.path.join(ROOT, "rust", "aha-hip", "src", "lib.rs")).read()
    m = re.search(r"#\[repr\(C\)\]\s*#\[derive\(Debug, Clone, Copy\)\]\s*pub struct AhaSamplingParams \{(.*?)\}", src, re.S)
    assert m
    assert re.findall(r"pub (\w+):", m.group(1)) == [f[0] for f in _lib.SamplingParams._fields_]
    assert re.findall(r"pub \w+: (\w+),", m.group(1)) == ["f32", "f32", "i32", "f32", "i32", "u32", "u64"]
    ext = src[src.index('extern "C" {'):]
    ext = ext[:ext.index("\n    }\n")]
    for name in NEW:
        assert re.search(rf"pub fn {name}\(", ext), name
    assert re.search(r"pub fn aha_hip_generate_batch_sampled\(\s*m: \*mut AhaModel,\s*ids: \*const u32,\s*seq_lens: \*const usize,"
                     r"\s*n_seqs: usize,\s*params: \*const AhaSamplingParams,\s*max_new: usize,\s*max_tokens_per_pass: usize,"
                     r"\s*tokens_out: \*mut u32,\s*n_out: \*mut usize,\s*step_logits_out: \*mut f32,?\s*\) -> i32;", ext)
    assert re.search(r"pub fn generate_batch_sampled\(\s*&mut self,\s*prompts: &\[&\[u32\]\],\s*params: &\[sys::AhaSamplingParams\],", src)


def _params(**kw):
    from aha_amd import sampling as hs
    return hs.SamplingParams(**kw).to_c()


def test_sampling_params_defaults_follow_the_reference():
    from aha_amd import sampling as hs
    p = hs.SamplingParams(0.6, 0.95, 20)
    assert p.repeat_last_n == 64 and p.seed == 299792458 and p.repeat_penalty is None
    c = p.to_c()
    assert c.flags == 3 and c.top_k == 20 and c.repeat_penalty == 1.0 and c.seed == 299792458
    assert abs(c.temperature - 0.6) < 1e-7 and abs(c.top_p - 0.95) < 1e-7
    assert hs.SamplingParams().to_c().flags == 0


def test_invalid_arguments_fail_before_device_work(hip_lib):
    """No GPU here: every call below must be refused on its arguments alone."""
    from aha_amd import _lib
    ids = (C.c_uint32 * 2)(1, 2)
    lens = (C.c_size_t * 1)(2)
    toks = (C.c_uint32 * 4)()
    n_out = (C.c_size_t * 1)()
    gen = hip_lib.aha_hip_generate_batch_sampled
    assert gen(None, ids, lens, 1, None, 4, 0, toks, n_out, None) == -1
    assert b"null params" in hip_lib.aha_hip_last_error()
    bad = [_params(temperature=0.7, top_k=1), _params(temperature=float("nan")), _params(temperature=0.7, repeat_penalty=0.0),
           _params(temperature=0.7, top_p=float("nan"))]
    bad[0].top_k = 0
    c = _params(temperature=0.7)
    c.repeat_last_n = -1
    bad.append(c)
    for p in bad:
        arr = (_lib.SamplingParams * 1)(p)
        assert gen(None, ids, lens, 1, arr, 4, 0, toks, n_out, None) == -1
        assert b"params of sequence 0" in hip_lib.aha_hip_last_error()
        h = C.c_void_p()
        assert hip_lib.aha_hip_sampler_create(C.byref(p), C.byref(h)) == -1 and not h.value
    good = (_lib.SamplingParams * 1)(_params(temperature=0.7, top_k=20, top_p=0.9))
    assert gen(None, ids, lens, 1, good, 4, 0, toks, n_out, None) == -1
    assert b"null model" in hip_lib.aha_hip_last_error()
    assert hip_lib.aha_hip_sampler_create(None, None) == -1
    assert hip_lib.aha_hip_sample_rows(None, 0, 0, 0, None, None, None, None, None, None, None, None, None) == -1
    assert hip_lib.aha_hip_sampler_pick(None, None, None, 0, 0.0, 0.0, None, 4, None, 0, None) == -1
    assert hip_lib.aha_hip_sampler_plan(None, 4, 0, None, None, None, None) == -1


# ---- the C++ sampler against the specification --------------------------------------------------------------------------------
class CppSampler:
    def __init__(self, lib, params):
        self.lib, self.h = lib, C.c_void_p()
        assert lib.aha_hip_sampler_create(C.byref(params), C.byref(self.h)) == 0

    def plan(self, V, n_gen):
        k, t, p, n = C.c_int32(), C.c_float(), C.c_float(), C.c_size_t()
        assert self.lib.aha_hip_sampler_plan(self.h, V, n_gen, C.byref(k), C.byref(t), C.byref(p), C.byref(n)) == 0
        return k.value, t.value, p.value, n.value

    def pick(self, cands, logits, V, generated):
        g = np.ascontiguousarray(generated, dtype=np.uint32)
        out = C.c_uint32()
        if cands is None:
            vals = idx = None
            k, mx, se = 0, 0.0, 0.0
        else:
            v, i, mx, se = cands
            vals, idx, k = np.ascontiguousarray(v, np.float32), np.ascontiguousarray(i, np.uint32), len(v)
        rc = self.lib.aha_hip_sampler_pick(self.h, None if vals is None else vals.ctypes.data, None if idx is None else idx.ctypes.data, k,
                                           float(mx), float(se), None if logits is None else logits.ctypes.data, V,
                                           g.ctypes.data if g.size else None, g.size, C.byref(out))
        if rc == -1 and b"WeightedIndex" in self.lib.aha_hip_last_error():
            return "error"      # the crate's Err (e.g. every weight zeroed by a top-p <= 0 over the full vector)
        assert rc in (0, 1), self.lib.aha_hip_last_error()
        return None if rc == 1 else int(out.value)

    def words(self):
        return int(self.lib.aha_hip_sampler_rng_words(self.h))

    def close(self):
        self.lib.aha_hip_sampler_destroy(self.h)


def candidates(pen_logits, k, temperature):
    """What the device candidate step returns for penalised logits (sumexp rounded to f32 as the device hands it over)."""
    from oracle import sampling as osamp
    vals, idx, mx, se = osamp.topk_candidates(pen_logits, k, temperature)
    return vals, idx, np.float32(mx), np.float32(se)


def mirror_pick(lp, repeat_penalty, repeat_last_n, logits, generated):
    """sampling.sample_and_push on host logits: the device half replaced by `candidates`, the draws counted."""
    from aha_amd import sampling as hs
    from aha_amd._lib import AhaHipError
    V = logits.shape[0]
    draws = [0]
    orig = lp.draw

    def counted(w):
        r = orig(w)
        draws[0] += 1
        return r
    lp.draw = counted
    pen, pctx = hs.penalty_context(repeat_penalty, repeat_last_n, generated)
    pl = logits.copy()
    if pen != 1.0:
        seen = set()
        for t in pctx:
            if t not in seen and 0 <= t < V:
                pl[t] = pl[t] / np.float32(pen) if pl[t] >= 0 else pl[t] * np.float32(pen)
            seen.add(t)
    kind = lp.sampling.kind
    cands = None
    if kind == "ArgMax" and pen == 1.0:
        token = int(np.argmax(logits))
        k = 0
    else:
        k = 1 if kind == "ArgMax" else lp.candidates_needed(V)
        token = None
        if k:
            cands = candidates(pl, k, lp.sampling.temperature if kind != "ArgMax" else 0.0)
            vals, idx, mx, se = cands
            if kind == "ArgMax":
                token = int(idx[0])
            else:
                w = lp.weights_from_candidates(vals, mx, se, idx)
                if w is not None:
                    token = hs.draw_from_candidates(lp, w, idx)
        if token is None:
            w, ids = lp.weights_from_logits(pl)
            try:
                pos = lp.draw(w)
                token = pos if ids is None else int(ids[pos])
            except AhaHipError:
                token = "error"
    lp.draw = orig
    return token, draws[0], k, cands, (pen, len(pctx))


def random_case(g, i):
    V = int(g.choice([5, 17, 64, 65, 100, 300, 1000]))
    t = float(g.choice([0.0, -1.0, 1e-8, 0.3, 0.6, 1.0, 2.0, 8.0]))
    top_p = [None, -0.1, 0.0, 0.3, 0.9, 0.95, 1.0, 1.2, float(g.uniform(0, 1))][int(g.integers(0, 9))]
    top_k = [None, 1, 5, 20, 64, 65, 100, V, V + 5][int(g.integers(0, 9))]
    pen = float(g.choice([1.0, 1.0, 1.1, 1.5, 0.8]))
    last_n = int(g.choice([0, 1, 8, 64]))
    style = i % 4
    if style == 0:
        logits = g.normal(0, 3, V)
    elif style == 1:
        logits = np.round(g.normal(0, 2, V) * 2) / 2           # many exact ties
    elif style == 2:
        logits = g.normal(0, 0.05, V)                           # flat: wide nuclei, fallbacks
    else:
        logits = np.full(V, 0.5) + (g.random(V) < 0.1) * 3.0    # tied probabilities, a few leaders
    logits = logits.astype(np.float32)
    gen = [int(x) for x in g.integers(0, V + 3 if i % 7 == 0 else V, size=int(g.integers(0, 80)))]
    return V, t, top_p, top_k, pen, last_n, logits, gen


def check_case(hip_lib, V, t, top_p, top_k, pen, last_n, logits, gen, seed):
    from aha_amd import sampling as hs
    sp = hs.SamplingParams(t, top_p, top_k, pen, last_n, seed)
    lp = hs.get_logit_processor(t, top_p, top_k, seed)
    cpp = CppSampler(hip_lib, sp.to_c())
    try:
        for step in range(3):   # the stream carries over between tokens
            want, draws, k, cands, (p_eff, n_ctx) = mirror_pick(lp, pen, last_n, logits, gen)
            pk, pt, pp, pn = cpp.plan(V, len(gen))
            assert (pk, pp, pn) == (k, np.float32(p_eff), n_ctx), (pk, pp, pn, k, p_eff, n_ctx)
            before = cpp.words()
            got = cpp.pick(cands, None, V, gen) if cands is not None else None
            if got is None:
                got = cpp.pick(cands, logits, V, gen)
            assert got == want, (V, t, top_p, top_k, pen, last_n, step)
            assert cpp.words() - before == draws, (V, t, top_p, top_k, step)
            if want == "error":
                break
            gen = gen + [want]
            logits = np.roll(logits, 3)
    finally:
        cpp.close()


def test_cpp_sampler_matches_the_specification_on_random_cases(hip_lib):
    g = np.random.default_rng(1234)
    for i in range(1500):
        check_case(hip_lib, *random_case(g, i), seed=int(g.integers(0, 2 ** 63)))


def test_cpp_sampler_edge_cases(hip_lib):
    """The cases the random sweep reaches only by luck: every Sampling kind, p at and beyond its bounds, a top-p cut on the last
    candidate (full-vector fallback), k > 64 and k >= V (full vector), tied probabilities."""
    from aha_amd import sampling as hs
    g = np.random.default_rng(99)
    flat = (g.normal(0, 0.02, 300)).astype(np.float32)
    tied = np.repeat(np.float32([2.0, 1.0, 0.0]), [10, 40, 50])
    for logits in (flat, tied, g.normal(0, 2, 1000).astype(np.float32)):
        V = logits.size
        for t in (0.0, 0.7, 1.5):
            for top_p in (None, -1.0, 0.0, 0.5, 0.95, 1.0, 2.0):
                for top_k in (None, 1, 20, 64, 65, V - 1, V, V + 1):
                    for pen, last_n in ((1.0, 64), (1.3, 4), (0.7, 0)):
                        check_case(hip_lib, V, t, top_p, top_k, pen, last_n, logits, [1, 2, 2, 3, V - 1], seed=7)
    # a TopP whose nucleus ends exactly on the 64th candidate: the candidates cannot decide, the full vector must
    logits = g.normal(0, 0.01, 500).astype(np.float32)
    vals, idx, mx, se = candidates(logits, 64, 1.0)
    prs = (np.exp((vals - mx) * np.float32(1.0), dtype=np.float32) / se).astype(np.float32)
    cs = np.cumsum(prs.astype(np.float64))
    p = float((cs[62] + cs[63]) / 2)
    lp = hs.get_logit_processor(1.0, p, None, 5)
    assert lp.weights_from_candidates(vals, mx, se, idx) is None
    cpp = CppSampler(hip_lib, hs.SamplingParams(1.0, p, None, seed=5).to_c())
    try:
        assert cpp.pick((vals, idx, mx, se), None, 500, []) is None and cpp.words() == 0   # asks for the logits, RNG untouched
        assert cpp.pick((vals, idx, mx, se), logits, 500, []) == mirror_pick(lp, 1.0, 64, logits, [])[0] and cpp.words() == 1
    finally:
        cpp.close()
    check_case(hip_lib, 500, 1.0, p, None, 1.0, 64, logits, [], seed=5)
    # a nucleus inside the candidates: decided without the logits
    p2 = float((cs[9] + cs[10]) / 2)
    cpp = CppSampler(hip_lib, hs.SamplingParams(1.0, p2, None, seed=5).to_c())
    try:
        assert cpp.pick((vals, idx, mx, se), None, 500, []) is not None and cpp.words() == 1
    finally:
        cpp.close()


def test_cpp_sampler_argmax_draws_nothing(hip_lib):
    from aha_amd import sampling as hs
    logits = np.float32([0.5, 3.0, 3.0, -1.0])
    cpp = CppSampler(hip_lib, hs.SamplingParams(0.0, 0.9, 5, 1.0, seed=1).to_c())
    try:
        assert cpp.plan(4, 3) == (0, 0.0, 1.0, 0)                   # greedy: the forward's argmax decides, no candidate step
        assert cpp.pick(None, logits, 4, [1, 1, 1]) == 1 and cpp.words() == 0
    finally:
        cpp.close()
    cpp = CppSampler(hip_lib, hs.SamplingParams(0.0, None, None, 2.0, 2, seed=1).to_c())
    try:
        assert cpp.plan(4, 3) == (1, 0.0, 2.0, 2)                   # greedy with a penalty: one candidate
        assert cpp.pick(None, logits, 4, [0, 1, 1]) == 2 and cpp.words() == 0
    finally:
        cpp.close()


# ---- code object ----------------------------------------------------------------------------------------------------------------
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


FAMILIES = ("topk_rows_stage1_kernel", "topk_rows_stage2a_kernel", "topk_rows_stage2b_kernel")


def _family(name):
    m = re.search(r"\d+([a-z_0-9]+?_kernel)", name)
    return m.group(1) if m else name


def test_sample_rows_kernels_have_no_flat_loads_scratch_or_spills(tmp_path):
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
    for n, k in meta.items():
        assert k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0 and k["private_segment_fixed_size"] == 0, (n, k)
        assert k["vgpr_count"] <= 128, (n, k)
    bad, seen = {}, set()
    for o in objs:
        dis = subprocess.run([f"{LLVM}/llvm-objdump", "-d", "--no-show-raw-insn", o], capture_output=True, text=True, check=True).stdout
        cur = None
        for line in dis.splitlines():
            m = re.match(r"^[0-9a-f]+ <(\S+)>:", line)
            if m:
                cur = m.group(1)
                continue
            if not cur or _family(cur) not in FAMILIES:
                continue
            seen.add(_family(cur))
            op = line.split()[0] if line.split() else ""
            if op.startswith("flat_") or op.startswith("scratch_"):
                bad.setdefault(cur, []).append(op)
    assert seen == set(FAMILIES) and not bad, bad
