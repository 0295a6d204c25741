"""CPU tier: allowed-token masks (guided decoding) are wired through every layer -- header, exports, ctypes table, Rust shim -- the
packing and the guided-choice trie of aha_amd/guided.py do what they say, and the host sampler (aha_hip_sampler_set_mask / _plan /
_pick) follows the definition of include/aha_hip.h, restated here in numpy:

  z = the row after the repeat penalty and the addends; z_i = -inf for every id whose bit (i & 31 of word i >> 5) is clear; the sampler
  runs on z; RNG consumption per token is unchanged; bits at positions >= V are ignored.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

from test_generate_sampled_cpu import CppSampler
from test_logit_adjust_cpu import ADJUSTS, SAMPLERS, numpy_pick, set_adjust

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_ARGS = {"aha_hip_generate_batch_masked": 16, "aha_hip_engine_submit_masked": 11, "aha_hip_engine_set_mask": 4,
          "aha_hip_sample_rows_masked": 18, "aha_hip_sampler_set_mask": 3}
NINF = float("-inf")


def test_mask_symbols_in_every_layer(hip_lib):
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
    for wrapper in ("pub fn generate_batch_masked<", "pub fn submit_masked(", "pub fn set_mask(", "pub type AhaTokenMaskFn"):
        assert wrapper in src, wrapper
    # the callback type: six arguments in the header, the ctypes prototype and the shim
    cb = re.search(r"typedef int \(\*aha_token_mask_fn\)\(([^;]*)\);", header)
    assert cb and len(cb.group(1).split(",")) == 6
    assert len(_lib.TOKEN_MASK_FN._argtypes_) == 6 and _lib.TOKEN_MASK_FN._restype_ is C.c_int
    # the header states the definition and what is out of scope
    sec = header[header.index("guided decoding: per-step allowed-token masks"):header.index("int aha_hip_sampler_set_mask(")]
    for phrase in ("ceil(V / 32)", "bit i & 31 of word i >> 5", ">= V in the", "RNG consumption per token is unchanged", "from the raw logits",
                   "The first token is masked too", "Stop tokens are ordinary ids", "JSON-schema", "aha_hip_generate_batch_spec",
                   "aha_hip_sample_candidates", "tensor-parallel"):
        assert phrase in sec, phrase


# ---- guided.py ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V", [1, 31, 32, 33, 37, 4096, 151936])
def test_pack_unpack_round_trip(V):
    from aha_amd.guided import mask_words, pack_mask, unpack_mask
    g = np.random.default_rng(V)
    for ids in ([0], [V - 1], sorted({0, V - 1, V // 2}), sorted(set(g.integers(0, V, size=min(V, 300)).tolist())), list(range(V))):
        w = pack_mask(ids, V)
        assert w.dtype == np.uint32 and w.shape == (mask_words(V),) == ((V + 31) // 32,)
        assert unpack_mask(w, V).tolist() == ids
        for i in ids[:50]:
            assert (int(w[i >> 5]) >> (i & 31)) & 1
        assert sum(bin(int(x)).count("1") for x in w) == len(ids)     # nothing else is set, the bits past V included
        w2 = w.copy()
        if V % 32:
            w2[-1] |= np.uint32((0xffffffff << (V % 32)) & 0xffffffff)  # garbage past V is ignored
        assert unpack_mask(w2, V).tolist() == ids
    assert pack_mask([3, 3, 0] if V > 3 else [0, 0], V).tolist() == pack_mask([0, 3] if V > 3 else [0], V).tolist()
    assert unpack_mask(pack_mask([], V), V).size == 0
    for bad in ([V], [-1]):
        with pytest.raises(ValueError):
            pack_mask(bad, V)
    with pytest.raises(ValueError):
        unpack_mask(np.zeros(mask_words(V) + 1, np.uint32), V)


def test_choice_constraint_trie():
    from aha_amd.guided import ChoiceConstraint, unpack_mask
    V, stops = 100, [2, 3]
    c = ChoiceConstraint([[5, 6, 7], [5, 6], [5, 9], [40], [41, 42, 43, 44, 45, 46]], stops, V)
    allowed = lambda gen: unpack_mask(c(0, gen), V).tolist()
    assert allowed([]) == [5, 40, 41]                                # shared prefixes: one child per distinct first token
    assert allowed([5]) == [6, 9]
    assert allowed([5, 6]) == [2, 3, 7]                              # [5, 6] is a choice and a prefix of [5, 6, 7]: stop or go on
    assert allowed([5, 6, 7]) == [2, 3] and allowed([40]) == [2, 3] and allowed([5, 9]) == [2, 3]
    assert allowed([41, 42, 43]) == [44] and allowed([41, 42, 43, 44, 45, 46]) == [2, 3]
    assert c.allowed([5, 6]) == [2, 3, 7]
    assert c(0, [5]) is c(7, [5])                                     # no per-prompt state: one cached mask per node
    for left in ([6], [5, 7], [40, 2], [5, 6, 7, 8], [41, 42, 43, 44, 45, 46, 47]):
        with pytest.raises(ValueError, match="not a prefix of any choice"):
            c(0, left)
    # a stop id that is also a choice token is a token inside the choice and a stop at its end
    c2 = ChoiceConstraint([[2, 8]], [2], V)
    assert unpack_mask(c2(0, []), V).tolist() == [2] and unpack_mask(c2(0, [2]), V).tolist() == [8] and unpack_mask(c2(0, [2, 8]), V).tolist() == [2]
    for bad in (dict(choices=[], stop_ids=[2]), dict(choices=[[1], []], stop_ids=[2]), dict(choices=[[1]], stop_ids=[]),
                dict(choices=[[V]], stop_ids=[2])):
        with pytest.raises(ValueError):
            ChoiceConstraint(vocab_size=V, **bad)


# ---- the host sampler -----------------------------------------------------------------------------------------------------------------
def set_mask(lib, cpp, words):
    if words is None:
        return lib.aha_hip_sampler_set_mask(cpp.h, None, 0)
    w = np.ascontiguousarray(words, dtype=np.uint32)
    return lib.aha_hip_sampler_set_mask(cpp.h, w.ctypes.data, w.size)


def random_mask(g, V, density, garbage=True):
    """Packed words allowing about density * V ids (at least one), with every bit past V set when `garbage`."""
    from aha_amd.guided import pack_mask
    ids = np.flatnonzero(g.random(V) < density)
    if not ids.size:
        ids = np.asarray([int(g.integers(0, V))])
    w = pack_mask(ids.tolist(), V)
    if garbage and V % 32:
        w[-1] |= np.uint32((0xffffffff << (V % 32)) & 0xffffffff)
    return w, ids


def test_set_mask_argument_errors(hip_lib):
    from aha_amd import sampling as hs
    from aha_amd.guided import pack_mask
    V = 300
    cpp = CppSampler(hip_lib, hs.SamplingParams().to_c())
    try:
        assert hip_lib.aha_hip_sampler_set_mask(None, None, 0) == -1 and b"sampler_set_mask" in hip_lib.aha_hip_last_error()
        assert set_mask(hip_lib, cpp, np.zeros(10, np.uint32)) == -1 and b"allows no id" in hip_lib.aha_hip_last_error()
        w = pack_mask([4], V)
        assert hip_lib.aha_hip_sampler_set_mask(cpp.h, w.ctypes.data, 0) == -1
        assert cpp.plan(V, 0)[0] == 0                                  # a refused mask leaves the sampler as it was
        # a wrong length, and a mask whose only bits lie past V, are caught where the vocabulary is known: in pick
        x = np.zeros(V, np.float32)
        out = C.c_uint32()
        assert set_mask(hip_lib, cpp, pack_mask([4], V + 64)) == 0
        assert hip_lib.aha_hip_sampler_pick(cpp.h, None, None, 0, 0.0, 0.0, x.ctypes.data, V, None, 0, C.byref(out)) == -1
        assert b"words" in hip_lib.aha_hip_last_error()
        past = np.zeros((V + 31) // 32, np.uint32)
        past[-1] = np.uint32(1 << (V % 32))
        assert set_mask(hip_lib, cpp, past) == 0
        assert hip_lib.aha_hip_sampler_pick(cpp.h, None, None, 0, 0.0, 0.0, x.ctypes.data, V, None, 0, C.byref(out)) == -1
        assert b"allows no id below vocab_size" in hip_lib.aha_hip_last_error()
        assert set_mask(hip_lib, cpp, None) == 0 and cpp.pick(None, x, V, []) == 0
    finally:
        cpp.close()


def test_plan_asks_for_one_candidate_while_a_mask_is_set(hip_lib):
    from aha_amd import sampling as hs
    from aha_amd.guided import pack_mask
    V = 300
    cpp = CppSampler(hip_lib, hs.SamplingParams().to_c())            # ArgMax, no repeat penalty
    try:
        assert cpp.plan(V, 0)[0] == 0 and cpp.plan(V, 9)[0] == 0
        assert set_mask(hip_lib, cpp, pack_mask([5, 7], V)) == 0
        assert cpp.plan(V, 0) == (1, 0.0, 1.0, 0) and cpp.plan(V, 9)[0] == 1   # the first token too
        assert set_mask(hip_lib, cpp, None) == 0
        assert cpp.plan(V, 0)[0] == 0 and cpp.plan(V, 9)[0] == 0
    finally:
        cpp.close()
    cpp = CppSampler(hip_lib, hs.SamplingParams(0.7, top_k=20).to_c())   # a sampled row keeps its own k
    try:
        assert set_mask(hip_lib, cpp, pack_mask([5], V)) == 0
        assert cpp.plan(V, 3)[0] == 20
    finally:
        cpp.close()


def masked_numpy_pick(lp, pen, last_n, x, gen, adj, words):
    """numpy_pick of tests/test_logit_adjust_cpu.py with step 3b between the addends and the sampler."""
    from aha_amd import sampling as hs
    from oracle import sampling as osamp
    V = x.shape[0]
    p_eff, pctx = hs.penalty_context(pen, last_n, gen)
    y = osamp.apply_repeat_penalty(x, p_eff, pctx) if p_eff != 1.0 else x.copy()
    y = np.asarray(y, dtype=np.float32).copy()
    if adj is not None:
        from test_logit_adjust_cpu import addends
        ids, a = addends(adj["presence"], adj["frequency"], adj["bias"], gen, V)
        with np.errstate(invalid="ignore"):
            y[ids] = y[ids] + a
    ids = np.arange(V)
    y[~((words[ids >> 5] >> (ids & 31).astype(np.uint32)) & np.uint32(1)).astype(bool)] = -np.inf
    if lp.sampling.kind == "ArgMax":
        return int(np.argmax(y)), y
    w, keep = lp.weights_from_logits(y)
    pos = lp.draw(w)
    return (pos if keep is None else int(keep[pos])), y


@pytest.mark.parametrize("si", range(len(SAMPLERS)))
def test_pick_on_full_vectors_follows_the_definition(hip_lib, si):
    """The full-vector path against numpy and against sampling.apply_token_mask (the product mirror), a fresh mask every step, with and
    without an adjust; the RNG words are those of the same sampler without a mask."""
    from aha_amd import sampling as hs
    V, steps = 300, 30                                               # 300 % 32 != 0: the last word is partial
    for ai, adj in enumerate([None, ADJUSTS[3]]):
        g = np.random.default_rng(500 * si + ai)
        sp = hs.SamplingParams(**SAMPLERS[si], seed=91 + ai)
        lp = hs.get_logit_processor(sp.temperature, sp.top_p, sp.top_k, sp.seed)
        pen = 1.0 if sp.repeat_penalty is None else sp.repeat_penalty
        cpp, plain = CppSampler(hip_lib, sp.to_c()), CppSampler(hip_lib, sp.to_c())
        try:
            if adj is not None:
                assert set_adjust(hip_lib, cpp, **adj) == 0 and set_adjust(hip_lib, plain, **adj) == 0
            gen, differs = [], False
            for step in range(steps):
                x = (g.normal(0, 1.0, V) + 4.0 * (np.arange(V) % 37 == 0)).astype(np.float32)
                words, ids = random_mask(g, V, (0.4, 0.02, 1.0)[step % 3])
                if adj is not None:                                   # id 12 carries a -inf bias: allow 13 too, so a finite logit is left
                    words[0] |= np.uint32(1 << 13)
                    ids = np.union1d(ids, [13])
                assert set_mask(hip_lib, cpp, words) == 0
                want, z = masked_numpy_pick(lp, pen, sp.repeat_last_n, x, gen, adj, words)
                if adj is None:                                       # the mirror's own step 3b gives the same vector
                    p_eff, pctx = hs.penalty_context(pen, sp.repeat_last_n, gen)
                    from oracle import sampling as osamp
                    y = osamp.apply_repeat_penalty(x, p_eff, pctx) if p_eff != 1.0 else x
                    assert np.array_equal(hs.apply_token_mask(y, words).view(np.uint32), z.view(np.uint32))
                got = cpp.pick(None, x, V, gen)
                assert got == want and got in set(ids.tolist()), (si, ai, step, got, want)
                plain_tok = plain.pick(None, x, V, gen)
                assert cpp.words() == plain.words(), (si, ai, step)  # RNG consumption per token is unchanged
                differs |= plain_tok != got
                gen.append(got)
            assert differs, (si, ai)
        finally:
            cpp.close()
            plain.close()


def test_an_all_ones_mask_and_a_cleared_mask_change_nothing(hip_lib):
    from aha_amd import sampling as hs
    V = 300
    ones = np.full((V + 31) // 32, 0xffffffff, np.uint32)
    for kw in SAMPLERS:
        sp = hs.SamplingParams(**kw, seed=5)
        a, b = CppSampler(hip_lib, sp.to_c()), CppSampler(hip_lib, sp.to_c())
        try:
            g = np.random.default_rng(3)
            gen = []
            for step in range(20):
                assert set_mask(hip_lib, a, ones if step % 2 else None) == 0
                x = g.normal(0, 2.0, V).astype(np.float32)
                ta, tb = a.pick(None, x, V, gen), b.pick(None, x, V, gen)
                assert ta == tb and a.words() == b.words()
                gen.append(ta)
        finally:
            a.close()
            b.close()


def test_product_mirror_masks_the_full_vector():
    from aha_amd import sampling as hs
    from aha_amd.guided import pack_mask
    x = np.arange(40, dtype=np.float32)
    z = hs.apply_token_mask(x, pack_mask([3, 33], 40))
    assert z[3] == 3 and z[33] == 33 and np.isneginf(np.delete(z, [3, 33])).all() and x[0] == 0     # a copy: the input is untouched
    with pytest.raises(ValueError):
        hs.apply_token_mask(x, pack_mask([3], 100))
    with pytest.raises(ValueError):
        hs.apply_token_mask(x, np.asarray([0, 1 << 8], np.uint32))  # only a bit past V
    ctx = hs.SamplingParams().context(4, 8)
    assert ctx.token_mask is None


def test_engine_and_batch_argument_errors_that_need_no_gpu(hip_lib):
    """Null handles are refused before anything else is looked at."""
    w = np.ones(4, np.uint32)
    rid = C.c_uint64()
    assert hip_lib.aha_hip_engine_set_mask(None, 1, w.ctypes.data, 4) == -1 and b"engine_set_mask: null engine" in hip_lib.aha_hip_last_error()
    ids = np.asarray([1, 2], np.uint32)
    assert hip_lib.aha_hip_engine_submit_masked(None, ids.ctypes.data, 2, None, None, None, w.ctypes.data, 4, 4, -1, C.byref(rid)) == -1
    assert b"engine_submit_masked: null engine" in hip_lib.aha_hip_last_error()
    assert hip_lib.aha_hip_engine_submit_masked(None, ids.ctypes.data, 2, None, None, None, w.ctypes.data, 4, 4, 21, C.byref(rid)) == -1
    assert b"top_logprobs must be -1" in hip_lib.aha_hip_last_error()
    from aha_amd import _lib
    cb = _lib.TOKEN_MASK_FN(lambda *a: 0)
    lens, toks, n_out = np.asarray([2], np.uint64), np.zeros(4, np.uint32), np.zeros(1, np.uint64)
    rc = hip_lib.aha_hip_generate_batch_masked(None, ids.ctypes.data, lens.ctypes.data, 1, None, None, None, None, 4, 0, C.cast(cb, C.c_void_p), None,
                                               toks.ctypes.data, n_out.ctypes.data, None, None)
    assert rc == -1 and b"null model" in hip_lib.aha_hip_last_error()
    top = np.asarray([5], np.int32)
    rc = hip_lib.aha_hip_generate_batch_masked(None, ids.ctypes.data, lens.ctypes.data, 1, None, None, None, top.ctypes.data, 4, 0,
                                               C.cast(cb, C.c_void_p), None, toks.ctypes.data, n_out.ctypes.data, None, None)
    assert rc == -1 and b"generate_batch_masked: top_logprobs and logprobs_out" in hip_lib.aha_hip_last_error()
    # sample_rows_masked: null mask_rows, and a row that names a mask without a masks buffer (checked before any device work)
    k, t, p, off = np.asarray([1], np.int32), np.zeros(1, np.float32), np.ones(1, np.float32), np.zeros(2, np.uint64)
    fake = C.c_void_p(256)                                            # never dereferenced: the checks come first
    args = (fake, 64, 1, 64, k.ctypes.data, t.ctypes.data, p.ctypes.data, None, off.ctypes.data, None, None, None)
    assert hip_lib.aha_hip_sample_rows_masked(*args, None, None, fake, fake, fake, None) == -1
    assert b"sample_rows_masked: null mask_rows" in hip_lib.aha_hip_last_error()
    mr = np.asarray([0], np.int32)
    assert hip_lib.aha_hip_sample_rows_masked(*args, None, mr.ctypes.data, fake, fake, fake, None) == -1
    assert b"sample_rows_masked: row 0" in hip_lib.aha_hip_last_error()
