"""CPU tier of tests/test_spec_rows_gpu.py: the two test entries are in the header, the library and the ctypes table and refuse bad arguments
before any device work; the helpers of tests/spec_rows_ref.py against hand-written tables; fused_ref fed a run's tokens in sequence against
oracle.qwen3; and what the GPU tests' references can and cannot see (a leaked successor token, an accept rule that does not stop)."""
import ctypes as C
import os
import re
import sys

import torch

from oracle import qwen3 as oq
from oracle.numerics import Numerics

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import spec_rows_ref as S  # noqa: E402
from spec_rows_ref import D, EPS, Case, Row, accept_ref, layout  # noqa: E402
from test_attn_decode_fused_gpu import ULPS, fused_ref, ulp_distance  # noqa: E402
from test_ops_gpu import assert_close_ulps  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = (("aha_hip_debug_attn_decode_rows", 15), ("aha_hip_debug_spec_accept", 8))


def test_entries_in_header_library_and_signatures(hip_lib):
    from aha_amd import _lib, ops
    header = open(os.path.join(ROOT, "include", "aha_hip.h")).read()
    for name, nargs in ENTRIES:
        decl = re.search(r"\bint %s\(([^;]*)\);" % name, header)
        assert decl, name
        assert len(decl.group(1).split(",")) == nargs, name
        assert hasattr(hip_lib, name), name
        assert len(_lib.SIGNATURES[name][1]) == nargs, name
    rust = open(os.path.join(ROOT, "rust", "aha-hip", "src", "lib.rs")).read()
    assert not any(name in rust for name, _ in ENTRIES)   # test entries: no Rust binding
    kernels_h = open(os.path.join(ROOT, "aha_amd", "csrc", "kernels.h")).read()
    assert re.search(r"SPEC_MAX_DRAFT = %d;" % S.SPEC_MAX_DRAFT, kernels_h) and "SPEC_OUT_WORDS = 2 + SPEC_MAX_DRAFT + 1" in kernels_h
    assert (ops.SPEC_MAX_DRAFT, ops.SPEC_OUT_WORDS) == (S.SPEC_MAX_DRAFT, S.SPEC_OUT_WORDS) == (15, 18)


def _rows_args(**kw):
    """A call that would be valid if its pointers were: every device pointer a non-null dummy that a refused call never reads."""
    p = C.c_void_p(64)
    a = dict(qkv=p, q_norm_w=p, k_norm_w=p, rope=p, page_ptrs=p, page0=(C.c_int32 * 3)(0, 0, 2), kv_len=(C.c_int32 * 3)(70, 71, 5), rows=3, nh=4,
             kvh=2, eps=EPS, scale=0.088, o=p, form=1, stream=None)
    a.update(kw)
    return list(a.values())


def _accept_args(**kw):
    p = C.c_void_p(64)
    a = dict(argmax=p, row_tok=(C.c_int32 * 6)(*range(6)), rows=6, seq_tab=(C.c_int32 * 4)(0, 3, 4, 1), n_seqs=2, layout=0, out=p, stream=None)
    a.update(kw)
    return list(a.values())


def test_bad_arguments_are_refused_before_device_work(hip_lib):
    """Every case returns AHA_ERR_INVALID on a machine without a GPU: nothing touched the device (the dummy pointers were never read)."""
    rows, accept = hip_lib.aha_hip_debug_attn_decode_rows, hip_lib.aha_hip_debug_spec_accept
    for ptr in ("qkv", "q_norm_w", "k_norm_w", "rope", "page_ptrs", "page0", "kv_len", "o"):
        assert rows(*_rows_args(**{ptr: None})) == -1, ptr
        assert hip_lib.aha_hip_last_error() == b"debug_attn_decode_rows: null pointer", ptr
    assert rows(*_rows_args(o=None, form=0)) == -1      # only the append alone may leave o out
    bad_rows = [dict(form=-1), dict(form=3), dict(rows=0), dict(rows=-2), dict(nh=5), dict(nh=0), dict(kvh=0), dict(nh=34, kvh=2), dict(nh=65, kvh=65),
                dict(kv_len=(C.c_int32 * 3)(70, 0, 5)), dict(kv_len=(C.c_int32 * 3)(70, 71, -1)), dict(page0=(C.c_int32 * 3)(0, -1, 2))]
    for kw in bad_rows:
        assert rows(*_rows_args(**kw)) == -1, kw
        assert hip_lib.aha_hip_last_error().startswith(b"debug_attn_decode_rows: "), kw
    assert rows(*_rows_args(form=3, o=None)) == -1 and b"form" in hip_lib.aha_hip_last_error()

    for ptr in ("argmax", "row_tok", "seq_tab", "out"):
        assert accept(*_accept_args(**{ptr: None})) == -1, ptr
        assert hip_lib.aha_hip_last_error() == b"debug_spec_accept: null pointer", ptr
    i32 = lambda *v: (C.c_int32 * len(v))(*v)   # noqa: E731
    bad_accept = [dict(layout=-1), dict(layout=2), dict(rows=0), dict(n_seqs=0), dict(n_seqs=-1),
                  dict(seq_tab=i32(0, 3, 4, 2)),              # rows 4 .. 6 of 6
                  dict(seq_tab=i32(0, 3, 6, 0)),              # a first row past the rows, no drafts
                  dict(seq_tab=i32(-1, 3, 4, 1)), dict(seq_tab=i32(0, -1, 4, 1)),
                  dict(seq_tab=i32(0, 6, 4, 1)),              # rows 0 .. 6
                  dict(rows=5, seq_tab=i32(0, 3, 4, 20), row_tok=i32(*range(5))),   # the clamp to 15 drafts still leaves rows 4 .. 19
                  dict(layout=1, n_seqs=1, seq_tab=i32(0, 4, 3)),                   # own 0, drafts 4 .. 6
                  dict(layout=1, n_seqs=1, seq_tab=i32(6, 1, 2)), dict(layout=1, n_seqs=1, seq_tab=i32(0, -1, 2)),
                  dict(layout=1, n_seqs=1, seq_tab=i32(-1, 1, 0)), dict(layout=1, n_seqs=1, seq_tab=i32(0, 1, -1)),
                  dict(layout=1, n_seqs=2, seq_tab=i32(0, 2, 2, 1, 4, 3))]          # the second sequence: drafts 4 .. 6
    for kw in bad_accept:
        assert accept(*_accept_args(**kw)) == -1, kw
        assert hip_lib.aha_hip_last_error().startswith(b"debug_spec_accept: "), kw
    assert b"sequence 1" in hip_lib.aha_hip_last_error()


def test_layout_against_hand_written_tables():
    runs = [(10, 2), (63, 0), (0, 1)]
    assert S.first_ids(runs) == [0, 3, 4]
    rows, seqs = layout(runs, "consecutive")
    assert rows == [Row(0, 0, 0, 11), Row(1, 0, 1, 12), Row(2, 0, 2, 13), Row(3, 1, 0, 64), Row(4, 2, 0, 1), Row(5, 2, 1, 2)]
    assert seqs == [(0, 2), (3, 0), (4, 1)]
    rows, seqs = layout(runs, "engine")
    assert rows == [Row(0, 0, 0, 11), Row(3, 1, 0, 64), Row(4, 2, 0, 1), Row(1, 0, 1, 12), Row(2, 0, 2, 13), Row(5, 2, 1, 2)]
    assert seqs == [(0, 3, 2), (1, 5, 0), (2, 5, 1)]
    for order in S.ORDERS:   # the GPU test's launch: every row once, kv_len ascending by one inside a run
        rows, _ = layout(S.RUNS, order)
        assert sorted(r.id for r in rows) == list(range(95))
        for s, (L0, k) in enumerate(S.RUNS):
            assert [r.kv_len for r in rows if r.seq == s] == list(range(L0 + 1, L0 + k + 2))


def test_run_pool_addresses_every_slot_of_a_sequence():
    runs = [(70, 3), (0, 2)]
    c = Case(2, 2, runs, 50)
    pool = c.pool
    assert pool.npg == [2, 1] and pool.page0 == [0, 2]
    kc, vc = S.rnd((70, 2 * D), 150), S.rnd((70, 2 * D), 250)     # what Case wrote for run 0
    k, v = pool.tokens(0, 70)
    assert torch.equal(k, kc) and torch.equal(v, vc)
    flat = pool.host.flatten()
    for slot in (0, 63, 64, 69, 73, 127):
        e = pool.slot_elems_at(0, slot)
        assert e.shape == (2 * 2 * D,) and int(e.min()) // pool.host.shape[1] == int(e.max()) // pool.host.shape[1] == pool.phys(0, slot // 64)
        k, v = pool.tokens(0, slot + 1)
        assert torch.equal(flat[e], torch.cat([k[slot], v[slot]]))
    assert torch.equal(pool.slot_elems_at(1, 2), pool.phys(1, 0) * pool.host.shape[1] + S.kv_pages.slot_index(2)[2])
    # the slots of a sequence partition its pages
    every = torch.cat([pool.slot_elems_at(0, t) for t in range(128)])
    assert every.unique().numel() == every.numel() == 2 * pool.host.shape[1]


def test_accept_ref_against_hand_written_records():
    #        row:  0   1   2   3   4   5   6
    am = [11, 12, 99, 14, 50, 61, 70]
    tok = [10, 11, 12, 13, 40, 50, 60]
    assert accept_ref(am, tok, (0, 3), 0) == ([11, 12, 99], 3, 2)          # drafts 11 12 13: two confirmed, then 99 != 13
    assert accept_ref(am, tok, (0, 1), 0) == ([11, 12], 2, 1)              # one draft, confirmed: the last row's pick rides along
    assert accept_ref(am, tok, (0, 0), 0) == ([11], 1, 0)
    assert accept_ref(am, tok, (4, 2), 0) == ([50, 61], 2, 5)              # 50 confirmed, 61 != 60
    assert accept_ref(am, tok, (2, 1), 0) == ([99], 1, 2)
    assert accept_ref(am, tok, (4, 5, 2), 1) == ([50, 61], 2, 5)           # the same sequence in the split layout
    assert accept_ref(am, tok, (6, 1, 2), 1) == ([70], 1, 6)               # own row 6 picks 70, draft row 1 holds 11
    assert accept_ref(am, tok, (0, 1, 0), 1) == ([11], 1, 0)
    assert accept_ref([1, 2, 3], [0, 1, 2], (1, 0, 1), 1) == ([2], 1, 1)   # own row behind its draft row: 2 != 0
    assert accept_ref([1, 2, 3], [2, 0, 0], (1, 0, 1), 1) == ([2, 1], 2, 0)
    n = 21                                                                 # 20 drafts, all confirmed: 15 are looked at
    assert accept_ref(list(range(1, n + 1)), list(range(n)), (0, 20), 0) == (list(range(1, 17)), 16, 15)
    assert accept_ref(list(range(1, n + 1)), list(range(n)), (0, 1, 20), 1) == (list(range(1, 17)), 16, 15)


def test_accept_cases_tell_a_rule_that_does_not_stop_at_the_first_mismatch():
    """Sanity of case (e): a rule that counts every confirmed draft instead of the longest prefix gives other records on the cases, and
    the cases hold every (k, a) once per layout."""
    def no_stop(argmax, row_tok, entry, lay):
        pos = (lambda i: entry[0] + i) if lay == 0 else (lambda i: entry[0] if i == 0 else entry[1] + i - 1)
        k = min(entry[-1], S.SPEC_MAX_DRAFT)
        a = sum(argmax[pos(i)] == row_tok[pos(i + 1)] for i in range(k))
        return [argmax[pos(i)] for i in range(a + 1)], a + 1, pos(a)

    cases = S.accept_cases()
    for lay in (0, 1):
        big = [c for c in cases if c["layout"] == lay and len(c["table"]) == 136]
        assert big
        for c in big:
            got = sorted((e[-1], accept_ref(c["argmax"], c["row_tok"], e, lay)[1] - 1) for e in c["table"])
            assert got == [(k, a) for k in range(16) for a in range(k + 1)]
    wrong = {c["name"] for c in cases for e in c["table"] if no_stop(c["argmax"], c["row_tok"], e, c["layout"]) != accept_ref(c["argmax"], c["row_tok"], e, c["layout"])}
    assert any("every (k, a)" in n and "layout 0" in n for n in wrong) and any("every (k, a)" in n and "layout 1" in n for n in wrong)
    assert any("match after the first mismatch" in n for n in wrong)
    for c in cases:   # every table stays inside its rows (the entry refuses others)
        for e in c["table"]:
            k = min(e[-1], S.SPEC_MAX_DRAFT)
            reach = [e[0]] + ([e[0] + k] if c["layout"] == 0 else [e[1], e[1] + k - 1] if k else [])
            assert 0 <= min(reach) and max(reach) < len(c["argmax"]) == len(c["row_tok"]), c["name"]


def test_run_reference_agrees_with_the_oracle():
    """A run's rows through fused_ref one after the other, every row appending its own token, against oracle.qwen3's causal attention over
    the same tokens (rms_norm, apply_rotary_pos_emb, eager_attention_forward on the f32 score chain).  q and k have the same rounding
    points in both; k differs from the oracle's by an f32-against-f64 rounding flip in a few elements, which moves a score by less than
    2^-8 of one product -- far below an output ulp -- so what separates the outputs is the rounding of the output itself: 1 bf16 ulp at
    row scale, the bound of tests/test_kv_pages_cpu.py."""
    nh, kvh, L0, k = 4, 2, 60, 7
    c = Case(nh, kvh, [(L0, k)], 21)
    n = k + 1
    kc, vc = c.pool.tokens(0, L0)
    k_all, v_all = torch.cat([kc, c.ref_k.reshape(n, kvh * D)]), torch.cat([vc, c.ref_v.reshape(n, kvh * D)])
    ref = S.run_ref(c, 0, k_all, v_all)

    nm = Numerics("bf16", matmul_f64=True, attn_scores_rounded=False)
    q = oq.rms_norm(nm, c.qkv[:, : nh * D].float().reshape(1, n, nh, D), c.qn.float(), EPS).transpose(1, 2)
    kk = oq.rms_norm(nm, c.qkv[:, nh * D: (nh + kvh) * D].float().reshape(1, n, kvh, D), c.kn.float(), EPS).transpose(1, 2)
    cos, sin = c.rope[:, :64].repeat(1, 2), c.rope[:, 64:].repeat(1, 2)
    q, kk = oq.apply_rotary_pos_emb(nm, q, kk, cos[None], sin[None])
    assert_close_ulps(c.ref_k.reshape(n, kvh * D), kk.transpose(1, 2).reshape(n, kvh * D), 2, 0.97, "the run's k against the oracle")
    K = torch.cat([kc.float().reshape(1, L0, kvh, D).transpose(1, 2), kk], 2)
    V = torch.cat([vc, c.ref_v.reshape(n, kvh * D)]).float().reshape(1, L0 + n, kvh, D).transpose(1, 2)
    col, row = torch.arange(L0 + n)[None, :], torch.arange(n)[:, None]
    mask = torch.zeros(n, L0 + n).masked_fill(col > L0 + row, float("-inf"))[None, None]
    want = oq.eager_attention_forward(nm, q, K, V, nh // kvh, mask, c.scale).reshape(n, nh, D)
    assert c.scale == oq.attn_scale(nm, D)
    for i in range(n):
        assert_close_ulps(ref[i].to(torch.bfloat16).reshape(nh, D), want[i], 1, None, f"row {i} against the oracle", row_scale=True)


def test_the_reference_sees_a_leaked_successor_only_while_the_cache_is_short():
    """Sanity of (c): the f64 reference of the run (0, 15) with ONE successor token visible to a row differs from the true one by more than
    the 3-ulp bound on every row that has a successor (measured: 45 .. 378 ulps for this shape, never below 11 for the others), so (c)
    sees such a leak there.  At a cache of 4090 tokens the same leak can hide inside the bound -- it does for the run's first row here;
    over the rows of that run it moves the output by 0.5 .. 31 ulps depending on the leaked token's score -- so there (c) cannot be
    relied on and only the bit comparison (b) of the GPU test is sure to see it."""
    nh, kvh = 8, 2

    def worst(c, L0, i, k_all, v_all):
        true = fused_ref(c.qkv[i], c.qn, c.kn, c.rope[i], k_all[: L0 + i], v_all[: L0 + i], nh, kvh, EPS, c.scale)[0]
        leak_k, leak_v = torch.cat([k_all[: L0 + i], k_all[L0 + i + 1: L0 + i + 2]]), torch.cat([v_all[: L0 + i], v_all[L0 + i + 1: L0 + i + 2]])
        leaked = fused_ref(c.qkv[i], c.qn, c.kn, c.rope[i], leak_k, leak_v, nh, kvh, EPS, c.scale)[0]
        a, b = leaked.to(torch.bfloat16).view(nh, D), true.to(torch.bfloat16).view(nh, D)
        return ulp_distance(a, b, b.float().abs().amax(-1, keepdim=True))

    c = Case(nh, kvh, [(0, 15)], 300)
    k_all, v_all = c.ref_k.reshape(16, kvh * D), c.ref_v.reshape(16, kvh * D)
    for i in range(15):
        assert worst(c, 0, i, k_all, v_all) > ULPS, i
    c = Case(nh, kvh, [(4090, 15)], 300)
    kc, vc = c.pool.tokens(0, 4090)
    k_all, v_all = torch.cat([kc, c.ref_k.reshape(16, kvh * D)]), torch.cat([vc, c.ref_v.reshape(16, kvh * D)])
    assert worst(c, 4090, 0, k_all, v_all) <= ULPS
