"""-m gpu: the kernels of a draft-and-verify decode step (kernels_batch.hip: kv_append_rows_kernel, attn_decode_rows_kernel = the fused
decode attention body with APPEND = false, spec_accept_rows_kernel, spec_accept_split_kernel) at op level, through the test entries
ops.debug_attn_decode_rows and ops.debug_spec_accept.

A step with drafts holds several rows of ONE sequence (tests/spec_rows_ref.py "run": kv_len = L0 + 1 .. L0 + k + 1 on the same page0).  It
appends the K/V of all rows first (form 2) and then attends without the body's own append (form 1 = both launches); a plain step does both
in one kernel (form 0), one row per sequence.  Speculation changes no output by contract, so:

  a. the pool after form 2 on the whole launch == the pool after form 0 on the same rows one at a time, over every element; the appended
     K against the f64 prologue at the fused test's bound, the appended V bit for bit.
  b. the outputs of form 1 on the whole launch == those of the one-row form 0 launches, bit for bit, in both launch orders and twice.
     THIS is the check that sees a row reading past its kv_len: in the one-row launches the slots behind a row hold the pool's 100x
     garbage, in the joint launch they hold its successors' K/V, finite and of normal size.  Any dependence on them gives other bits.
     Against a reference such a leak is sure to show only while the cache is short (tests/test_spec_rows_cpu.py: one leaked token at
     kv_len <= 16 moves every row by 11 .. 378 ulps); at kv_len in the thousands one more token of normal size weighs about 1 / kv_len
     and moves a row by 0.5 .. 31 ulps depending on its score, so it can stay inside the 3-ulp bound -- there only (b) is sure to see it.
     (Tried: the page loop's mask `t0 + t < L_old` widened by `|| t0 + t == L_old + 1`, the slot behind the row's own.  (b) and (d) then
     name every row whose successor's slot lies on a page the row loads, those of (505, 15), (1020, 7) and (4090, 15) included; (a) and
     (e) still pass.)
  c. every row of form 1 against fused_ref (tests/test_attn_decode_fused_gpu.py) at the project's decode-attention bound, 3 bf16 ulps
     per head at the head's largest |output| and for the row at its rms.  The cached tokens of a row are its inputs: they are read back
     from the pool as the append left them ((a) holds them to their own reference), the row's own token comes from the reference prologue.
  d. a second step over a rejected run: from L0 + 3 with other rows and k = 7, over the first step's stale slots; (a) and (b) again.
  e. the accept kernels, both layouts, against the rule restated in Python (spec_rows_ref.accept_ref).

Head shapes (2, 2), (6, 2), (8, 2), (16, 1), (32, 8): g = 1, 3, 4, 16 and the 8-kv-head shape of the real models.  Runs (L0, k), all in one
launch per head shape: (0, 15) an empty cache, the first row has kv_len 1; (56, 15) crosses the page inside the run; (63, 1), (64, 3) the
page edge; (250, 15) 1 -> 2 splits between rows of one sequence; (505, 15) crosses 512; (1020, 7) 4 -> 5 splits; (4090, 15) 16 -> 17
splits, the second merge batch; (300, 0) a plain row among them.  The smallest shapes that reach each path, none is a workload shape.

Measured on an MI355X: worst distance of form 1 from the bf16-rounded f64 reference in bf16 ulps, "per-head scale / row-rms scale", per
(g, run); g = 4 is the larger of (8, 2) and (32, 8):

  run (L0, k)        g = 1       g = 3       g = 4      g = 16
     (0, 15)   1.00 / 3.00 1.00 / 3.00 1.00 / 3.00 1.00 / 2.50
    (56, 15)   1.00 / 1.50 1.00 / 2.00 1.00 / 2.06 1.00 / 2.00
     (63, 1)   1.00 / 1.00 1.00 / 1.00 1.00 / 1.50 1.00 / 1.50
     (64, 3)   1.00 / 1.00 1.00 / 2.00 1.00 / 2.00 1.00 / 2.00
   (250, 15)   1.00 / 2.00 1.00 / 1.00 1.00 / 1.50 1.00 / 1.50
   (505, 15)   1.00 / 1.00 1.00 / 1.00 1.00 / 1.00 1.00 / 1.00
   (1020, 7)   1.00 / 1.00 1.00 / 1.00 1.00 / 1.13 1.00 / 1.00
  (4090, 15)   1.00 / 1.06 1.00 / 1.00 1.00 / 1.50 1.00 / 1.13
    (300, 0)   1.00 / 1.00 1.00 / 1.00 1.00 / 1.00 1.00 / 1.00

A figure is the worst over the k + 1 rows of the run.  The 3.00 of (0, 15) is the rms scale of rows with 2 .. 16 tokens (a single element
of a row that mixes few tokens); by (b) these are the bits of the default fused kernel on the same rows, not of the draft path.  (a), (b),
(d) and (e) held bit for bit on that run: no pool element and no output element differed.
"""
import functools
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import spec_rows_ref as S  # noqa: E402
from spec_rows_ref import D, EPS, ORDERS, RUNS, SHAPES, Case, layout  # noqa: E402
from test_attn_decode_fused_gpu import K_EXACT, K_ULPS, ULPS, ulp_distance  # noqa: E402
from test_ops_gpu import assert_close_ulps  # noqa: E402

pytestmark = pytest.mark.gpu

STEP2_OF = [1, 4]            # the runs (56, 15) and (250, 15) of RUNS ...
STEP2_KEEP, STEP2_K = 3, 7   # ... continue from L0 + 3 (two drafts confirmed) with 7 new drafts


@functools.lru_cache(maxsize=None)
def case(nh, kvh):
    return Case(nh, kvh, RUNS, 300)


@functools.lru_cache(maxsize=None)
def case2(nh, kvh):
    assert [RUNS[s] for s in STEP2_OF] == [(56, 15), (250, 15)]
    return Case(nh, kvh, [(RUNS[s][0] + STEP2_KEEP, STEP2_K) for s in STEP2_OF], 700, pool=case(nh, kvh).pool, pool_seq=STEP2_OF)


class Launcher:
    """A Case's inputs on the device and its launches; outputs come back in canonical row order on the CPU."""

    def __init__(self, c):
        self.c, self.pool = c, c.pool
        self.qkv, self.rope, self.qn, self.kn = (t.to("cuda") for t in (c.qkv, c.rope, c.qn, c.kn))

    def run(self, rows, form):
        from aha_amd import ops
        c = self.c
        idx = torch.tensor([r.id for r in rows], device="cuda")
        o = ops.debug_attn_decode_rows(self.qkv[idx].contiguous(), self.qn, self.kn, self.rope[idx].contiguous(), self.pool.ptrs,
                                       [self.pool.page0[c.pool_seq[r.seq]] for r in rows], [r.kv_len for r in rows], c.nh, c.kvh, EPS, c.scale, form)
        torch.cuda.synchronize()
        if o is None:
            return None
        out = torch.zeros(c.R, c.nh * D, dtype=torch.bfloat16)
        out[idx.cpu()] = o.cpu()
        return out

    def one_by_one(self):
        """Form 0, one launch per row, kv_len ascending within every run: the plain decode of the same tokens."""
        out = torch.zeros(self.c.R, self.c.nh * D, dtype=torch.bfloat16)
        for r in layout(self.c.runs, "consecutive")[0]:
            out[r.id] = self.run([r], 0)[r.id]
        return out


def bits(t):
    return t.view(torch.int16)


def differing_rows(c, a, b):
    rows = layout(c.runs, "consecutive")[0]
    return [(c.runs[r.seq], r.i) for r in rows if not torch.equal(bits(a[r.id]), bits(b[r.id]))]


def check_append(c, start, joint, single):
    """(a) for Case c: start / joint / single are pool images on the device -- before the step, after form 2 on all rows, after the
    one-row form 0 launches."""
    pool, kvh = c.pool, c.kvh
    n_diff = int((bits(joint) != bits(single)).sum())
    assert n_diff == 0, f"{n_diff} pool elements differ between the joint append and the one-row fused launches"
    rows = layout(c.runs, "consecutive")[0]
    changed = torch.nonzero((bits(joint) != bits(start)).flatten()).flatten().cpu()
    allowed = torch.cat([pool.slot_elems_at(c.pool_seq[r.seq], r.kv_len - 1) for r in rows])
    assert torch.isin(changed, allowed).all(), f"{int((~torch.isin(changed, allowed)).sum())} pool elements outside the appended slots changed"
    image = joint.cpu()
    first = S.first_ids(c.runs)
    k_got = torch.zeros(c.R, kvh * D, dtype=torch.bfloat16)
    for s, (L0, k) in enumerate(c.runs):
        kk, vv = pool.tokens(c.pool_seq[s], L0 + k + 1, image)
        ids = slice(first[s], first[s] + k + 1)
        k_got[ids] = kk[L0:]
        assert torch.equal(bits(vv[L0:]), bits(c.ref_v[ids].reshape(k + 1, kvh * D))), f"run {(L0, k)}: appended v differs from the qkv rows'"
    k_ref = c.ref_k.reshape(c.R, kvh * D)
    for r in rows:
        assert_close_ulps(k_got[r.id], k_ref[r.id], K_ULPS, None, f"run {c.runs[r.seq]} row {r.i}: appended k")
    exact = float((k_got.float() == k_ref.float()).float().mean())
    assert exact >= K_EXACT, f"only {exact:.4f} of the appended k bit-identical to the reference"


def check_outputs(c, ln, start, o_single):
    """(b) for Case c from the pool image `start`: form 1 on the whole launch, both orders, twice each, against the one-row launches."""
    for order in ORDERS:
        rows = layout(c.runs, order)[0]
        got = []
        for _ in range(2):
            c.pool.dev.copy_(start)
            got.append(ln.run(rows, 1))
        assert torch.equal(bits(got[0]), bits(got[1])), f"{order} order: the same launch twice gave different output bits: {differing_rows(c, got[0], got[1])}"
        bad = differing_rows(c, got[0], o_single)
        assert not bad, f"{order} order: (run, row) whose joint output differs from its one-row launch: {bad}"


@pytest.fixture
def on_device(request):
    """The pool of the head shape on the device for the test, dropped after it."""
    def up(nh, kvh):
        pool = case(nh, kvh).pool
        pool.upload()
        request.addfinalizer(lambda: [delattr(pool, a) for a in ("dev", "before", "ptrs") if hasattr(pool, a)])
        return pool
    return up


@pytest.mark.parametrize("nh,kvh", SHAPES)
def test_append_bits_equal_the_fused_kernels(gpu, on_device, nh, kvh):
    """(a): kv_append_rows_kernel on all rows writes the page bits the fused kernel's own append writes row after row, and nothing else."""
    c, pool = case(nh, kvh), on_device(nh, kvh)
    ln = Launcher(c)
    assert ln.run(layout(c.runs, "consecutive")[0], 2) is None
    joint = pool.dev.clone()
    pool.restore()
    ln.one_by_one()
    check_append(c, pool.before, joint, pool.dev)
    pool.restore()
    ln.run(layout(c.runs, "engine")[0], 2)
    assert torch.equal(bits(joint), bits(pool.dev)), "the append in the engine's row order left other pool bits"


@pytest.mark.parametrize("nh,kvh", SHAPES)
def test_output_bits_equal_the_one_row_launches(gpu, on_device, nh, kvh):
    """(b): append-then-attend over rows of one sequence gives every row the bits of its own plain decode step.  In the one-row launches
    the slots behind a row hold 100x garbage, in the joint launch its successors' K/V: a row that read a slot past its kv_len would get
    other bits here, whatever a reference at long cache lengths can resolve."""
    c, pool = case(nh, kvh), on_device(nh, kvh)
    ln = Launcher(c)
    o_single = ln.one_by_one()
    check_outputs(c, ln, pool.before, o_single)


@pytest.mark.parametrize("nh,kvh", SHAPES)
def test_rows_against_the_f64_reference(gpu, on_device, nh, kvh):
    """(c): every row of the append-then-attend launch against fused_ref over the tokens the append left in the pool."""
    c, pool = case(nh, kvh), on_device(nh, kvh)
    g = nh // kvh
    o = Launcher(c).run(layout(c.runs, "consecutive")[0], 1)
    image = pool.dev.cpu()
    first = S.first_ids(c.runs)
    for s, (L0, k) in enumerate(c.runs):
        k_all, v_all = pool.tokens(s, L0 + k, image)
        ref = S.run_ref(c, s, k_all, v_all)
        worst_head = worst_rms = 0.0
        for i in range(k + 1):
            r = first[s] + i
            got, want = o[r], ref[r].to(torch.bfloat16)
            worst_head = max(worst_head, ulp_distance(got.view(nh, D), want.view(nh, D), want.float().view(nh, D).abs().amax(-1, keepdim=True)))
            worst_rms = max(worst_rms, ulp_distance(got, want, want.float().pow(2).mean().sqrt()))
        print(f"ULP nh={nh} kvh={kvh} g={g} run=({L0}, {k}) head={worst_head:.3f} rms={worst_rms:.3f}")
        for i in range(k + 1):
            r = first[s] + i
            got, want = o[r], ref[r].to(torch.bfloat16)
            assert_close_ulps(got.view(nh, D), want.view(nh, D), ULPS, None, f"run {(L0, k)} row {i}, per head", row_scale=True)
            assert_close_ulps(got, want, ULPS, None, f"run {(L0, k)} row {i}, row rms")
            if L0 + i == 0:   # kv_len 1: p = 1 and sum = 1, the output IS the new v
                v_new = c.ref_v[r].view(kvh, 1, D).expand(kvh, g, D).contiguous()
                assert torch.equal(bits(got.view(kvh, g, D)), bits(v_new)), "kv_len 1 must return the new v bit for bit"


@pytest.mark.parametrize("nh,kvh", SHAPES)
def test_second_step_over_a_rejected_run(gpu, on_device, nh, kvh):
    """(d): step 1 leaves 16 appended tokens behind (56, 15) and (250, 15); two drafts are confirmed and step 2 starts at L0 + 3 with other
    rows and 7 drafts: its slots hold step 1's rejected tokens, the slots behind its last row still do.  (a) and (b) from that state."""
    c1, pool = case(nh, kvh), on_device(nh, kvh)
    Launcher(c1).run(layout(c1.runs, "consecutive")[0], 1)
    start = pool.dev.clone()
    c2 = case2(nh, kvh)
    ln = Launcher(c2)
    ln.run(layout(c2.runs, "consecutive")[0], 2)
    joint = pool.dev.clone()
    pool.dev.copy_(start)
    o_single = ln.one_by_one()
    check_append(c2, start, joint, pool.dev)
    check_outputs(c2, ln, start, o_single)


def test_accept_kernels_against_the_rule(gpu):
    """(e): COUNT, LAST_ROW and TOKENS[0 .. count) of every sequence of every case, both kernels; words behind the count are not compared."""
    from aha_amd import ops
    cases = S.accept_cases()
    assert {(c["layout"], len(c["table"])) for c in cases} >= {(lay, n) for lay in (0, 1) for n in (1, 64, 65, 136)}
    for c in cases:
        am = torch.tensor(c["argmax"], dtype=torch.int32, device="cuda")
        out = ops.debug_spec_accept(am, c["row_tok"], c["table"], c["layout"]).cpu().tolist()
        assert len(out) == len(c["table"])
        for s, entry in enumerate(c["table"]):
            toks, count, last = S.accept_ref(c["argmax"], c["row_tok"], entry, c["layout"])
            rec = out[s]
            assert rec[S.OUT_COUNT] == count and rec[S.OUT_LAST_ROW] == last, f"{c['name']}: sequence {s} {entry}: got {rec[:2]}, want {[count, last]}"
            assert rec[S.OUT_TOKENS: S.OUT_TOKENS + count] == toks, f"{c['name']}: sequence {s} {entry}: tokens"
