"""Helpers of tests/test_spec_rows_gpu.py and its CPU tier: the rows of a draft-and-verify decode step ("runs"), their two launch orders, a
page pool whose every slot can be addressed, the accept rule restated, and the inputs of the accept cases.  Plain helpers: no test, no GPU
needed to import.

A run (L0, k) is one sequence with L0 cached tokens and k drafts: k + 1 rows with kv_len = L0 + 1 .. L0 + k + 1 on the same page0 (row i's
input is the sequence's last token for i = 0 and draft i behind it).  Rows have a canonical id -- run by run, i ascending -- in which the
inputs (qkv, rope) and the references are kept; a launch order is a list of Row records that name them.
"""
import os
import sys
from collections import namedtuple

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kv_pages  # noqa: E402
from rope_ref import D, Pool, norm_weights, prologue_rows_ref, rnd  # noqa: E402
from test_attn_decode_fused_gpu import EPS, bf16_scale, fused_ref, rope_rows  # noqa: E402,F401

SPEC_MAX_DRAFT = 15                 # kernels.h
SPEC_OUT_WORDS = 2 + SPEC_MAX_DRAFT + 1
OUT_COUNT, OUT_LAST_ROW, OUT_TOKENS = 0, 1, 2
ORDERS = ("consecutive", "engine")
SHAPES = [(2, 2), (6, 2), (8, 2), (16, 1), (32, 8)]
RUNS = [(0, 15), (56, 15), (63, 1), (64, 3), (250, 15), (505, 15), (1020, 7), (4090, 15), (300, 0)]

Row = namedtuple("Row", "id seq i kv_len")   # canonical id, the run, the position inside it (0: the sequence's own row), cache length after it


# ---- runs and their launch orders --------------------------------------------------------------------------------------------------
def first_ids(runs):
    """Canonical id of every run's first row."""
    out, n = [], 0
    for _, k in runs:
        out.append(n)
        n += k + 1
    return out


def layout(runs, order):
    """The rows of `runs` in launch order: "consecutive" -- run by run, a run's rows back to back (spec_decode_loop's step) -- or "engine"
    -- every run's first row first, then the draft rows, run by run (engine_step's).
    -> (rows [Row], seqs): seqs[s] = (row0, k) for the consecutive order, the entry of spec_accept_rows_kernel, and (own row, first draft
    row, k) for the engine's, the entry of spec_accept_split_kernel (first draft row: where the run's drafts would start, also for k = 0)."""
    assert order in ORDERS
    ids = first_ids(runs)
    rows, seqs = [], []
    if order == "consecutive":
        for s, (L0, k) in enumerate(runs):
            seqs.append((len(rows), k))
            rows += [Row(ids[s] + i, s, i, L0 + i + 1) for i in range(k + 1)]
        return rows, seqs
    rows = [Row(ids[s], s, 0, L0 + 1) for s, (L0, _) in enumerate(runs)]
    for s, (L0, k) in enumerate(runs):
        seqs.append((s, len(rows), k))
        rows += [Row(ids[s] + i, s, i, L0 + i + 1) for i in range(1, k + 1)]
    return rows, seqs


# ---- the pool ------------------------------------------------------------------------------------------------------------------------
class RunPool(Pool):
    """rope_ref.Pool with one sequence per run, sized for the run's last row; any slot of a sequence can be addressed."""

    def __init__(self, kvh, runs, seed):
        super().__init__(kvh, [L0 + k + 1 for L0, k in runs], seed)

    def slot_elems_at(self, s, slot):
        """Flat pool indices (page * page_elems + element) of the 2 * kvh * 128 elements of token slot `slot` of sequence s: k, then v."""
        assert 0 <= slot < self.npg[s] * 64
        return self.phys(s, slot // 64) * self.host.shape[1] + kv_pages.slot_index(self.kvh)[slot % 64]

    def tokens(self, s, n, image=None):
        """(k, v), each (n, kvh * 128): the first n token slots of sequence s as a pool image on the CPU holds them (default: the host
        image the pool was built with)."""
        image = self.host if image is None else image
        assert image.shape == self.host.shape and n <= self.npg[s] * 64
        t = torch.arange(n)
        pg = self.perm[self.page0[s] + t // 64]
        kv = image[pg[:, None], kv_pages.slot_index(self.kvh)[t % 64]]
        return kv[:, : self.kvh * D], kv[:, self.kvh * D:]


class Case:
    """Inputs of one head shape and one list of runs, all on the CPU: the pool with every run's L0 cached tokens written, and per canonical
    row its qkv and rope rows and the reference prologue (q, k, v) -- k is what the append must write.  A later step of some of the
    sequences of another Case passes that Case's pool and, per run, the pool sequence it continues (pool_seq)."""

    def __init__(self, nh, kvh, runs, seed, pool=None, pool_seq=None):
        self.nh, self.kvh, self.runs = nh, kvh, list(runs)
        self.pool_seq = list(range(len(runs))) if pool_seq is None else list(pool_seq)
        self.R = sum(k + 1 for _, k in runs)
        self.qn, self.kn = norm_weights()
        self.scale = bf16_scale()
        self.qkv = rnd((self.R, (nh + 2 * kvh) * D), seed)
        self.rope = rope_rows(self.R, seed + 1)
        self.ref_q, self.ref_k, self.ref_v = prologue_rows_ref(self.qkv, self.qn, self.kn, self.rope, nh, kvh, EPS)
        self.pool = pool
        if pool is None:
            self.pool = RunPool(kvh, runs, seed + 2)
            for s, (L0, _) in enumerate(runs):
                self.pool.write(s, rnd((L0, kvh * D), seed + 100 + s), rnd((L0, kvh * D), seed + 200 + s))


def run_ref(c, s, k_all, v_all, rows=None):
    """The f64 reference outputs of run s of Case c: k_all, v_all (>= kv_len - 1 of the last row, kvh * 128) bf16 are the sequence's cache
    tokens -- row i sees the first L0 + i of them and its own token from the reference prologue.  -> {canonical id: o (nh * 128) f64}."""
    L0, k = c.runs[s]
    r0 = first_ids(c.runs)[s]
    out = {}
    for i in (range(k + 1) if rows is None else rows):
        r = r0 + i
        out[r] = fused_ref(c.qkv[r], c.qn, c.kn, c.rope[r], k_all[: L0 + i], v_all[: L0 + i], c.nh, c.kvh, EPS, c.scale)[0]
    return out


# ---- the accept rule -------------------------------------------------------------------------------------------------------------
def accept_ref(argmax, row_tok, entry, layout):
    """The rule of spec_accept_rows_kernel (layout 0, entry = (row0, n_draft): position i of the sequence is row row0 + i) and
    spec_accept_split_kernel (layout 1, entry = (own, d0, n_draft): position 0 is row own, position i >= 1 row d0 + i - 1).  Draft i is the
    input token of position i; at most SPEC_MAX_DRAFT drafts are looked at.  a = the longest prefix with argmax(position i) == draft
    i + 1.  -> (tokens = argmax(position 0 .. a), count = a + 1, the row of position a)."""
    if layout == 0:
        row0, nd = entry
        pos = lambda i: row0 + i   # noqa: E731
    else:
        own, d0, nd = entry
        pos = lambda i: own if i == 0 else d0 + i - 1   # noqa: E731
    k = min(int(nd), SPEC_MAX_DRAFT)
    a = 0
    while a < k and int(argmax[pos(a)]) == int(row_tok[pos(a + 1)]):
        a += 1
    return [int(argmax[pos(i)]) for i in range(a + 1)], a + 1, pos(a)


def _scatter(rows, per_seq):
    return [per_seq[r.seq][r.i] for r in rows]


def accept_sequence(k, a, seed, rematch=True):
    """Input tokens and picks of one sequence's k + 1 positions with exactly `a` confirmed drafts: (tok[k + 1], am[k + 1]).  Position i < a
    picks draft i + 1, position a (if a < k) something else, and with `rematch` every position behind it picks its next draft again -- the
    rule must stop at the first mismatch."""
    g = torch.Generator().manual_seed(seed)
    tok = [int(x) for x in torch.randperm(100000, generator=g)[: k + 2] + 1]   # distinct: the last one is no draft of the sequence
    am = [tok[i + 1] for i in range(k + 1)]
    if a < k:
        am[a] = tok[a + 1] + 100000
        if not rematch:
            am[a + 1:] = [t + 200000 for t in am[a + 1:]]
    return tok[: k + 1], am


def accept_case(name, seqs, order, layout_id):
    """One launch of the accept kernel: seqs = [(tok, am)] per sequence -> dict(name, argmax, row_tok, table, layout)."""
    runs = [(0, len(t) - 1) for t, _ in seqs]
    rows, tab = layout(runs, order)
    if order == "consecutive" and layout_id == 1:   # the split kernel on consecutive rows: the drafts start right behind the own row
        tab = [(r0, r0 + 1, k) for r0, k in tab]
    assert len(tab[0]) == (3 if layout_id else 2)
    return dict(name=name, argmax=_scatter(rows, [s[1] for s in seqs]), row_tok=_scatter(rows, [s[0] for s in seqs]), table=tab, layout=layout_id)


def accept_cases():
    """The launches of the accept test, both layouts."""
    pairs = [(k, a) for k in range(SPEC_MAX_DRAFT + 1) for a in range(k + 1)]
    assert len(pairs) == 136
    every = [accept_sequence(k, a, 1000 + 16 * k + a) for k, a in pairs]
    cases = []
    for lay, order in ((0, "consecutive"), (1, "consecutive"), (1, "engine")):
        tag = f"layout {lay} {order}"
        cases.append(accept_case(f"every (k, a), 136 sequences, {tag}", every, order, lay))
        for n, first in ((1, 100), (64, 30), (65, 60)):
            cases.append(accept_case(f"{n} sequences, {tag}", every[first: first + n], order, lay))
        # picks 1 and 2 confirmed, 3 refused, 4 and 5 would match again
        cases.append(accept_case(f"match after the first mismatch, {tag}", [([5, 6, 7, 8, 9, 10], [6, 7, 99, 9, 10, 11])], order, lay))
        # every draft repeats the token before it; position 2 picks something else
        cases.append(accept_case(f"a draft equal to the token before it, {tag}", [([7, 7, 7, 7], [7, 7, 9, 7]), ([3, 3], [3, 3])], order, lay))
        # NDRAFT = 20 on 21 rows, every pick confirmed: the rule stops at SPEC_MAX_DRAFT
        c = accept_case(f"NDRAFT 20, all confirmed, {tag}", [accept_sequence(20, 20, 77)], order, lay)
        assert c["table"][0][-1] == 20
        cases.append(c)
    # the split layout alone: a sequence without drafts between two that draft, and draft blocks in another order than the own rows
    three = [accept_sequence(3, 3, 31), accept_sequence(0, 0, 32), accept_sequence(2, 1, 33)]
    cases.append(accept_case("NDRAFT 0 between two that draft, layout 1 engine", three, "engine", 1))
    c = accept_case("draft blocks in reverse order, layout 1 engine", three, "engine", 1)
    # rows: own 0 1 2 | drafts of 0 (3 4 5) | drafts of 2 (6 7)  ->  own 0 1 2 | drafts of 2 (3 4) | a row of no sequence (5) | drafts of 0 (6 7 8)
    am, tk = c["argmax"], c["row_tok"]
    c["argmax"] = am[:3] + am[6:8] + [424242] + am[3:6]
    c["row_tok"] = tk[:3] + tk[6:8] + [am[2]] + tk[3:6]   # the stray row holds what sequence 2's own row picked: it must not be read as a draft
    c["table"] = [(0, 6, 3), (1, 6, 0), (2, 3, 2)]
    cases.append(c)
    return cases
