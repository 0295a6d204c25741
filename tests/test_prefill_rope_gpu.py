"""-m gpu: the prefill's rope table, q/k-norm + RoPE + paged KV write and the Q load fused into the prefill attention, as the model's
prefill launches them, against an f64 reference of the operation (tests/prefill_rope_ref.py).

The kernels under test (aha_amd/csrc/kernels_elem.hip, kernels_attn.hip) are reached through ops.debug_prefill_rope and
ops.debug_prefill_attn_qfuse: rope_table_kernel; qknorm_rope_rows_kernel<8> and <2> (skip_q) with their V block role, from a cache offset
the host names, with and without the table, and in the packed form (row_slot / page_rows); qknorm_rope_kernel writing pages (below 16 rows,
and with the cache offset read from the device); the Q load of attn_prefill_kernel with q_norm_w / q_rope_tab, single sequence, two segments
in one launch, and packed with and without seg_kv0.  (ops.qknorm_rope, which tests/test_ops_gpu.py covers, only reaches the per-element kernel
with a contiguous destination.)

Inputs: every element of the page pool starts as finite garbage and the pages of a sequence are a seeded permutation of the pool with
spare pages (rope_ref.Pool); the tokens in front of a call's cache offset are written with kv_pages.pack_pages.  After
every call the whole pool is read back: K of every written slot within 2 bf16 ulps of the reference with >= 0.97 bit-identical
(test_ops_gpu.py::test_qknorm_rope's bound), V bit-identical, q as K, EVERY other element of the pool bit-unchanged.  Every call's
positions run through 0.., 4000.., 39900.. and 130000.. on three different position rows with an interleaved M-RoPE axis map, so the table
and the in-place cosf path both see angles up to 1.3e5 rad.

Measured on an MI355X (the tests print these as "MEASURED ..." lines with -s).  The table: all 124416 entries of either position set
bit-identical to the reference (distance 0, share 1.00000; the cap is 0.999).  K and q: worst distance from the reference in bf16 ulps at
max(|ref|, rms) / smallest bit-identical share over the form's calls (the cap is 2 ulps / 0.97); "-" = the form writes no q (skip_q) or
does not run for the shape; a share of 0.9999 is one to three elements of one call:

  (nh, kvh) skip_q   table k      table q      no_table k   no_table q   device_start k  device_start q  packed k     packed + kv0 k
  (4, 2)    0        0 / 1.0000   0.25/0.9999  0 / 1.0000   0 / 1.0000   0 / 1.0000      0 / 1.0000      0 / 1.0000   0 / 1.0000
  (6, 2)    0        0 / 1.0000   0.25/1.0000  0 / 1.0000   0 / 1.0000   0 / 1.0000      0 / 1.0000      0 / 1.0000   0 / 1.0000
  (8, 2)    0        1 / 0.9999   0.25/1.0000  0 / 1.0000   0.25/1.0000  0 / 1.0000      0 / 1.0000      0 / 1.0000   0 / 1.0000
  (8, 1)    1        0 / 1.0000   -            0 / 1.0000   -            0 / 1.0000      0 / 1.0000      0 / 1.0000   0 / 1.0000
  (6, 3)    1        1 / 0.9999   -            0 / 1.0000   -            0 / 1.0000      0 / 1.0000      0 / 1.0000   0 / 1.0000
  (32, 8)   0        0 / 1.0000   1 / 1.0000   0 / 1.0000   0.25/1.0000  0 / 1.0000      0.5 / 1.0000    -            -
  (32, 8)   1        0 / 1.0000   -            0 / 1.0000   -            -               -               1 / 0.9999   1 / 0.9999

(the calls below 16 rows of the skip_q shapes run with skip_q 0: k 0 / 1.0000, q 0 / 1.0000.)  Far from both caps: the device's cosf / sinf
round to the same bf16 as f64 cos / sin on every table entry here, and the rare differing element is one rounding of a product or sum.

Mutations of the kernels, one at a time on a scratch copy, each wrong in values only, and what caught them on the device:
  - rotate-half sign flipped for the high half: test_pages_after_the_write (all 7; first at offset 0, S 16: ~40 % of K more than 2 ulps off)
    and test_the_forms_leave_the_same_bits (all 6: the per-element kernel's pages differ);
  - first = a.nh - 1 under skip_q: test_pages_after_the_write ((8,1) and (6,3) at S 16: "skip_q, yet q was written"; (32,8) skip_q at S 16
    and the packed calls of (4,2), (6,2), (8,2): K rows never written) and test_the_forms_leave_the_same_bits (4 of 6: the packed pages);
  - kpage_elem with fragment stride 2: test_pages_after_the_write (all 7; first at S 17 -- at 16 rows only fragment row 0 is written and
    the stride does not show) and test_the_forms_leave_the_same_bits (all 6);
  - ok[e] ignored in the partial V piece: test_pages_after_the_write (all 7: "12288 pool elements outside the written slots changed" at
    offset 0, S 16) and test_the_forms_leave_the_same_bits (all 6);
  - q_rope_tab not advanced for the second segment: test_q_fused_two_segments_in_one_call[8-2] (the split launch; (32, 8) is one launch and
    rightly passes);
  - rbf dropped from one RoPE product: test_pages_after_the_write (all 7: K only 0.79 - 0.82 bit-identical) and
    test_the_forms_leave_the_same_bits (all 6).
"""
import functools
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import prefill_rope_ref as R  # noqa: E402
from prefill_rope_ref import D, EPS, Pool  # noqa: E402
from test_ops_gpu import NM_F32SCORES, _attn_ref, assert_close_ulps  # noqa: E402

pytestmark = pytest.mark.gpu

K_ULPS, K_EXACT = 2, 0.97            # test_ops_gpu.py::test_qknorm_rope
TAB_EXACT = 0.999                    # tests/test_prefill_rope_cpu.py: torch's own f32 cos / sin reach it on these positions
FORMS = {"table": 0, "no_table": 1, "device_start": 2, "packed": 3}
DEVICE_START_CASES = [(0, 17), (61, 16), (200, 77), (62, 15)]
NO_TABLE_CASES = [(0, 19), (5, 30), (200, 130)]
SHAPES = sorted({(nh, kvh) for nh, kvh, _ in R.HEAD_SHAPES})


@functools.lru_cache(maxsize=None)
def rows_case(nh, kvh, S, half_k=False):
    """Inputs and reference of S rows of one head shape, computed once and shared by every call on them.  half_k (the attention cases): a k
    norm weight around 0.5 instead of 1, see check_attention."""
    qkv = R.rnd((S, (nh + 2 * kvh) * D), 300 + S)
    qn, kn = R.norm_weights()
    if half_k:
        kn = R.rnd((D,), 9, 0.05, 0.5)
    pos, axis, inv = R.positions(S), R.axis_mixed(), R.inv_freq()
    tab = R.table_ref(pos, axis, inv)
    q, k, v = R.rope_ref(qkv, qn, kn, tab, nh, kvh)
    return dict(nh=nh, kvh=kvh, S=S, qkv=qkv, qn=qn, kn=kn, pos=pos, axis=axis, inv=inv, tab=tab, q=q, k=k, v=v)


def launch_rope(c, ptrs, form, kv_start=0, skip_q=0, row_slot=None, page_rows=None, rows=None):
    """-> (table, q) on the CPU; rows: a slice of the case's rows (their own positions travel with them)."""
    from aha_amd import ops
    sl = slice(None) if rows is None else rows
    tab, q = ops.debug_prefill_rope(c["qkv"][sl].contiguous().cuda(), c["qn"].cuda(), c["kn"].cuda(), c["pos"][:, sl].contiguous().cuda(),
                                    c["axis"].cuda(), c["inv"].cuda(), ptrs, c["nh"], c["kvh"], EPS, FORMS[form], kv_start, skip_q, row_slot,
                                    page_rows)
    return tab.cpu(), q.cpu()


class Stats:
    """Worst ulp distance and smallest bit-identical share per (head shape, form), printed for the module docstring."""

    def __init__(self):
        self.d = {}

    def add(self, key, got, ref):
        w, e = self.d.get(key, (0.0, 1.0))
        self.d[key] = (max(w, R.worst_ulps(got, ref)), min(e, R.exact_share(got, ref)))

    def dump(self):
        for key, (w, e) in self.d.items():
            print("MEASURED", *key, f"worst={w:.3f} exact={e:.4f}")


def check_write(what, c, pool, image, q, written, skip_q, stats, key, rows=None):
    """Every assertion on one call: `written` = [(pool sequence, its cache tokens, the rows of the case that went there)], image = the pool
    read back, q = the call's q output."""
    nh, kvh = c["nh"], c["kvh"]
    for r, toks, rws in written:
        k_got, v_got = R.read_tokens(image, pool, r, toks)
        assert R.same_bits(v_got, c["v"][rws]), f"{what}: V of sequence {r} is not the qkv rows' bit for bit"
        stats.add(key + ("k",), k_got, c["k"][rws])
        assert_close_ulps(k_got, c["k"][rws], K_ULPS, K_EXACT, f"{what}: K of sequence {r}")
    m = R.untouched_mask(pool, [(r, toks) for r, toks, _ in written])
    diff = (image.view(torch.int16) != pool.host.view(torch.int16)) & m
    assert not diff.any(), f"{what}: {int(diff.sum())} pool elements outside the written slots changed"
    sl = slice(None) if rows is None else rows
    if skip_q:
        assert not q.view(torch.int16).any(), f"{what}: skip_q, yet q was written"
    else:
        stats.add(key + ("q",), q, c["q"][sl])
        assert_close_ulps(q, c["q"][sl], K_ULPS, K_EXACT, f"{what}: q")


def one_sequence_call(nh, kvh, off, S, form, skip_q, stats, repeat=False):
    c = rows_case(nh, kvh, S)
    pool = Pool(kvh, [off + S], 50 + off + S)
    R.prefill_prefix(pool, 0, off, 400 + off)
    pool.upload()
    try:
        ptrs = pool.ptrs[: pool.npg[0]].contiguous()
        what = f"nh {nh} kvh {kvh} offset {off} S {S} {form} skip_q {skip_q}"
        tab, q = launch_rope(c, ptrs, form, off, skip_q)
        image = pool.dev.cpu()
        toks = torch.arange(off, off + S)
        check_write(what, c, pool, image, q, [(0, toks, slice(None))], skip_q, stats, (nh, kvh, skip_q, form))
        assert int((R.bf16_ordinal(tab) - R.bf16_ordinal(c["tab"])).abs().max()) <= 1, f"{what}: table"
        if repeat:   # (e) the same launch on the restored pool: the same bits
            pool.restore()
            tab2, q2 = launch_rope(c, ptrs, form, off, skip_q)
            assert R.same_bits(tab, tab2) and R.same_bits(q, q2) and R.same_bits(image, pool.dev.cpu()), f"{what}: a repeat launch gave other bits"
    finally:
        del pool.dev, pool.before, pool.ptrs


def packed_call(nh, kvh, lens, kv0s, stats):
    S = sum(lens)
    c = rows_case(nh, kvh, S)
    pool = Pool(kvh, [k0 + ln for ln, k0 in zip(lens, kv0s)], 70 + sum(kv0s))
    for j, k0 in enumerate(kv0s):
        R.prefill_prefix(pool, j, k0, 500 + 2 * j)
    pool.upload()
    try:
        pages, slot, prow = R.packed_plan(lens, kv0s, pool.page0)
        ptrs = pool.ptrs[torch.tensor(pages, device="cuda")].contiguous()
        what = f"nh {nh} kvh {kvh} packed {lens} kv0 {kv0s}"
        _, q = launch_rope(c, ptrs, "packed", 0, 1, slot, prow)
        image = pool.dev.cpu()
        written, r0 = [], 0
        for j, (ln, k0) in enumerate(zip(lens, kv0s)):
            written.append((j, torch.arange(k0, k0 + ln), slice(r0, r0 + ln)))
            r0 += ln
        check_write(what, c, pool, image, q, written, 1, stats, (nh, kvh, 1, "packed" + ("_kv0" if any(kv0s) else "")))
    finally:
        del pool.dev, pool.before, pool.ptrs


# ---- (a) the table -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mrope", [False, True])
def test_rope_table_against_f64_cos_sin(gpu, mrope):
    """Every entry within one representable bf16 value of bf16(f32(cos_f64(angle))): the kernel rounds a value whose own error is far
    below a bf16 ulp, so it lands on the reference or its neighbour; >= 0.999 of them on the reference itself."""
    t = torch.tensor(R.TABLE_POSITIONS, dtype=torch.int32)
    S = t.numel()
    pos = torch.stack([t, t.roll(300), t.roll(600)] if mrope else [t, t, t]).contiguous()
    axis = R.axis_mixed() if mrope else R.axis_plain()
    nh, kvh = 4, 2
    c = dict(rows_case(nh, kvh, S), pos=pos, axis=axis)
    ref = R.table_ref(pos, axis, c["inv"])
    pool = Pool(kvh, [S], 31)
    pool.upload()
    try:
        tab, _ = launch_rope(c, pool.ptrs[: pool.npg[0]].contiguous(), "table", 0, 0)
    finally:
        del pool.dev, pool.before, pool.ptrs
    dist = (R.bf16_ordinal(tab) - R.bf16_ordinal(ref)).abs()
    share = float((dist == 0).float().mean())
    print(f"MEASURED table mrope={mrope} entries={dist.numel()} worst={int(dist.max())} exact={share:.5f}")
    assert torch.isfinite(tab.float()).all()
    assert int(dist.max()) <= 1, f"{int((dist > 1).sum())} table entries more than one bf16 value from the reference"
    assert share >= TAB_EXACT, f"only {share:.5f} of the table bit-identical to the reference"


# ---- (b), (e) pages after the write ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nh,kvh,skip_q", R.HEAD_SHAPES)
def test_pages_after_the_write(gpu, nh, kvh, skip_q):
    """The model's prefill call at every (cache offset, S), each launched twice; the device-scalar form and the form without a table on a
    subset; the packed form on segments with pages of their own, without and with cache prefixes."""
    stats = Stats()
    for off, S in R.OFFSET_CASES:
        one_sequence_call(nh, kvh, off, S, "table", skip_q if S >= 16 else 0, stats, repeat=True)
    for off, S in NO_TABLE_CASES:
        one_sequence_call(nh, kvh, off, S, "no_table", skip_q, stats)
    if not skip_q or (nh, kvh, 0) not in R.HEAD_SHAPES:   # (the per-element kernel knows no skip_q: once per head shape)
        for off, S in DEVICE_START_CASES:
            one_sequence_call(nh, kvh, off, S, "device_start", 0, stats)
    if skip_q or (nh, kvh, 1) not in R.HEAD_SHAPES:       # (the packed form is skip_q by definition: once per head shape)
        packed_call(nh, kvh, R.PACKED_LENS, (0,) * len(R.PACKED_LENS), stats)
        packed_call(nh, kvh, R.PACKED_LENS, R.PACKED_KV0, stats)
    stats.dump()


# ---- (c) the forms agree bit for bit --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nh,kvh", SHAPES)
def test_the_forms_leave_the_same_bits(gpu, nh, kvh):
    """kernels_elem.hip claims the rows kernel bit-identical to the per-element kernel by construction, with the table or without: one call
    (offset 64, 83 rows: a full page and a partial one, a clamped last wave) through all four forms."""
    off, S = 64, 83
    c = rows_case(nh, kvh, S)
    pool = Pool(kvh, [off + S], 91)
    R.prefill_prefix(pool, 0, off, 600)
    pool.upload()
    try:
        ptrs = pool.ptrs[: pool.npg[0]].contiguous()
        out = {}
        for form in ("table", "no_table", "device_start"):
            pool.restore()
            _, q = launch_rope(c, ptrs, form, off, 0)
            out[form] = (pool.dev.cpu(), q)
        pool.restore()
        launch_rope(c, pool.ptrs[1: pool.npg[0]].contiguous(), "packed", 0, 1, list(range(S)), [(0, 64), (64, S - 64)])
        out["packed"] = (pool.dev.cpu(), None)
        assert not R.same_bits(out["table"][0], pool.host), "nothing was written"
        for form in ("no_table", "device_start", "packed"):
            assert R.same_bits(out["table"][0], out[form][0]), f"{form}: K / V pages differ from the table form's"
            if out[form][1] is not None:
                assert R.same_bits(out["table"][1], out[form][1]), f"{form}: q differs from the table form's"
    finally:
        del pool.dev, pool.before, pool.ptrs


# ---- (d) Q fused into the attention ---------------------------------------------------------------------------------------------------------
def check_attention(what, o, q, k, v, nh, kvh, off):
    """tests/test_engine_gpu.py's bounds: 3 ulps at row scale from the oracle with the f32 score chain's rounding points, 4 from the eager
    one.  The eager oracle rounds every score to bf16 twice, up to 2^-8 |score| each way, and a probability moves by as much; with keys of
    the q heads' size (|score| up to ~5) the two ORACLES are 3 - 6 ulps apart on these rows (computed on the CPU, no kernel involved), and
    the second bound would measure the conventions, not the kernel.  So the attention cases halve the keys -- a k norm weight around 0.5
    (rows_case half_k) and cached prefix keys of std 0.5 -- which brings the oracles within 2 ulps of each other on every case here."""
    assert_close_ulps(o, _attn_ref(q, k, v, nh, kvh, D, True, off, NM_F32SCORES), 3, None, what + " vs the f32-score oracle", row_scale=True)
    assert_close_ulps(o, _attn_ref(q, k, v, nh, kvh, D, True, off), 4, None, what + " vs the eager oracle", row_scale=True)


def overrides(fn):
    @functools.wraps(fn)
    def run(*a, **kw):
        from aha_amd import ops
        try:
            ops.attn_form(16)
            ops.attn_variant(-1)
            return fn(*a, **kw)
        finally:
            ops.attn_form(-1)
            ops.attn_variant(-1)
    return run


@pytest.mark.parametrize("half_k", [True, False])
@pytest.mark.parametrize("S,off", [(16, 0), (65, 0), (130, 64), (100, 333)])
@pytest.mark.parametrize("nh,kvh", [(8, 2), (32, 8)])
@overrides
def test_q_fused_into_the_attention_single_sequence(gpu, nh, kvh, S, off, half_k):
    """The attention reading the raw q heads gives the bits of the attention reading the rope kernel's q, over the pages that kernel wrote.
    With keys of full size (half_k False: the score magnitudes of a model) the bit-identity alone, which needs no oracle; with halved keys
    the two oracle bounds as well (check_attention)."""
    from aha_amd import ops
    c = rows_case(nh, kvh, S, half_k=half_k)
    pool = Pool(kvh, [off + S], 110 + S)
    R.prefill_prefix(pool, 0, off, 700, 0.5 if half_k else 1.0)
    pool.upload()
    try:
        ptrs = pool.ptrs[: pool.npg[0]].contiguous()
        what = f"nh {nh} kvh {kvh} S {S} offset {off} half_k {half_k}"
        tab, q = launch_rope(c, ptrs, "table", off, 0)
        image = pool.dev.cpu()
        check_write(what, c, pool, image, q, [(0, torch.arange(off, off + S), slice(None))], 0, Stats(), ())
        k, v = R.read_tokens(image, pool, 0, torch.arange(off + S))
        fused = ops.debug_prefill_attn_qfuse(c["qkv"].cuda(), c["qn"].cuda(), tab.cuda(), ptrs, nh, kvh, EPS, off, off + S).cpu()
        plain = ops.attn_prefill(q.cuda(), k.cuda(), v.cuda(), nh, kvh, D, off, True).cpu()
        assert R.same_bits(image, pool.dev.cpu()), f"{what}: the attention wrote to the pool"
        assert R.same_bits(fused, plain), f"{what}: {int((fused.view(torch.int16) != plain.view(torch.int16)).sum())} output elements differ from the un-fused path's"
        if half_k:
            check_attention(what, fused, q, k, v, nh, kvh, off)
    finally:
        del pool.dev, pool.before, pool.ptrs


@pytest.mark.parametrize("nh,kvh", [(32, 8), (8, 2)])
@overrides
def test_q_fused_two_segments_in_one_call(gpu, nh, kvh):
    """AttnPrefillArgs::S2: (32, 8) is one launch with the second segment's rows from row S on inside the kernel; (8, 2) has no XCD-aware
    order, the launcher splits it and moves q, o and q_rope_tab on by S rows."""
    from aha_amd import ops
    S1, off1, S2, off2 = 40, 30, 50, 150
    c = rows_case(nh, kvh, S1 + S2, half_k=True)
    pool = Pool(kvh, [off2 + S2], 130)
    R.prefill_prefix(pool, 0, off2, 710, 0.5)
    pool.upload()
    try:
        ptrs = pool.ptrs[: pool.npg[0]].contiguous()
        what = f"nh {nh} kvh {kvh} two segments"
        tab1, q1 = launch_rope(c, ptrs, "table", off1, 0, rows=slice(0, S1))
        tab2, q2 = launch_rope(c, ptrs, "table", off2, 0, rows=slice(S1, S1 + S2))
        tab, q = torch.cat([tab1, tab2]), torch.cat([q1, q2])
        assert not R.same_bits(tab1[:S1], tab2[:S1])   # (a table that is not moved on for the second segment would show)
        image = pool.dev.cpu()
        check_write(what, c, pool, image, q, [(0, torch.arange(off1, off1 + S1), slice(0, S1)), (0, torch.arange(off2, off2 + S2), slice(S1, S1 + S2))],
                    0, Stats(), ())
        k, v = R.read_tokens(image, pool, 0, torch.arange(off2 + S2))
        fused = ops.debug_prefill_attn_qfuse(c["qkv"].cuda(), c["qn"].cuda(), tab.cuda(), ptrs, nh, kvh, EPS, off1, off1 + S1,
                                             seg2=(S2, off2, off2 + S2)).cpu()
        plain = torch.cat([ops.attn_prefill(q1.cuda(), k[: off1 + S1].cuda(), v[: off1 + S1].cuda(), nh, kvh, D, off1, True).cpu(),
                           ops.attn_prefill(q2.cuda(), k.cuda(), v.cuda(), nh, kvh, D, off2, True).cpu()])
        assert R.same_bits(fused[:S1], plain[:S1]), f"{what}: first segment differs from the un-fused path's"
        assert R.same_bits(fused[S1:], plain[S1:]), f"{what}: second segment differs from the un-fused path's"
        check_attention(what + ", first", fused[:S1], q1, k[: off1 + S1], v[: off1 + S1], nh, kvh, off1)
        check_attention(what + ", second", fused[S1:], q2, k, v, nh, kvh, off2)
    finally:
        del pool.dev, pool.before, pool.ptrs


@pytest.mark.parametrize("with_kv0", [False, True])
@pytest.mark.parametrize("nh,kvh", [(8, 2), (32, 8)])
@overrides
def test_q_fused_packed(gpu, nh, kvh, with_kv0):
    """The packed launch (seg_tab / seg_items, optional seg_kv0) over pages the packed rope form wrote, against ops.attn_prefill_segs fed the q
    of the un-fused rope stage and the token-major K / V unpacked from those pages."""
    from aha_amd import ops
    lens = R.PACKED_LENS
    kv0s = R.PACKED_KV0 if with_kv0 else (0,) * len(lens)
    S = sum(lens)
    c = rows_case(nh, kvh, S, half_k=True)
    pool = Pool(kvh, [k0 + ln for ln, k0 in zip(lens, kv0s)], 150)
    for j, k0 in enumerate(kv0s):
        R.prefill_prefix(pool, j, k0, 720 + 2 * j, 0.5)
    scratch = Pool(kvh, [S], 151)   # the un-fused rope stage writes its K / V here; only its q is used
    pool.upload()
    scratch.upload()
    try:
        what = f"nh {nh} kvh {kvh} packed, kv0 {kv0s}"
        pages, slot, prow = R.packed_plan(lens, kv0s, pool.page0)
        tab, _ = launch_rope(c, pool.ptrs[torch.tensor(pages, device="cuda")].contiguous(), "packed", 0, 1, slot, prow)
        _, q = launch_rope(c, scratch.ptrs[: scratch.npg[0]].contiguous(), "table", 0, 0)
        image = pool.dev.cpu()
        written, r0 = [], 0
        for j, (ln, k0) in enumerate(zip(lens, kv0s)):
            written.append((j, torch.arange(k0, k0 + ln), slice(r0, r0 + ln)))
            r0 += ln
        check_write(what, c, pool, image, torch.zeros_like(q), written, 1, Stats(), ())
        assert_close_ulps(q, c["q"], K_ULPS, K_EXACT, what + ": q of the un-fused rope stage")
        caches = [R.read_tokens(image, pool, j, torch.arange(k0 + ln)) for j, (ln, k0) in enumerate(zip(lens, kv0s))]
        k, v = torch.cat([kc for kc, _ in caches]), torch.cat([vc for _, vc in caches])
        n_ptrs = sum(pool.npg)
        fused = ops.debug_prefill_attn_qfuse(c["qkv"].cuda(), c["qn"].cuda(), tab.cuda(), pool.ptrs[:n_ptrs].contiguous(), nh, kvh, EPS,
                                             segs=[(ln, p0, k0) for ln, p0, k0 in zip(lens, pool.page0, kv0s)], with_kv0=with_kv0).cpu()
        plain = ops.attn_prefill_segs(q.cuda(), k.cuda(), v.cuda(), nh, kvh, list(zip(lens, kv0s)), with_kv0).cpu()
        assert R.same_bits(fused, plain), f"{what}: {int((fused.view(torch.int16) != plain.view(torch.int16)).sum())} output elements differ from the un-fused path's"
        r0 = 0
        for j, (ln, k0) in enumerate(zip(lens, kv0s)):
            check_attention(f"{what}, segment {j}", fused[r0:r0 + ln], q[r0:r0 + ln], caches[j][0], caches[j][1], nh, kvh, k0)
            r0 += ln
    finally:
        del pool.dev, pool.before, pool.ptrs, scratch.dev, scratch.before, scratch.ptrs


def test_the_64_row_form_takes_no_fused_q(gpu):
    """AHA_ERR_UNSUPPORTED where attn_prefill_takes_qfuse says no."""
    from aha_amd import _lib, ops
    nh, kvh, S = 8, 2, 65
    c = rows_case(nh, kvh, S)
    pool = Pool(kvh, [S], 170)
    pool.upload()
    try:
        ptrs = pool.ptrs[: pool.npg[0]].contiguous()
        tab, _ = launch_rope(c, ptrs, "table", 0, 0)
        ops.attn_form(65)
        with pytest.raises(_lib.AhaHipError) as e:
            ops.debug_prefill_attn_qfuse(c["qkv"].cuda(), c["qn"].cuda(), tab.cuda(), ptrs, nh, kvh, EPS, 0, S)
        assert e.value.code == -6   # AHA_ERR_UNSUPPORTED
    finally:
        ops.attn_form(-1)
        del pool.dev, pool.before, pool.ptrs
