"""CPU tier of tests/test_prefill_rope_gpu.py: the two test entries are in the header, the library and the ctypes table and refuse bad
arguments before any device work; the many-row f64 reference (tests/prefill_rope_ref.py) agrees with oracle.qwen3; and the caps the GPU
tests put on bit-identical shares hold for the reference ALONE -- with torch's f32 cos / sin in place of f64 ones it stays far above them, so
a kernel that misses a cap is off by more than an f32 cos / sin implementation may be."""
import ctypes as C
import os
import re
import sys

import torch

from oracle import qwen3 as oq
from oracle.numerics import Numerics

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import prefill_rope_ref as R  # noqa: E402
from prefill_rope_ref import D, EPS  # noqa: E402
from test_ops_gpu import assert_close_ulps  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = (("aha_hip_debug_prefill_rope", 22), ("aha_hip_debug_prefill_attn_qfuse", 21))


def test_entries_in_header_library_and_signatures(hip_lib):
    from aha_amd import _lib
    header = open(os.path.join(ROOT, "include", "aha_hip.h")).read()
    for name, nargs in ENTRIES:
        decl = re.search(r"\bint %s\(([^;]*)\);" % name, header)
        assert decl, name
        assert len(decl.group(1).split(",")) == nargs, name
        assert hasattr(hip_lib, name), name
        assert len(_lib.SIGNATURES[name][1]) == nargs, name
    for form, value in (("TABLE", 0), ("NO_TABLE", 1), ("DEVICE_START", 2), ("PACKED", 3)):
        assert re.search(r"#define AHA_ROPE_FORM_%s %d\b" % (form, value), header), form


def _rope_args(**kw):
    """A call that would be valid if its pointers were: every pointer a non-null dummy that a refused call never reads."""
    p = C.c_void_p(64)
    slot = (C.c_int32 * 20)(*range(20))
    prow = (C.c_int32 * 2)(0, 20)
    a = dict(qkv=p, q_norm_w=p, k_norm_w=p, pos=p, axis_map=p, inv_freq=p, page_ptrs=p, n_page_ptrs=2, S=20, nh=4, kvh=2, d=128, eps=EPS, form=0,
             kv_start=0, skip_q=0, row_slot=slot, page_rows=prow, n_pages=1, rope_tab=p, q_out=p, stream=None)
    a.update(kw)
    return list(a.values())


def _attn_args(**kw):
    p = C.c_void_p(64)
    a = dict(qkv=p, q_norm_w=p, rope_tab=p, page_ptrs=p, n_page_ptrs=2, S=20, nh=4, kvh=2, d=128, eps=EPS, scale=0.088, kv_offset=0, kv_total=20,
             S2=0, kv_offset2=0, kv_total2=0, segs=None, n_seg=0, with_kv0=0, o=p, stream=None)
    a.update(kw)
    return list(a.values())


def test_bad_arguments_are_refused_before_device_work(hip_lib):
    """Every case returns AHA_ERR_INVALID on a machine without a GPU: nothing touched the device (the dummy pointers were never read)."""
    rope, attn = hip_lib.aha_hip_debug_prefill_rope, hip_lib.aha_hip_debug_prefill_attn_qfuse
    for ptr in ("qkv", "q_norm_w", "k_norm_w", "pos", "axis_map", "inv_freq", "page_ptrs", "rope_tab", "q_out"):
        assert rope(*_rope_args(**{ptr: None})) == -1, ptr
        assert b"null" in hip_lib.aha_hip_last_error()
    seg = (C.c_int32 * 3)(20, 0, 0)
    bad_rope = [dict(S=0), dict(S=-3), dict(d=64), dict(nh=0), dict(kvh=0), dict(n_page_ptrs=0), dict(form=4), dict(form=-1), dict(skip_q=2),
                dict(kv_start=-1), dict(kv_start=109), dict(S=129), dict(kv_start=1 << 30),          # the cache range against 2 pages
                dict(form=2, skip_q=1), dict(skip_q=1, S=15), dict(form=3, skip_q=0),
                dict(form=3, skip_q=1, row_slot=None), dict(form=3, skip_q=1, page_rows=None), dict(form=3, skip_q=1, n_pages=0),
                dict(form=3, skip_q=1, n_pages=3),
                dict(form=3, skip_q=1, row_slot=(C.c_int32 * 20)(*([0] * 19 + [64]))),                # a slot past the call's one page
                dict(form=3, skip_q=1, row_slot=(C.c_int32 * 20)(*([-1] + [0] * 19))),
                dict(form=3, skip_q=1, page_rows=(C.c_int32 * 2)(0, 0)), dict(form=3, skip_q=1, page_rows=(C.c_int32 * 2)(0, 65)),
                dict(form=3, skip_q=1, page_rows=(C.c_int32 * 2)(1, 20)), dict(form=3, skip_q=1, page_rows=(C.c_int32 * 2)(-1, 4))]
    for kw in bad_rope:
        assert rope(*_rope_args(**kw)) == -1, kw
        assert hip_lib.aha_hip_last_error().startswith(b"debug_prefill_rope"), kw
    for ptr in ("qkv", "q_norm_w", "rope_tab", "page_ptrs", "o"):
        assert attn(*_attn_args(**{ptr: None})) == -1, ptr
    bad_attn = [dict(S=0), dict(d=64), dict(nh=34, kvh=2), dict(nh=5, kvh=2), dict(kvh=0), dict(n_page_ptrs=0),
                dict(kv_total=129), dict(kv_total=0), dict(kv_offset=-1), dict(kv_offset=1, kv_total=20),   # rows past kv_total
                dict(S2=-1), dict(S2=5, kv_offset2=30, kv_total2=129), dict(S2=5, kv_offset2=30, kv_total2=34), dict(S2=5, kv_offset2=-1, kv_total2=40),
                dict(n_seg=-1), dict(n_seg=1), dict(n_seg=1, segs=seg, S2=3),
                dict(n_seg=1, segs=(C.c_int32 * 3)(19, 0, 0)), dict(n_seg=1, segs=(C.c_int32 * 3)(0, 0, 0)),
                dict(n_seg=1, segs=(C.c_int32 * 3)(20, 2, 0)), dict(n_seg=1, segs=(C.c_int32 * 3)(20, -1, 0)),
                dict(n_seg=1, segs=(C.c_int32 * 3)(20, 0, 64)),                                             # a kv0 without with_kv0
                dict(n_seg=1, with_kv0=1, segs=(C.c_int32 * 3)(20, 0, 32)), dict(n_seg=1, with_kv0=1, segs=(C.c_int32 * 3)(20, 0, 128)),
                dict(n_seg=1, with_kv0=1, segs=(C.c_int32 * 3)(20, 1, 64))]
    for kw in bad_attn:
        assert attn(*_attn_args(**kw)) == -1, kw
        assert hip_lib.aha_hip_last_error().startswith(b"debug_prefill_attn_qfuse"), kw


def test_many_row_reference_against_the_oracle():
    """rms_norm + apply_rotary_pos_emb of oracle.qwen3 under Numerics("bf16", matmul_f64=True) on the same bf16 table: the same rounding points,
    f32 arithmetic between them in the oracle against f64 here.  An f32 intermediate is 2^-24 off in relative terms and a bf16 rounding
    decides at 2^-9, so a rounding flips about once in 2^14 elements and then by one ulp: 1 ulp, 0.999 bit-identical."""
    nm = Numerics("bf16", matmul_f64=True)
    nh, kvh, S = 6, 3, 77
    qkv = R.rnd((S, (nh + 2 * kvh) * D), 41)
    qn, kn = R.norm_weights()
    pos, axis, inv = R.positions(S), R.axis_mixed(), R.inv_freq()
    tab = R.table_ref(pos, axis, inv)
    q, k, v = R.rope_ref(qkv, qn, kn, tab, nh, kvh)
    oq_q = oq.rms_norm(nm, qkv[:, : nh * D].float().reshape(1, S, nh, D), qn.float(), EPS).transpose(1, 2)
    oq_k = oq.rms_norm(nm, qkv[:, nh * D: (nh + kvh) * D].float().reshape(1, S, kvh, D), kn.float(), EPS).transpose(1, 2)
    cos, sin = tab[:, :64].float().repeat(1, 2), tab[:, 64:].float().repeat(1, 2)
    oq_q, oq_k = oq.apply_rotary_pos_emb(nm, oq_q, oq_k, cos[None], sin[None])
    assert torch.equal(v, qkv[:, (nh + kvh) * D:])
    assert_close_ulps(q, oq_q.transpose(1, 2).reshape(S, nh * D), 1, 0.999, "q against the oracle")
    assert_close_ulps(k, oq_k.transpose(1, 2).reshape(S, kvh * D), 1, 0.999, "k against the oracle")
    # and the table is the oracle's own cos / sin of the same f32 angles, cast to bf16, up to the f32 library's last bit
    ang = R.angles_f32(pos, axis, inv)
    assert int((R.bf16_ordinal(tab) - R.bf16_ordinal(torch.cat([ang.cos(), ang.sin()], 1).to(torch.bfloat16))).abs().max()) <= 1


def test_table_cap_holds_for_an_f32_cos_sin():
    """The GPU test wants >= 0.999 of the table bit-identical to bf16(f32(cos_f64)).  torch's f32 cos / sin of the same f32 angles -- another
    correctly working f32 implementation -- reach it on the test's positions, plain and M-RoPE, and never leave the neighbouring bf16 value."""
    t = torch.tensor(R.TABLE_POSITIONS, dtype=torch.int32)
    inv = R.inv_freq()
    for pos, axis in ((torch.stack([t, t, t]), R.axis_plain()), (torch.stack([t, t.roll(300), t.roll(600)]), R.axis_mixed())):
        ref, f32 = R.table_ref(pos, axis, inv), R.table_ref(pos, axis, inv, f32_trig=True)
        assert ref.numel() == 2 * 62208
        dist = (R.bf16_ordinal(ref) - R.bf16_ordinal(f32)).abs()
        assert int(dist.max()) <= 1
        assert float((dist == 0).float().mean()) >= 0.9999


def test_page_caps_hold_for_an_f32_cos_sin():
    """The GPU test wants K and q within 2 bf16 ulps of the reference with >= 0.97 bit-identical.  The reference from torch's f32 cos / sin
    agrees with the reference from f64 ones to >= 0.995 on every row count the GPU test uses (a table entry that rounds the other way moves
    two elements of every head by at most one rounding of a product and one of the sum), and never by more than the 2 ulps."""
    nh, kvh = 8, 2
    qn, kn = R.norm_weights()
    axis, inv = R.axis_mixed(), R.inv_freq()
    for S in sorted({s for _, s in R.OFFSET_CASES} | {83, 90, sum(R.PACKED_LENS)}):
        qkv = R.rnd((S, (nh + 2 * kvh) * D), 300 + S)
        pos = R.positions(S)
        a = R.rope_ref(qkv, qn, kn, R.table_ref(pos, axis, inv), nh, kvh)
        b = R.rope_ref(qkv, qn, kn, R.table_ref(pos, axis, inv, f32_trig=True), nh, kvh)
        for x, y, what in ((a[0], b[0], "q"), (a[1], b[1], "k")):
            n_diff = int((x.float() != y.float()).sum())
            # (S = 1: 256 k elements, one flipped table entry moves 2 per head = 4 of them; the share bound only where it has the resolution)
            assert n_diff <= max(4 * kvh, int(0.005 * x.numel())), (S, what, n_diff)
            assert_close_ulps(y, x, 2, None, f"S {S} {what}")
