"""-m gpu: ops.attn_decode_fused_kv8 (attn_decode_fused_kv8_kernel and its table twin, attn_decode_fused_body<true, LINEAR, KV8 = true>) on the
inputs, pools and f64 reference of tests/test_kv8_gpu.py, one launch per cache length: 1 (the new token only), 2, 64 / 65 (the append slot
on either side of a page boundary), 129, 257, 1025 (5 splits: merged in registers), 4500 (18 splits: merged through LDS).
table: the permuted pool's KV8 twin through its page table.  linear: the same pages in logical order at a constant stride of TWO pages,
other pages' bytes in between (a step taken from the bf16 page size, or a stride of one page, reads a wrong page); the table kernel then
runs over that layout too and has to give the linear kernel's bits.  Output: test_attn_decode_fused_gpu.ULPS against the f64 attention over
the DEQUANTISED cache; the KV8 pool afterwards = the pool before + quant.quantize_kv of the slots the bf16 kernel appends."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kv_pages  # noqa: E402
from rope_ref import D  # noqa: E402
from test_attn_decode_fused_gpu import EPS, ULPS  # noqa: E402
from test_kv8_gpu import LENS, Pool8, case  # noqa: E402
from test_ops_gpu import assert_close_ulps  # noqa: E402

from aha_amd import quant  # noqa: E402

pytestmark = pytest.mark.gpu
SINGLE_LENS = [1, 2, 64, 65, 129, 257, 1025, 4500]


@pytest.mark.parametrize("form", ["table", "linear"])
@pytest.mark.parametrize("nh,kvh", [(2, 2), (16, 1), (32, 8)])
def test_single_sequence_attention_over_kv8_pages(gpu, nh, kvh, form):
    from aha_amd import ops
    c = case(nh, kvh)
    pool, rows = c["pool"], [LENS.index(L) for L in SINGLE_LENS]
    p8 = Pool8(pool)
    qn, kn = c["qn"].to("cuda"), c["kn"].to("cuda")
    nbytes = p8.host.shape[1]
    # linear: logical page j at row 2 j, row 2 j + 1 holds logical page j - 1's bytes again (a stride of one page reads those)
    logical = p8.host[pool.perm]
    lin = torch.stack([logical, logical.roll(1, 0)], 1).reshape(-1, nbytes).to("cuda")

    def run(r, L, kind):
        args = (c["qkv"][r].contiguous().to("cuda"), qn, kn, c["rope"][r].contiguous().to("cuda"))
        if kind == "bf16":
            return ops.debug_attn_decode_fused(*args, pool.ptrs[pool.page0[r]:].contiguous(), L, nh, kvh, EPS, c["scale"])
        base = lin.data_ptr() + 2 * pool.page0[r] * nbytes
        if kind == "linear":
            return ops.attn_decode_fused_kv8(*args, None, base, 2 * nbytes, L, nh, kvh, EPS, c["scale"]).cpu()
        ptrs = p8.ptrs[pool.page0[r]:] if form == "table" else base + 2 * nbytes * torch.arange(pool.npg[r], device="cuda")
        return ops.attn_decode_fused_kv8(*args, ptrs.contiguous(), 0, 0, L, nh, kvh, EPS, c["scale"]).cpu()

    try:
        o, _ = [run(r, L, form) for r, L in zip(rows, SINGLE_LENS)], [run(r, L, "bf16") for r, L in zip(rows, SINGLE_LENS)]
        slots = [kv_pages.unpack_slot(pool.dev[pool.slot_elems(r)[1]].cpu(), kvh, pool.slot_elems(r)[2]) for r in rows]
        (kq, ks), (vq, vs) = (quant.quantize_kv(torch.stack([s[i] for s in slots]).view(-1, kvh, D)) for i in (0, 1))
        want = p8.with_slots(rows, kq, ks, vq, vs)
        if form == "table":
            assert torch.equal(p8.dev.cpu(), want), "the KV8 pool is not the old pool + the quantised appended slots"
        else:
            got = lin.cpu().view(-1, 2, nbytes)
            assert torch.equal(got[:, 0], want[pool.perm]), "the KV8 pages are not the old pages + the quantised appended slots"
            assert torch.equal(got[:, 1], logical.roll(1, 0)), "the linear kernel wrote into a page between its own"
            assert torch.equal(p8.dev.cpu(), p8.host)
            for i, (r, L) in enumerate(zip(rows, SINGLE_LENS)):   # (c) the same layout through the table kernel: the same bits
                assert torch.equal(run(r, L, "table").view(torch.int16), o[i].view(torch.int16)), f"kv_len {L}: table and linear outputs differ"
        for i, (r, L) in enumerate(zip(rows, SINGLE_LENS)):
            ref = c["ref_o"][r].to(torch.bfloat16)
            assert_close_ulps(o[i].view(nh, D), ref.view(nh, D), ULPS, None, f"{form} nh {nh} kvh {kvh} kv_len {L}, per head", row_scale=True)
            assert_close_ulps(o[i], ref, ULPS, None, f"{form} nh {nh} kvh {kvh} kv_len {L}, row rms")
    finally:
        del pool.dev, pool.before, pool.ptrs
