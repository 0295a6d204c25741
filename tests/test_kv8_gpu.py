"""-m gpu: the E4M3 KV cache at op level -- ops.quantize_kv_pages byte for byte against quant.quantize_kv + pack_kv8_pages, and
ops.attn_decode_batch_kv8 (attn_decode_fused_body<.., KV8>, aha_amd/csrc/attn_decode_body.h) against the f64 reference of
tests/test_attn_decode_fused_gpu.py over the DEQUANTISED cache, at that test's 3 bf16 ulps: both sides hold the same values, so FP8 earns
no looser bound.  Per-(token, kv head) K and V magnitudes vary by 2^-4 .. 2^4: a scale read from the wrong token, head or K / V half is an
O(1) error.  The pools are rope_ref.Pool's: finite garbage wherever no token was written, pages addressed through a permutation."""
import functools
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kv_pages  # noqa: E402
from rope_ref import D, Pool, norm_weights, prologue_ref, rnd  # noqa: E402
from test_attn_decode_fused_gpu import EPS, ULPS, bf16_scale, rope_rows, ulp_distance  # noqa: E402
from test_ops_gpu import assert_close_ulps  # noqa: E402

from aha_amd import quant  # noqa: E402

pytestmark = pytest.mark.gpu

SHAPES = [(2, 2), (8, 2), (16, 1), (32, 8)]
LENS = [1, 2, 64, 65, 129, 257, 300, 1025, 4500]


def tokens(L, kvh, seed):
    """(L, kvh * 128) bf16 with a magnitude of 2^-4 .. 2^4 per (token, kv head)."""
    mag = torch.exp2(torch.randint(-4, 5, (L, kvh, 1), generator=torch.Generator().manual_seed(seed)).float())
    return (rnd((L, kvh, D), seed + 1).float() * mag).to(torch.bfloat16).view(L, kvh * D)


def roundtrip(x, kvh):
    return quant.dequantize_kv(*quant.quantize_kv(x.view(-1, kvh, D))).view(x.shape)


def kv8_images(host, kvh):
    """bf16 page images (P, page elements) -> the KV8 images the reference quantiser gives for all 64 slots of every page."""
    kv = host[:, kv_pages.slot_index(kvh)]                                     # (P, 64, [k | v] (kvh * 128))
    (kq, ks), (vq, vs) = (quant.quantize_kv(x.reshape(-1, 64, kvh, D)) for x in (kv[..., : kvh * D], kv[..., kvh * D:]))
    return quant.pack_kv8_pages(kq, ks, vq, vs)


class Pool8:
    """A rope_ref.Pool (bf16) and its KV8 twin on the device, both addressed by the pool's permutation."""

    def __init__(self, pool):
        self.pool, self.host = pool, kv8_images(pool.host, pool.kvh)
        pool.upload()
        self.dev = self.host.to("cuda")
        self.ptrs = (self.dev.data_ptr() + pool.perm.to(torch.int64) * self.host.shape[1]).to("cuda")

    def with_slots(self, rows, kq, ks, vq, vs):
        """The host image with the slots that `rows` append to replaced by the given codes (rows, kvh, 128) and scales (rows, kvh)."""
        want = self.host.clone()
        idx = quant._kv8_index(self.pool.kvh)
        for i, r in enumerate(rows):
            _, pg, t = self.pool.slot_elems(r)
            for ix, val in zip(idx, (kq[i], vq[i], ks[i], vs[i])):
                want[pg, ix[t]] = val
        return want


@pytest.mark.parametrize("kvh", [1, 2, 8])
def test_quantize_kv_pages_equals_the_reference_quantiser(gpu, kvh):
    from aha_amd import ops
    lens = [66, 131, 3]
    pool = Pool(kvh, lens, 30 + kvh)
    for r, L in enumerate(lens):
        pool.write(r, tokens(L - 1, kvh, 300 + r), tokens(L - 1, kvh, 400 + r))
    pool.upload()
    P = pool.host.shape[0]
    assert ops.kv8_page_bytes(kvh) == quant.kv8_page_bytes(kvh) == 16512 * kvh
    dst = torch.full((P, 16512 * kvh), 0xa5, dtype=torch.uint8, device="cuda")
    ops.quantize_kv_pages(pool.ptrs, dst.data_ptr() + torch.arange(P, device="cuda") * dst.shape[1], kvh)
    torch.cuda.synchronize()
    assert torch.equal(dst.cpu(), kv8_images(pool.host, kvh)[pool.perm]), "KV8 page bytes differ from quantize_kv + pack_kv8_pages"


@functools.lru_cache(maxsize=None)
def case(nh, kvh):
    """Inputs and the f64 reference of one head shape: every cache length is one sequence of the pool and one row of the launch."""
    R = len(LENS)
    pool = Pool(kvh, LENS, 50)
    qkv, (qn, kn), rope, scale = rnd((R, (nh + 2 * kvh) * D), 51), norm_weights(), rope_rows(R, 52), bf16_scale()
    ref_o = []
    for r, L in enumerate(LENS):
        kc, vc = tokens(L - 1, kvh, 500 + r), tokens(L - 1, kvh, 600 + r)
        pool.write(r, kc, vc)
        # test_attn_decode_fused_gpu.fused_ref's body restated: that function takes the new token's k and v from the prologue itself, and
        # here they pass through the quantiser like every cached token
        q, k_new, v_new = prologue_ref(qkv[r], qn, kn, rope[r], nh, kvh, EPS)
        K = torch.cat([roundtrip(kc, kvh).view(-1, kvh, D), roundtrip(k_new, kvh)[None]]).double()
        V = torch.cat([roundtrip(vc, kvh).view(-1, kvh, D), roundtrip(v_new, kvh)[None]]).double()
        p = torch.softmax(torch.einsum("kgd,lkd->kgl", q.double().view(kvh, nh // kvh, D), K) * scale, -1)
        ref_o.append(torch.einsum("kgl,lkd->kgd", p, V).reshape(nh * D))
    return dict(nh=nh, kvh=kvh, pool=pool, qkv=qkv, qn=qn, kn=kn, rope=rope, scale=scale, ref_o=ref_o)


def launch(ops_fn, c, ptrs, rows, lens, **kw):
    pool = c["pool"]
    o = ops_fn(c["qkv"][rows].contiguous().to("cuda"), c["qn"].to("cuda"), c["kn"].to("cuda"), c["rope"][rows].contiguous().to("cuda"), ptrs,
               [pool.page0[r] for r in rows], lens, c["nh"], c["kvh"], EPS, c["scale"], **kw)
    torch.cuda.synchronize()
    return None if o is None else o.cpu()


@pytest.mark.parametrize("nh,kvh", SHAPES)
def test_attention_over_kv8_pages_against_the_f64_reference(gpu, nh, kvh):
    """All lengths as rows of one launch: the output; the appended codes and scale bytes = quantize_kv of the slot the bf16 kernel appends
    on the same inputs (the prologue is shared code, so those bits are the kernel's own k); nothing else in the KV8 pool changes."""
    from aha_amd import ops
    c = case(nh, kvh)
    pool, rows = c["pool"], list(range(len(LENS)))
    p8 = Pool8(pool)
    o = launch(ops.attn_decode_batch_kv8, c, p8.ptrs, rows, LENS)
    launch(ops.attn_decode_batch, c, pool.ptrs, rows, LENS)
    slots = [kv_pages.unpack_slot(pool.dev[pool.slot_elems(r)[1]].cpu(), kvh, pool.slot_elems(r)[2]) for r in rows]
    (kq, ks), (vq, vs) = (quant.quantize_kv(torch.stack([s[i] for s in slots]).view(-1, kvh, D)) for i in (0, 1))
    assert torch.equal(p8.dev.cpu(), p8.with_slots(rows, kq, ks, vq, vs)), "the KV8 pool is not the old pool + the quantised appended slots"
    for r, L in enumerate(LENS):
        got, ref = o[r], c["ref_o"][r].to(torch.bfloat16)
        print(f"ULP-KV8 nh={nh} kvh={kvh} kv_len={L} head={ulp_distance(got.view(nh, D), ref.view(nh, D), ref.float().view(nh, D).abs().amax(-1, keepdim=True)):.3f}"
              f" rms={ulp_distance(got, ref, ref.float().pow(2).mean().sqrt()):.3f}")
        assert_close_ulps(got.view(nh, D), ref.view(nh, D), ULPS, None, f"nh {nh} kvh {kvh} kv_len {L}, per head", row_scale=True)
        assert_close_ulps(got, ref, ULPS, None, f"nh {nh} kvh {kvh} kv_len {L}, row rms")
    del pool.dev, pool.before, pool.ptrs


@pytest.mark.parametrize("nh,kvh", [(8, 2), (32, 8)])
def test_append_then_attend_forms_equal_the_fused_launch(gpu, nh, kvh):
    """Rows of ONE sequence at ascending lengths across a page boundary (a last token and its drafts): the append alone (form 2) and
    append-then-attend (form 1) write the bytes of one-row fused launches (form 0) in order, and form 1 gives their output bits."""
    from aha_amd import ops
    c = dict(case(nh, kvh))
    seq = LENS.index(65)                        # 64 cached tokens: page 0 is full and page 1 holds the sequence's own garbage
    c["pool"] = pool = Pool(kvh, [67], 70)
    pool.write(0, tokens(62, kvh, 71), tokens(62, kvh, 72))
    p8 = Pool8(pool)
    pool.page0 = [0] * len(LENS)                       # the four rows share the sequence's pages
    rows, lens = [seq, seq + 1, seq + 2, seq + 3], [63, 64, 65, 66]
    outs = [launch(ops.attn_decode_batch_kv8, c, p8.ptrs, [r], [L], form=0) for r, L in zip(rows, lens)]
    fused = p8.dev.clone()
    p8.dev.copy_(p8.host)
    assert launch(ops.attn_decode_batch_kv8, c, p8.ptrs, rows, lens, form=2) is None
    assert torch.equal(p8.dev, fused), "form 2 wrote other bytes than the fused launches"
    p8.dev.copy_(p8.host)
    o1 = launch(ops.attn_decode_batch_kv8, c, p8.ptrs, rows, lens, form=1)
    assert torch.equal(p8.dev, fused), "form 1 wrote other bytes than the fused launches"
    assert torch.equal(o1.view(torch.int16), torch.cat(outs).view(torch.int16)), "form 1's output bits differ from the fused launches'"
