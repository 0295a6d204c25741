"""The host mirror of the KV page layout (tests/kv_pages.py) against the layout as aha_amd/csrc/common.h states it, and the f64 reference
of the fused decode attention (tests/test_attn_decode_fused_gpu.py fused_ref) against oracle.qwen3 -- no GPU, no kernel involved."""
import os
import sys

import torch

from oracle import qwen3 as oq
from oracle.numerics import Numerics

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kv_pages  # noqa: E402
from test_attn_decode_fused_gpu import fused_ref, rnd, rope_rows, bf16_scale  # noqa: E402
from test_ops_gpu import assert_close_ulps  # noqa: E402


def test_element_maps_are_bijections():
    for KS in (2, 4):
        assert sorted(kv_pages.kpage_elem(t, e, KS) for t in range(64) for e in range(32 * KS)) == list(range(64 * 32 * KS))
    assert sorted(kv_pages.vpage_elem(t, e) for t in range(64) for e in range(128)) == list(range(64 * 128))
    assert sorted(kv_pages.v_slot(t) for t in range(64)) == list(range(64))


def test_pinned_values_worked_out_by_hand_from_the_header():
    assert kv_pages.kpage_elem(0, 0, 4) == 0
    # token 17 = sub 1, c 1; dim 45 = k4 1, G 1, j 5: fragment 1 * 4 + 1 = 5, piece 1 * 16 + 1 = 17 -> 5 * 512 + 17 * 8 + 5
    assert kv_pages.kpage_elem(17, 45, 4) == 2701
    # token 16 = kk 0, sub1 1, G 0, j 0 -> slot 4; dim 0: fragment 0, piece 0 -> element 4
    assert kv_pages.v_slot(16) == 4
    assert kv_pages.vpage_elem(16, 0) == 4
    # token 47 = kk 1, sub1 0, G 3, j 3 -> slot 32 + 24 + 3 = 59 = kk 1, G 3, j 3; dim 21 = ds 1, c 5: fragment 3, piece 53
    assert kv_pages.v_slot(47) == 59
    assert kv_pages.vpage_elem(47, 21) == 1963


def test_pack_pages_round_trips_every_token():
    kvh, L = 2, 130
    k, v = rnd((L, kvh * 128), 1), rnd((L, kvh * 128), 2)
    filled = rnd((3, kv_pages.page_elems(kvh)), 3, 100.0)
    pages = kv_pages.pack_pages(k, v, kvh, out=filled.clone())
    assert pages.shape == (3, 2 * kvh * 64 * 128)
    for i in range(L):
        kk, vv = kv_pages.unpack_slot(pages[i // 64], kvh, i % 64)
        assert torch.equal(kk, k[i]) and torch.equal(vv, v[i]), i
    # the slots of tokens >= L keep what the caller put there, and the slot masks of a page partition it
    tail = torch.zeros(kv_pages.page_elems(kvh), dtype=torch.bool)
    for t in range(L % 64, 64):
        tail |= kv_pages.slot_mask(kvh, t)
    assert torch.equal(pages[2][tail], filled[2][tail]) and not torch.equal(pages[2][~tail], filled[2][~tail])
    count = sum(kv_pages.slot_mask(kvh, t).long() for t in range(64))
    assert torch.equal(count, torch.ones_like(count))
    assert int(kv_pages.slot_mask(kvh, 5).sum()) == 2 * kvh * 128
    zeros = kv_pages.pack_pages(k, v, kvh)
    assert not zeros[2][tail].any() and torch.equal(zeros[2][~tail], pages[2][~tail])


def test_k_fragment_pieces_are_what_the_header_says_a_lane_loads():
    """Lane l = G * 16 + c: its 16-byte piece of K fragment (sub, k4) is dims k4*32 + G*8 .. +8 of token sub*16 + c."""
    kvh = 2
    k, v = rnd((64, kvh * 128), 4), rnd((64, kvh * 128), 5)
    page = kv_pages.pack_pages(k, v, kvh)[0]
    for h in range(kvh):
        block = page[h * 8192: (h + 1) * 8192].view(16, 64, 8)   # [fragment sub * 4 + k4][lane][8 elements]
        for sub in range(4):
            for k4 in range(4):
                for lane in range(64):
                    G, c = lane // 16, lane % 16
                    d0 = h * 128 + k4 * 32 + G * 8
                    assert torch.equal(block[sub * 4 + k4, lane], k[sub * 16 + c, d0: d0 + 8]), (h, sub, k4, lane)


def test_v_fragment_pieces_are_what_the_header_says_a_lane_loads():
    """Lane l = G * 16 + c: its piece of V fragment (ds, kk) is slots kk*32 + G*8 .. +8 of dim ds*16 + c, slot kk*32 + G*8 + sub1*4 + j
    holding token kk*32 + sub1*16 + G*4 + j."""
    kvh = 2
    k, v = rnd((64, kvh * 128), 6), rnd((64, kvh * 128), 7)
    page = kv_pages.pack_pages(k, v, kvh)[0]
    for h in range(kvh):
        block = page[(kvh + h) * 8192: (kvh + h + 1) * 8192].view(16, 64, 8)   # [fragment ds * 2 + kk][lane][8 slots]
        for ds in range(8):
            for kk in range(2):
                for lane in range(64):
                    G, c = lane // 16, lane % 16
                    toks = [kk * 32 + sub1 * 16 + G * 4 + j for sub1 in range(2) for j in range(4)]
                    assert torch.equal(block[ds * 2 + kk, lane], v[toks, h * 128 + ds * 16 + c]), (h, ds, kk, lane)


def test_f64_reference_agrees_with_the_oracle():
    """rms_norm, apply_rotary_pos_emb and eager_attention_forward of oracle.qwen3 on the f32 score chain: q and k have the same rounding
    points in both, so what separates them is the oracle's bf16 P and f32 softmax against f64 -- within the rounding of the output, 1 bf16
    ulp at row scale."""
    nh, kvh, L, d = 4, 2, 70, 128
    nm = Numerics("bf16", matmul_f64=True, attn_scores_rounded=False)
    qkv = rnd((1, (nh + 2 * kvh) * d), 11)
    qn, kn = rnd((d,), 12, 0.1, 1.0), rnd((d,), 13, 0.1, 1.0)
    rope = rope_rows(1, 14)
    kc, vc = rnd((L - 1, kvh * d), 15), rnd((L - 1, kvh * d), 16)
    scale = bf16_scale()
    o, k_new, v_new = fused_ref(qkv[0], qn, kn, rope[0], kc, vc, nh, kvh, 1e-6, scale)

    q = oq.rms_norm(nm, qkv[:, : nh * d].float().reshape(1, 1, nh, d), qn.float(), 1e-6).transpose(1, 2)
    k = oq.rms_norm(nm, qkv[:, nh * d: (nh + kvh) * d].float().reshape(1, 1, kvh, d), kn.float(), 1e-6).transpose(1, 2)
    cos, sin = rope[:, :64].repeat(1, 2), rope[:, 64:].repeat(1, 2)
    q, k = oq.apply_rotary_pos_emb(nm, q, k, cos[None], sin[None])
    assert torch.equal(v_new, qkv[0, (nh + kvh) * d:])
    assert_close_ulps(k_new, k.reshape(-1), 2, 0.97, "k_new against the oracle")
    K = torch.cat([kc.float().reshape(1, L - 1, kvh, d).transpose(1, 2), k], 2)
    V = torch.cat([vc.float().reshape(1, L - 1, kvh, d).transpose(1, 2), qkv[:, (nh + kvh) * d:].float().reshape(1, 1, kvh, d).transpose(1, 2)], 2)
    assert scale == oq.attn_scale(nm, d)
    ref = oq.eager_attention_forward(nm, q, K, V, nh // kvh, None, scale).reshape(nh, d)
    assert_close_ulps(o.to(torch.bfloat16).reshape(nh, d), ref, 1, None, "f64 reference against the oracle", row_scale=True)
