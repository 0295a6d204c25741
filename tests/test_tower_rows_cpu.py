"""CPU tier of tests/test_tower_rows_gpu.py: the towers' test entries are in the header, the library and the ctypes table and refuse bad
arguments before any device work; model creation refuses a tower width the LayerNorm kernel cannot cover; the host references
(tests/tower_rows_ref.py) agree with the oracle's restatements; the generalised page mirror is tests/kv_pages.py's at 128 / 128; and every
cap the GPU tests put on a bit-identical share holds for a torch f32 restatement ALONE on the tests' own inputs, so a kernel that misses one
is off by more than another correct f32 implementation is."""
import ctypes as C
import os
import re
import sys
from types import SimpleNamespace

import numpy as np
import torch

from oracle import qwen3 as oq
from oracle import qwen3_asr as oa
from oracle import qwen3vl as ov
from oracle.numerics import Numerics

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kv_pages  # noqa: E402
import tower_rows_ref as T  # noqa: E402
from test_ops_gpu import assert_close_ulps  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NM = Numerics("bf16", matmul_f64=True)
ENTRIES = (("aha_hip_debug_layernorm_rows", 8), ("aha_hip_debug_gemm_layernorm", 17), ("aha_hip_debug_vit_pos_embed", 11),
           ("aha_hip_debug_vit_rope", 16), ("aha_hip_debug_scatter_rows", 8), ("aha_hip_debug_audio_im2col1", 8),
           ("aha_hip_debug_im2col_nhwc", 7), ("aha_hip_debug_audio_tokens_gather", 7), ("aha_hip_debug_sinus_pe_add", 5),
           ("aha_hip_debug_kv_pack_generic", 11))


def test_entries_in_header_library_and_signatures(hip_lib):
    from aha_amd import _lib
    header = open(os.path.join(ROOT, "include", "aha_hip.h")).read()
    readme = open(os.path.join(ROOT, "tests", "tools", "README.md")).read()
    for name, nargs in ENTRIES:
        decl = re.search(r"\bint %s\(([^;]*)\);" % name, header)
        assert decl, name
        assert len(decl.group(1).split(",")) == nargs, name
        assert hasattr(hip_lib, name), name
        assert len(_lib.SIGNATURES[name][1]) == nargs, name
        assert "`%s`" % name in readme, name


P = C.c_void_p(64)   # a non-null dummy pointer that a refused call never reads


def _refused(hip_lib, name, good, bad_list):
    """Every variant of the valid-but-for-its-pointers call `good` in bad_list returns AHA_ERR_INVALID with the entry's name in the message."""
    fn = getattr(hip_lib, name)
    for kw in bad_list:
        a = dict(good)
        a.update(kw)
        assert fn(*a.values()) == -1, (name, kw)
        assert hip_lib.aha_hip_last_error().startswith(name[len("aha_hip_"):].encode()), (name, kw, hip_lib.aha_hip_last_error())


def _grid(*g):
    return (C.c_uint32 * len(g))(*g)


def test_bad_arguments_are_refused_before_device_work(hip_lib):
    """On a machine without a GPU: nothing touched the device, the dummy pointers were never read."""
    nulls = lambda *names: [{n: None} for n in names]
    _refused(hip_lib, "aha_hip_debug_layernorm_rows", dict(x=P, w=P, b=P, y=P, rows=4, dim=1152, eps=1e-6, stream=None),
             nulls("x", "w", "b", "y") + [dict(rows=0), dict(rows=-1), dict(dim=0), dict(dim=-8), dict(dim=148), dict(dim=1156), dict(dim=8200), dict(dim=16384)])
    _refused(hip_lib, "aha_hip_debug_gemm_layernorm",
             dict(A=P, W=P, C=P, M=5, N=1152, K=320, lda=320, ldw=320, ldc=1152, bias=P, residual=P, act=0, norm_w=P, norm_b=P, norm_out=P, eps=1e-6, stream=None),
             nulls("A", "W", "C", "norm_w", "norm_b", "norm_out") +
             [dict(M=0), dict(N=0), dict(K=0), dict(N=1156, ldc=1156), dict(K=324, lda=324, ldw=324), dict(N=8200, ldc=8200), dict(ldc=1160), dict(lda=316),
              dict(ldw=312), dict(act=4), dict(act=-1)])
    g1, g3 = _grid(1, 4, 6), _grid(1, 4, 6, 2, 6, 4, 1, 2, 2)
    _refused(hip_lib, "aha_hip_debug_vit_pos_embed",
             dict(grid=g1, n_grids=1, G=8, merge=2, table=P, x=P, N=24, D=144, idx=P, wt=P, stream=None),
             nulls("grid", "table", "x", "idx", "wt") +
             [dict(n_grids=0), dict(G=0), dict(merge=0), dict(D=0), dict(D=148), dict(N=23), dict(N=0), dict(grid=_grid(1, 3, 6), N=18), dict(grid=_grid(1, 4, 5), N=20),
              dict(grid=_grid(0, 4, 6), N=0), dict(grid=g3, n_grids=3, N=24)])
    _refused(hip_lib, "aha_hip_debug_vit_rope",
             dict(qkv=P, grid=g3, n_grids=3, merge=2, inv_freq=P, page_ptrs=P, n_page_ptrs=4, N=76, nh=2, hd=72, cs_tab=P, q_out=P, rowcol=P, page_of=P,
                  slot_of=P, stream=None),
             nulls("qkv", "grid", "inv_freq", "page_ptrs", "cs_tab", "q_out", "rowcol", "page_of", "slot_of") +
             [dict(hd=64), dict(hd=128), dict(nh=0), dict(n_grids=0), dict(merge=0), dict(N=75), dict(n_page_ptrs=3), dict(n_page_ptrs=0),  # 4 frames: 4 pages
              dict(grid=_grid(1, 10, 8), n_grids=1, N=80, n_page_ptrs=1), dict(grid=_grid(1, 5, 8), n_grids=1, N=40)])
    rows = (C.c_int32 * 3)(2, 0, 19)
    _refused(hip_lib, "aha_hip_debug_scatter_rows", dict(dst=P, src=P, rows=rows, n=3, dst_rows=20, D=256, add=0, stream=None),
             nulls("dst", "src", "rows") + [dict(n=0), dict(dst_rows=0), dict(D=0), dict(D=260), dict(add=2), dict(dst_rows=19),
                                            dict(rows=(C.c_int32 * 3)(2, -1, 5))])
    ch = (C.c_int32 * 6)(0, 130, 0, 0, 130, 1)
    _refused(hip_lib, "aha_hip_debug_audio_im2col1", dict(feat=P, ld=130, chunks=ch, C=2, mels=128, win=100, out=P, stream=None),
             nulls("feat", "chunks", "out") + [dict(C=0), dict(mels=0), dict(win=0), dict(ld=0), dict(ld=129),          # the clip runs past the row
                                               dict(chunks=(C.c_int32 * 6)(0, 130, 0, 0, 130, 2)),                      # a window past its clip
                                               dict(chunks=(C.c_int32 * 6)(-1, 130, 0, 0, 130, 1)), dict(chunks=(C.c_int32 * 6)(0, 0, 0, 0, 130, 1))])
    _refused(hip_lib, "aha_hip_debug_im2col_nhwc", dict(x=P, out=P, B=2, Hin=32, Win=25, Cin=480, stream=None),
             nulls("x", "out") + [dict(B=0), dict(Hin=0), dict(Win=0), dict(Cin=0), dict(Cin=484)])
    _refused(hip_lib, "aha_hip_debug_audio_tokens_gather", dict(x=P, out=P, B=2, Fq=16, T=13, Cc=32, stream=None),
             nulls("x", "out") + [dict(B=0), dict(Fq=0), dict(T=0), dict(Cc=0)])
    _refused(hip_lib, "aha_hip_debug_sinus_pe_add", dict(x=P, rows=39, d=128, T=13, stream=None),
             nulls("x") + [dict(rows=0), dict(d=0), dict(d=127), dict(T=0)])
    slot = (C.c_int32 * 3)(0, 64, 127)
    _refused(hip_lib, "aha_hip_debug_kv_pack_generic",
             dict(src=P, ld=384, k_off=128, v_off=256, page_ptrs=P, n_page_ptrs=2, N=3, nh=2, hd=64, slot_of=slot, stream=None),
             nulls("src", "page_ptrs") + [dict(N=0), dict(nh=0), dict(hd=0), dict(hd=72), dict(n_page_ptrs=0), dict(n_page_ptrs=1), dict(ld=380), dict(k_off=-1),
                                          dict(v_off=260), dict(slot_of=(C.c_int32 * 3)(0, 64, 128)), dict(slot_of=(C.c_int32 * 3)(-1, 0, 1)),
                                          dict(slot_of=None, N=129)])


def test_model_create_refuses_tower_widths_the_layernorm_cannot_cover(hip_lib):
    """launch_layernorm_rows holds a row of at most 8192 elements in 16-byte pieces and would normalise a prefix of a wider or ragged one:
    creation refuses such a vision (hidden, or hidden * merge^2 of the post-shuffle norm) or audio width, before it touches the device."""
    from aha_amd import _lib
    ctx = C.create_string_buffer(256)
    out = C.c_void_p()
    name = b"model.visual.patch_embed.proj.weight"

    def create(**kw):
        d = _lib.ModelDesc()
        d.arch, d.hidden_size, d.intermediate_size, d.num_hidden_layers, d.num_attention_heads = _lib.AHA_ARCH_QWEN3VL, 512, 1024, 2, 4
        d.num_key_value_heads, d.head_dim, d.vocab_size, d.compute_dtype = 2, 128, 2048, _lib.AHA_BF16
        d.vis_spatial_merge_size, d.vis_patch_size, d.vis_num_heads, d.vis_hidden_size = 2, 16, 2, 144
        d.aud_d_model = 128
        for k, v in kw.items():
            setattr(d, k, v)
        tv = _lib.TensorView(name=name, data=None, dtype=_lib.AHA_BF16, ndim=1)
        rc = hip_lib.aha_hip_model_create(C.addressof(ctx), C.byref(d), C.byref(tv), 1, C.byref(out))
        return rc, hip_lib.aha_hip_last_error()

    for kw in (dict(vis_hidden_size=148, vis_num_heads=2), dict(vis_hidden_size=72 * 29, vis_num_heads=29),   # 2088 * 4 = 8352 > 8192
               dict(vis_hidden_size=72 * 120, vis_num_heads=120)):
        rc, msg = create(**kw)
        assert rc == -6 and b"LayerNorm" in msg and b"vision" in msg, (kw, rc, msg)
    for kw in (dict(aud_d_model=132), dict(aud_d_model=64 * 129)):
        rc, msg = create(arch=_lib.AHA_ARCH_QWEN3ASR, **kw)
        assert rc == -6 and b"LayerNorm" in msg and b"audio" in msg, (kw, rc, msg)


def test_generalised_page_mirror_reproduces_kv_pages_at_128():
    for kvh in (1, 2, 8):
        assert torch.equal(kv_pages.slot_index_of(kvh, 128, 128), kv_pages.slot_index(kvh))
        assert kv_pages.page_elems_of(kvh, 128, 128) == kv_pages.page_elems(kvh)
    for nh, dqk, dv in ((2, 96, 80), (5, 96, 80), (2, 64, 64), (14, 64, 64)):
        el = kv_pages.slot_index_of(nh, dqk, dv)
        n = kv_pages.page_elems_of(nh, dqk, dv)
        assert el.shape == (64, nh * (dqk + dv)) and sorted(el.reshape(-1).tolist()) == list(range(n))   # a bijection onto the page
        assert int(el[:, : nh * dqk].max()) < nh * 64 * dqk <= int(el[:, nh * dqk:].min())               # the K block first
        # a 16-byte piece holds 8 consecutive dims of one token in K, and one dim of 8 tokens in V
        assert torch.equal(el[:, 8:16], el[:, 8:9] + torch.arange(8))
        v0 = el[:, nh * dqk].sort().values.reshape(8, 8)
        assert torch.equal(v0, v0[:, :1] + torch.arange(8)) and bool((v0[:, 0] % 8 == 0).all())


def _vision(G, D, table=None):
    cfg = SimpleNamespace(vision=SimpleNamespace(num_position_embeddings=G * G, head_dim=72, spatial_merge_size=2, hidden_size=D, num_heads=D // 72))
    w = {"model.visual.pos_embed.weight": (T.rnd((G * G, D), 5, 0.5) if table is None else table).float()}
    return ov.OracleVision(cfg, w, NM)


def test_layernorm_reference_against_the_oracle():
    """oracle.qwen3vl.layer_norm is the same definition in f32: a bf16 rounding flips about once in 2^14 elements, by one ulp."""
    for dim, eps, kind in ((144, 1e-6, "offset"), (1152, 1e-6, "small"), (4608, 1e-6, "offset"), (896, 1e-5, "small")):
        x, w, b = T.layernorm_inputs(dim, kind, 11)
        assert_close_ulps(T.layernorm_ref(x, w, b, eps), ov.layer_norm(NM, x.float(), w.float(), b.float(), eps), 1, 0.999, f"dim {dim} {kind}")


def test_vit_tables_and_pos_embed_against_the_oracle():
    for G, D in ((48, 144), (8, 144)):
        o = _vision(G, D)
        table = T.bf(o.w["model.visual.pos_embed.weight"])
        for grids in T.POS_GRIDS:
            t = T.vit_tables(grids, G)
            idx, wt = o.pos_embed_indices(np.asarray(grids))
            assert np.array_equal(idx, t["idx"]) and np.array_equal(wt.view(np.uint32), t["wt"].view(np.uint32)), (G, grids)
            x = T.rnd((t["N"], D), 6)
            assert T.same_bits(T.pos_embed_ref(x, table, t["idx"], t["wt"]), T.bf(NM.r(x.float() + o.pos_embed(np.asarray(grids))))), (G, grids)
            fr, rows, cols = o.rot_pos(np.asarray(grids))
            assert np.array_equal(rows, t["rowcol"][:, 0]) and np.array_equal(cols, t["rowcol"][:, 1])
            assert torch.equal(fr, T.vit_rope_angles(t["rowcol"], o.inv_freq.float()))
    # the identity: a grid of the table's own side reads every table row with weight exactly 1
    t = T.vit_tables([(1, 48, 48)], 48)
    assert set(np.unique(t["wt"]).tolist()) == {0.0, 1.0} and np.array_equal(np.sort(t["idx"][0]), np.arange(48 * 48))
    assert torch.allclose(T.vit_inv_freq(), _vision(8, 144).inv_freq.float(), rtol=2e-7, atol=0)


def test_vit_rotation_against_the_oracle_helpers():
    """The rotation of OracleVision.attention (apply_rotary_pos_emb_vision: r(r(u * cos) + r(rotate_half(u) * sin)) with oracle.qwen3's
    rotate_half and the oracle's rounding), on the table of torch's f32 cos / sin as the oracle computes it."""
    t = T.vit_tables([(1, 6, 10), (2, 4, 4)], 8)
    inv = T.vit_inv_freq()
    ang = T.vit_rope_angles(t["rowcol"], inv)
    emb = torch.cat([ang, ang], -1)
    c, s = NM.r(emb.cos())[:, None], NM.r(emb.sin())[:, None]
    u = T.rnd((t["N"], 5, 72), 8)
    want = NM.r(NM.r(u.float() * c) + NM.r(oq.rotate_half(u.float()) * s))
    assert T.same_bits(T.vit_rope_apply(u, T.vit_rope_table_ref(t["rowcol"], inv, f32_trig=True)), T.bf(want))


def test_im2col_references_against_the_oracle_conv():
    """im2col + f64 matmul against OracleAudioEncoder._conv (an f64 conv2d, bias, tanh-GELU): the same sums in another order."""
    H = 32
    w1, b1, w2, b2 = T.rnd((H, 1, 3, 3), 20, 0.3), T.rnd((H,), 21, 0.1), T.rnd((H, H, 3, 3), 22, 0.06), T.rnd((H,), 23, 0.1)
    enc = oa.OracleAudioEncoder(SimpleNamespace(), {"a.conv2d1.weight": w1, "a.conv2d1.bias": b1, "a.conv2d2.weight": w2, "a.conv2d2.bias": b2}, NM, "a.")
    clips = [(0, 100), (100, 130), (230, 7)]
    feat = torch.randn(128, 240, generator=torch.Generator().manual_seed(24))
    chunks = T.audio_chunks(clips)
    wins = torch.stack([torch.cat([T.bf(feat[:, c0 + i * 100:c0 + min(F, (i + 1) * 100)]).float(), torch.zeros(128, max(0, (i + 1) * 100 - F))], 1)
                        for c0, F, i in chunks])[:, None]                                    # (C, 1, 128, 100), each window padded on its own
    act = lambda cols, w, b: NM.r(ov.gelu_tanh(NM.r(NM.r((cols.double() @ w.double().t()).float()) + b.float())))
    y1 = enc._conv(wins, "conv2d1")                                                          # (C, H, 64, 50)
    got1 = act(T.audio_im2col1_ref(feat, clips)[:, :9], w1.reshape(H, 9), b1)
    assert_close_ulps(got1, y1.permute(0, 2, 3, 1).reshape(-1, H), 1, 0.999, "conv1 through im2col1")
    x2 = T.bf(y1.permute(0, 2, 3, 1))[:2].contiguous()                                       # NHWC (2, 64, 50, H)
    y2 = enc._conv(x2.float().permute(0, 3, 1, 2), "conv2d2")
    got2 = act(T.im2col_nhwc_ref(x2), w2.permute(0, 2, 3, 1).reshape(H, 9 * H), b2)          # weight columns (kh, kw, cin)
    assert_close_ulps(got2, y2.permute(0, 2, 3, 1).reshape(-1, H), 1, 0.999, "conv2 through im2col_nhwc")


def test_layernorm_cap_holds_for_an_f32_layernorm():
    """The GPU tests want <= 1 ulp and >= 0.995 bit-identical.  torch's f32 two-pass LayerNorm alone, on every (dim, eps, input kind) of the
    GPU test and on GEMM-output-like rows of its widths: never more than 1 ulp; smallest bit-identical share measured 0.99953 on the mean-8
    and std-0.05 rows and the GEMM-like rows (10 x closer to 1 than the cap), 0.99794 on the mean-64 rows (the f32 mean itself is 2^-18 of
    a standard deviation off there; still twice as close as the cap).
    A one-pass E[x^2] - mean^2 variance in f32 stays at 0.9988 on the mean-8 rows -- they do not tell it from the two-pass form at this cap --
    and drops to 0.96 on the mean-64 rows, which is why the GPU test has them."""
    worst = {}
    cases = [(d, e, k, T.layernorm_inputs(d, k, 100 + d)) for d in T.LN_DIMS for e in T.LN_EPS for k in T.LN_KINDS]
    cases += [(n, 1e-6, "gemm", (T.rnd((130, n), 7 + n), T.rnd((n,), 8, 0.1, 1.0), T.rnd((n,), 9, 0.5))) for n in T.GEMM_LN_N]
    for dim, eps, kind, (x, w, b) in cases:
        ref, f32 = T.layernorm_ref(x, w, b, eps), T.layernorm_f32(x, w, b, eps)
        assert_close_ulps(f32, ref, T.LN_ULPS, 0.9965 if kind == "far" else 0.999, f"f32 LayerNorm dim {dim} eps {eps} {kind}")
        worst[kind == "far"] = min(worst.get(kind == "far", 1.0), float((f32.float() == ref.float()).float().mean()))
    print(f"MEASURED f32 LayerNorm smallest bit-identical share {worst[False]:.5f}, on the mean-64 rows {worst[True]:.5f}")
    for kind, lo, hi in (("offset", 0.0, 1.01), ("far", 0.0, 0.98)):   # (the mean-8 figure is printed, not asserted)
        x, w, b = T.layernorm_inputs(1152, kind, 100 + 1152)
        x32 = x.float()
        mu = x32.mean(-1, keepdim=True)
        one_pass = T.bf((x32 - mu) / torch.sqrt((x32 * x32).mean(-1, keepdim=True) - mu * mu + 1e-6) * w.float() + b.float())
        share = float((one_pass.float() == T.layernorm_ref(x, w, b, 1e-6).float()).float().mean())
        print(f"MEASURED one-pass f32 variance on the {kind} rows: {share:.5f} bit-identical")
        assert lo <= share < hi, (kind, share)


def test_rope_table_cap_holds_for_an_f32_cos_sin():
    """The GPU test wants every table entry within one bf16 value of the f64 one and >= 0.99 bit-identical.  torch's f32 cos / sin of the same
    f32 angles: bit-identical on EVERY entry of every grid of the GPU test (positions below 100; share 1.00000 measured), and on all
    positions below 384."""
    inv = T.vit_inv_freq()
    for grids in T.ROPE_GRIDS + [[(1, 384, 2)]]:
        rc = T.vit_tables(grids, 8)["rowcol"]
        a, b = T.vit_rope_table_ref(rc, inv), T.vit_rope_table_ref(rc, inv, f32_trig=True)
        assert torch.equal(a, b), grids


def test_sinus_table_cap_holds_for_the_oracle_table():
    """The GPU test wants the kernel's table within one bf16 value of the f64 one and >= 0.99 bit-identical.  OracleAudioEncoder.pos_embed with
    the reference switch (torch f32 sin / cos of f32 angles from an f32 powf) alone: never more than one value away, bit-identical share
    measured 1.00000 at d 128 and at d 896 (positions below 13)."""
    enc = oa.OracleAudioEncoder(SimpleNamespace(), {}, NM, "a.", oa.AsrSwitches(pe_reference=True))
    for d, Tn, _ in T.SINUS_CASES:
        ref, got = T.sinus_table_ref(Tn, d), T.bf(enc.pos_embed(Tn, d))
        dist = (T.bf16_ordinal(ref) - T.bf16_ordinal(got)).abs()
        share = float((dist == 0).float().mean())
        print(f"MEASURED oracle sinusoidal table d {d}: worst {int(dist.max())} exact {share:.5f}")
        assert int(dist.max()) <= 1 and share >= 0.999, (d, int(dist.max()), share)
