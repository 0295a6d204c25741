"""-m gpu: the row-wise kernels of the Qwen3-VL vision tower and the Qwen3-ASR audio tower, one by one, against host references of the same
operations (tests/tower_rows_ref.py).  The whole-tower tests (test_vl_gpu.py, test_asr_gpu.py, the multimodal batch tests) bound these kernels
only through embeddings of tiny towers at 0.08 / 0.02 standard deviations; here each one is held to its own definition.

The kernels (aha_amd/csrc/kernels_vit.hip, kernels_audio.hip, kernels_gemm.hip) are reached through the op-level test entries of
tests/tools/README.md, which launch the production launchers unchanged: layernorm_rows_kernel<1 / 3 / 9 / 16>; the LayerNorm riding on a GEMM
call (gemm_splitk_reduce_layernorm_kernel, or the appended launch); pos_embed_add_kernel with the tower's host corner tables
(vision_host_tables, the function the tower itself calls); vit_rope_table_kernel + vit_rope_pack_kernel; scatter_rows_kernel;
audio_im2col1_kernel, im2col_nhwc_kernel, audio_tokens_gather_kernel, sinus_pe_add_kernel, kv_pack_generic_kernel.

Every output buffer, every page pool and a guard page on either side of it start as the bf16 pattern 0x7FA5 (a NaN with a payload), and the
page pointers are handed over in a seeded scrambled order, so "not written" and "written where it must not be" both show.  Everything but the
two trigonometric tables and the LayerNorm is compared bit for bit: every rounding point of those operations is defined.

Caps on bit-identical shares (LayerNorm 0.995, the tables 0.99) are conditions, not measurements: tests/test_tower_rows_cpu.py shows that a
torch f32 restatement alone stays well above them on the same inputs.

Measured on an MI355X (the tests print "MEASURED ..." lines with -s): both trigonometric tables bit-identical to the reference on every
entry; the whole file runs in under 4 s.

Mutations of kernels_vit.hip, one at a time on a scratch copy, each wrong in values only, and what caught them on the device:
  - rowcol[2n + 1] for the first quarter in vit_rope_table_kernel: test_vit_rope_stage (all 3); the whole-tower tests stayed green;
  - one rbf dropped from pos_embed_add_kernel's sum: test_vit_pos_embed (all 3); the whole-tower tests stayed green;
  - the LayerNorm variance as E[x^2] - mean^2: test_layernorm_rows (all 10: 0.958 - 0.986 bit-identical on the mean-64 rows; the mean-8
    rows stay above the cap) and test_gemm_with_riding_layernorm (the three folded widths); of the whole-tower tests only a pinned digest;
  - 0 instead of 1.0 in V pad dim 72: test_vit_rope_stage (all 3), and the whole-tower tests widely (the row sum is gone).
"""
import functools
import os
import sys

import numpy as np
import pytest
import torch

from oracle.numerics import Numerics

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kv_pages  # noqa: E402
import tower_rows_ref as T  # noqa: E402
from test_ops_gpu import assert_close_ulps  # noqa: E402

pytestmark = pytest.mark.gpu
NM = Numerics("bf16", matmul_f64=True)


def bits(x):
    return x.contiguous().view(torch.int16)


def assert_same_bits(got, ref, what):
    g, r = bits(got.cpu()), bits(ref)
    assert g.shape == r.shape, f"{what}: shape {tuple(g.shape)} vs {tuple(r.shape)}"
    n = int((g != r).sum())
    assert n == 0, f"{what}: {n}/{g.numel()} elements differ from the reference bit for bit"


# ---- LayerNorm ---------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def ln_case(dim, kind, eps):
    x, w, b = T.layernorm_inputs(dim, kind, 100 + dim)
    return x, w, b, T.layernorm_ref(x, w, b, eps)


@pytest.mark.parametrize("dim", T.LN_DIMS)
def test_layernorm_rows(gpu, dim):
    """Every VPL instantiation at its first and last width, 1 / 4 / 5 / 37 rows (four rows per block), both epsilons, on rows of mean 8, of
    std 0.05 and of mean 64: within 1 bf16 ulp of the f64 LayerNorm with >= 0.995 bit-identical; the rows past `rows` keep the fill; a
    launch of fewer rows gives the bits of the 37-row launch's first rows.

    The mean-64 rows take the share cap at the 37-row launch only.  Any f32 LayerNorm holds the row mean (about 64) to 2^-18, one value per
    row, and that shifts a whole row's outputs: torch's f32 form alone leaves 0.998 of 37 such rows on the reference's bf16 value
    (tests/test_tower_rows_cpu.py) but single rows of 144 elements down to 0.986 and the first four rows at dim 144, eps 1e-5 at 0.9948
    (computed on the CPU, no kernel involved), and 0.995 of 144 or 576 elements is zero or two elements.
    The launches of 1, 4 and 5 of these rows are held to the 1-ulp bound and, bit for bit, to the 37-row launch instead."""
    from aha_amd import ops
    for kind in T.LN_KINDS:
        for eps in T.LN_EPS:
            x, w, b, ref = ln_case(dim, kind, eps)
            xd, wd, bd = x.to(gpu), w.to(gpu), b.to(gpu)
            full = None
            for rows in reversed(T.LN_ROWS):
                out = T.filled((x.shape[0] + 3, dim)).to(gpu)
                ops.debug_layernorm_rows(xd, wd, bd, eps, out=out, rows=rows)
                got = out.cpu()
                what = f"dim {dim} rows {rows} eps {eps} {kind}"
                if full is None:
                    full = got
                    print(f"MEASURED layernorm {what}: exact {float((got[:rows].float() == ref[:rows].float()).float().mean()):.5f}")
                assert_close_ulps(got[:rows], ref[:rows], T.LN_ULPS, T.LN_EXACT if kind != "far" or got is full else None, what)
                assert_same_bits(got[:rows], full[:rows], what + ": against the 37-row launch")
                assert bool(T.is_fill(got[rows:]).all()), f"{what}: rows past `rows` were written"


# ---- GEMM with the LayerNorm riding on it --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("plan", [(0, 0), (256, 2)])
@pytest.mark.parametrize("N", T.GEMM_LN_N)
def test_gemm_with_riding_layernorm(gpu, N, plan):
    """C within test_ops_gpu.py::test_gemm_bias_act_residual's bound (2 ulps, 0.97) of the f64 chain; norm_out bit-identical to the
    stand-alone LayerNorm of the C the call produced (the claim of kernels_gemm.hip's comments) and within the LayerNorm bound of the f64
    LayerNorm of that C.  (256, 2) ends in the reduce pass, which folds the norm in for N = 520 .. 1536; 144 and 1544 get the appended
    launch.  The residual is C itself, as in the ViT block.  (This test found the folded norm 2 of 18720 elements off the stand-alone
    launch at N = 144 -- values on a bf16 tie, the compiler contracting the two kernels' multiply-adds differently -- whereupon the fold
    was restricted to the widths whose stand-alone kernel it matches.)"""
    from aha_amd import ops
    eps = 1e-6
    nw, nb = T.rnd((N,), 31, 0.1, 1.0), T.rnd((N,), 32, 0.5)
    ops.gemm_plan(*plan)
    try:
        for M in T.GEMM_LN_M:
            for K in T.GEMM_LN_K:
                A, W, b, res = T.rnd((M, K), 33 + M), T.rnd((N, K), 34 + K, 0.02), T.rnd((N,), 35, 0.5), T.rnd((M, N), 36)
                y = NM.linear(A.float(), W.float())
                yb = NM.r(y + b.float())
                for epi, ref in (("bias+residual", NM.r(res.float() + yb)), ("bias", yb), ("none", y)):
                    what = f"M {M} N {N} K {K} plan {plan} {epi}"
                    c_buf = res.clone().to(gpu) if epi == "bias+residual" else T.filled((M, N)).to(gpu)
                    n_buf = T.filled((M, N)).to(gpu)
                    C, Y = ops.debug_gemm_layernorm(A.to(gpu), W.to(gpu), nw.to(gpu), nb.to(gpu), eps, None if epi == "none" else b.to(gpu),
                                                    c_buf if epi == "bias+residual" else None, out=c_buf, norm_out=n_buf)
                    alone = ops.debug_layernorm_rows(C, nw.to(gpu), nb.to(gpu), eps)
                    C, Y, alone = C.cpu(), Y.cpu(), alone.cpu()
                    assert_close_ulps(C, ref, 2, 0.97, what + ": C")
                    assert_same_bits(Y, alone, what + ": norm_out against the stand-alone LayerNorm of C")
                    assert_close_ulps(Y, T.layernorm_ref(C, nw, nb, eps), T.LN_ULPS, T.LN_EXACT, what + ": norm_out")
    finally:
        ops.gemm_plan(0, 0)


# ---- ViT position embedding ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("G,D", T.POS_CONFIGS)
def test_vit_pos_embed(gpu, G, D):
    """The host corner indices and weights equal the reference's exactly (the weights as f32 bits) and x after the call is bit-identical, for
    grids below, at (the identity: every weight 1 or 0) and above the table's side, on one axis or both, and three grids in one call."""
    from aha_amd import ops
    table = T.rnd((G * G, D), 40 + G, 0.5)
    td = table.to(gpu)
    for grids in T.POS_GRIDS:
        t = T.vit_tables(grids, G)
        x = T.rnd((t["N"], D), 41)
        xd = x.to(gpu)
        idx, wt = ops.debug_vit_pos_embed(xd, td, grids, G)
        what = f"G {G} D {D} grids {grids}"
        assert np.array_equal(idx, t["idx"]), what + ": corner indices"
        assert np.array_equal(wt.view(np.uint32), t["wt"].view(np.uint32)), what + ": corner weights (f32 bits)"
        if grids == [(1, G, G)]:
            assert set(np.unique(wt).tolist()) == {0.0, 1.0}, what + ": the identity grid has a weight other than 0 or 1"
        assert_same_bits(xd, T.pos_embed_ref(x, table, t["idx"], t["wt"]), what + ": x")


# ---- ViT rope stage --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nh", T.ROPE_NH)
def test_vit_rope_stage(gpu, nh):
    """The table within one bf16 value of the f64 cos / sin of the f32 angle, >= 0.99 bit-identical, rows < 18 following the patch row (grids
    with h != w); then, given that table, q_out and the whole pool -- K and V pages, pad elements, tail slots, guard pages -- bit-identical to
    the reference image.  nh 5 runs the tail of the four-heads-in-flight loop, 16 four full trips."""
    from aha_amd import ops
    inv = T.vit_inv_freq()
    for gi, grids in enumerate(T.ROPE_GRIDS):
        t = T.vit_tables(grids, 8)
        N, n_pages = t["N"], len(t["pages"])
        what = f"nh {nh} grids {grids}"
        qkv = T.rnd((N, 3 * nh * T.VIT_HD), 50 + gi)
        pool = T.Pool(n_pages + 1, kv_pages.page_elems_of(nh, T.VIT_DQK, T.VIT_DV), 60 + gi)   # (a spare page the call must not touch)
        ptrs = pool.upload()
        q_out = T.filled((N, nh, T.VIT_DQK)).to(gpu)
        tab, rowcol, page_of, slot_of = ops.debug_vit_rope(qkv.to(gpu), grids, inv.to(gpu), ptrs[:n_pages].contiguous(), nh, q_out)
        tab = tab.cpu()
        for name, got in (("rowcol", rowcol), ("page_of", page_of), ("slot_of", slot_of)):
            assert np.array_equal(got, t[name]), f"{what}: host table {name}"
        ref_tab = T.vit_rope_table_ref(t["rowcol"], inv)
        assert torch.equal(T.bf(tab).float(), tab), what + ": a table entry is not a bf16 value"
        dist = (T.bf16_ordinal(T.bf(tab)) - T.bf16_ordinal(T.bf(ref_tab))).abs()
        share = float((dist == 0).float().mean())
        print(f"MEASURED vit rope table {what}: worst {int(dist.max())} exact {share:.5f}")
        assert int(dist.max()) <= 1, f"{what}: {int((dist > 1).sum())} table entries more than one bf16 value from the reference"
        assert share >= T.TAB_EXACT, f"{what}: only {share:.5f} of the table bit-identical to the reference"
        q_ref, image = T.vit_pages_ref(pool, qkv, tab, t, nh)
        assert_same_bits(q_out, q_ref, what + ": q_out")
        got = pool.dev.cpu()
        assert bool(T.is_fill(got[0]).all() and T.is_fill(got[-1]).all()), what + ": a guard page was written"
        assert bool(T.is_fill(got[pool.phys(n_pages)]).all()), what + ": a page past the call's pages was written"
        assert_same_bits(got, image, what + ": the pool (K / V pages, pads, tail slots, everything else untouched)")
        del pool.dev, pool.ptrs


# ---- scatter rows ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [256, 4096])
@pytest.mark.parametrize("add", [False, True])
def test_scatter_rows(gpu, D, add):
    from aha_amd import ops
    rows = [13, 2, 19, 0, 7, 8, 11]
    src = T.rnd((7, D), 70)
    dst = T.rnd((20, D), 71) if add else T.filled((20, D))
    ref = dst.clone()
    ref[rows] = T.bf(dst[rows].float() + src.float()) if add else src
    dd = dst.to(gpu)
    ops.debug_scatter_rows(dd, src.to(gpu), rows, add)
    assert_same_bits(dd, ref, f"scatter D {D} add {add}")


# ---- audio staging -------------------------------------------------------------------------------------------------------------------------------------
def test_audio_im2col1(gpu):
    """Clips of 100, 130, 7 and 250 frames back to back in a dense random feature buffer: each clip's last window is zero-padded although
    the next clip's frames lie right behind it; the border taps and columns 9..15 are zero."""
    from aha_amd import ops
    lens = [100, 130, 7, 250]
    clips = [(sum(lens[:i]), F) for i, F in enumerate(lens)]
    feat = torch.randn(128, sum(lens) + 13, generator=torch.Generator().manual_seed(80))
    chunks = T.audio_chunks(clips)
    ref = T.audio_im2col1_ref(feat, clips)
    assert ref.shape == (len(chunks) * 64 * 50, 16) and len(chunks) == 7
    out = ops.debug_audio_im2col1(feat.to(gpu), chunks, T.filled(tuple(ref.shape)).to(gpu)).cpu()
    assert not bits(out[:, 9:]).any(), "columns 9..15 are not zero"
    r = out.reshape(7, 64, 50, 16)
    assert not bits(r[:, 0, :, 0:3]).any() and not bits(r[:, :, 0, 0:9:3]).any(), "the top / left border taps are not zero"
    assert not bits(r[3, :, 4:, :]).any(), "the 7-frame clip's window is not zero past its frames"   # taps of output column 4 read frames 7..9
    assert_same_bits(out, ref, "im2col1")


@pytest.mark.parametrize("shape", [(3, 64, 50, 32), (2, 32, 25, 480), (1, 32, 25, 520)])
def test_im2col_nhwc(gpu, shape):
    from aha_amd import ops
    x = T.rnd(shape, 81)
    ref = T.im2col_nhwc_ref(x)
    out = ops.debug_im2col_nhwc(x.to(gpu), T.filled(tuple(ref.shape)).to(gpu))
    assert_same_bits(out, ref, f"im2col_nhwc {shape}")


@pytest.mark.parametrize("B,Fq,Tn,Cc", [(3, 16, 13, 32), (2, 16, 13, 480)])
def test_audio_tokens_gather(gpu, B, Fq, Tn, Cc):
    from aha_amd import ops
    nchw = T.rnd((B, Cc, Fq, Tn), 82)                                         # the conv stack's output as the reference model holds it
    ref = nchw.permute(0, 3, 1, 2).reshape(B * Tn, Cc * Fq)
    out = ops.debug_audio_tokens_gather(nchw.permute(0, 2, 3, 1).contiguous().to(gpu), T.filled((B * Tn, Cc * Fq)).to(gpu))
    assert_same_bits(out, ref.contiguous(), f"tokens_gather {(B, Fq, Tn, Cc)}")


@pytest.mark.parametrize("d,Tn,rows", T.SINUS_CASES)
def test_sinus_pe_add(gpu, d, Tn, rows):
    """On a zero x the call yields the kernel's own bf16 table (position r % T): within one bf16 value of the f64 table, >= 0.99 bit-identical;
    on a random x the result is bf16(x + that table) bit for bit.  Rows past `rows` keep the fill."""
    from aha_amd import ops
    z = T.filled((rows + 2, d))
    z[:rows] = 0
    tab = ops.debug_sinus_pe_add(z.to(gpu), Tn, rows).cpu()
    assert bool(T.is_fill(tab[rows:]).all()), "rows past `rows` were written"
    tab = tab[:rows]
    ref = T.sinus_table_ref(Tn, d)[torch.arange(rows) % Tn]
    dist = (T.bf16_ordinal(tab) - T.bf16_ordinal(ref)).abs()
    share = float((dist == 0).float().mean())
    print(f"MEASURED sinusoidal table d {d}: worst {int(dist.max())} exact {share:.5f}")
    assert int(dist.max()) <= 1 and share >= T.TAB_EXACT, f"d {d}: worst {int(dist.max())} bf16 values, {share:.5f} bit-identical"
    assert_same_bits(tab[Tn:2 * Tn], tab[:Tn], "the table of rows T .. 2T - 1 against rows 0 .. T - 1")
    x = T.rnd((rows, d), 83)
    got = ops.debug_sinus_pe_add(x.to(gpu), Tn)
    assert_same_bits(got, T.bf(x.float() + tab.float()), f"sinus_pe_add d {d}")


@pytest.mark.parametrize("nh,hd", [(2, 64), (14, 64), (2, 128)])
def test_kv_pack_generic(gpu, nh, hd):
    """77 rows in slot order (two pages, the second partly filled), and three clips that each start a page (slot_of); the K / V heads sit at
    columns nh * hd and 2 nh * hd of a fused q | k | v row.  The whole pool -- unwritten slots, a spare page, guard pages -- against the image."""
    from aha_amd import ops
    ld = 3 * nh * hd
    lens = (30, 70, 13)
    slot_of = [p0 * 64 + i for p0, n in zip((0, 1, 3), lens) for i in range(n)]
    for N, slots, n_pages in ((77, None, 2), (sum(lens), slot_of, 4)):
        src = T.rnd((N, ld), 90 + N)
        pool = T.Pool(n_pages + 1, kv_pages.page_elems_of(nh, hd, hd), 91 + N)
        ptrs = pool.upload()
        ops.debug_kv_pack_generic(src.to(gpu), nh * hd, 2 * nh * hd, ptrs[:n_pages].contiguous(), nh, hd, slots)
        got = pool.dev.cpu()
        what = f"kv_pack nh {nh} hd {hd} N {N} slot_of {slots is not None}"
        assert bool(T.is_fill(got[0]).all() and T.is_fill(got[-1]).all() and T.is_fill(got[pool.phys(n_pages)]).all()), what + ": a guard or spare page was written"
        assert_same_bits(got, T.kv_pack_ref(pool, src, nh * hd, 2 * nh * hd, nh, hd, slots), what)
        del pool.dev, pool.ptrs
