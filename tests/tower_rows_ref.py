"""Host references of the vision and audio towers' row kernels, for tests/test_tower_rows_gpu.py and tests/test_tower_rows_cpu.py.

Plain torch / numpy, written from each operation's definition (the reference model's op sequence, one rounding to bf16 per tensor op) and,
for the pages, from the layout's description (tests/kv_pages.py, "KV page layout" in aha_amd/csrc/common.h) -- not from the kernels' index
expressions.  Everything here runs on the CPU.
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kv_pages  # noqa: E402
from prefill_rope_ref import bf16_ordinal, same_bits  # noqa: E402,F401

PAGE_TOKENS = 64
FILL = 0x7FA5   # the bf16 bit pattern of the fill (a NaN with a payload): "never written" shows, and so does "written where it must not be"
VIT_HD, VIT_DQK, VIT_DV = 72, 96, 80


# ---- the cases of tests/test_tower_rows_gpu.py (the CPU tier checks its caps on the same inputs) ---------------------------------------------
LN_DIMS = (144, 512, 520, 896, 1152, 1536, 1544, 4608, 4616, 8192)   # first and last width of VPL 1 / 3 / 9 / 16, and the real 896, 1152, 4608
LN_ROWS = (1, 4, 5, 37)                                              # four rows per block
LN_EPS = (1e-6, 1e-5)
LN_KINDS = ("offset", "small", "far")
LN_ULPS, LN_EXACT = 1, 0.995
# N: 144 and 1544 are outside the widths the reduce pass folds the norm in for (520 .. 1536: the norm is an appended launch); 520, 1152, 1536 inside
GEMM_LN_M, GEMM_LN_N, GEMM_LN_K = (5, 130), (144, 520, 1152, 1536, 1544), (320, 1152)
# (table side G, D): the real table; the tiny towers'; a D above 2048 (a second trip of the 256-thread loop)
POS_CONFIGS = ((48, 1152), (8, 144), (8, 2056))
POS_GRIDS = [[(1, 2, 2)], [(1, 4, 6)], [(2, 6, 4)], [(1, 48, 48)], [(1, 50, 46)], [(1, 2, 98)], [(1, 14, 14)], [(1, 4, 6), (2, 6, 4), (1, 8, 8)]]
# segment lengths 60, 64 and 196; two frames of 120 rows, each starting a page; several grids in one call
ROPE_GRIDS = [[(1, 6, 10)], [(1, 4, 16)], [(1, 14, 14)], [(2, 10, 12)], [(1, 6, 10), (2, 10, 12), (1, 2, 98)]]
ROPE_NH = (2, 5, 16)
TAB_EXACT = 0.99
SINUS_CASES = ((128, 13, 39), (896, 13, 39))   # (d, T, rows)


def bf(x):
    return x.to(torch.bfloat16)


def rnd(shape, seed, std=1.0, mean=0.0):
    g = torch.Generator().manual_seed(seed)
    return bf(torch.randn(shape, generator=g) * std + mean)


def filled(shape, dtype=torch.bfloat16):
    """A buffer of the fill pattern (bf16), or of its f32 / int32 counterpart 0x7FA57FA5."""
    if dtype == torch.bfloat16:
        return torch.full(shape, FILL, dtype=torch.int16).view(torch.bfloat16)
    return torch.full(shape, 0x7FA57FA5, dtype=torch.int32).view(dtype)


def is_fill(x):
    return x.contiguous().view(torch.int16) == FILL


# ---- LayerNorm -------------------------------------------------------------------------------------------------------------------------------
def layernorm_ref(x, w, b, eps):
    """LayerNorm over the last dim in f64 on the bf16 inputs, rounded once to bf16."""
    x64, eps64 = x.double(), float(np.float32(eps))
    mu = x64.mean(-1, keepdim=True)
    var = ((x64 - mu) ** 2).mean(-1, keepdim=True)
    return bf(((x64 - mu) / torch.sqrt(var + eps64) * w.double() + b.double()).float())


def layernorm_f32(x, w, b, eps):
    """The same in torch f32 (two-pass variance): the restatement the CPU tier holds the GPU tests' caps against."""
    x32 = x.float()
    mu = x32.mean(-1, keepdim=True)
    var = ((x32 - mu) ** 2).mean(-1, keepdim=True)
    return bf((x32 - mu) / torch.sqrt(var + eps) * w.float() + b.float())


def layernorm_inputs(dim, kind, seed, rows=37):
    """kind "offset": rows of mean 8, std 1; "small": rows of std 0.05; "far": rows of mean 64, std 1 -- a one-pass E[x^2] - mean^2
    variance in f32 cancels 12 bits there and leaves only ~0.96 of the outputs on the reference's bf16 value (on the mean-8 rows it still
    reaches 0.999: tests/test_tower_rows_cpu.py measures both).  w around 1, b random."""
    x = rnd((rows, dim), seed, 0.05) if kind == "small" else rnd((rows, dim), seed, 1.0, 8.0 if kind == "offset" else 64.0)
    return x, rnd((dim,), seed + 1, 0.1, 1.0), rnd((dim,), seed + 2, 0.5)


# ---- ViT: host tables ------------------------------------------------------------------------------------------------------------------------
def linspace_f32(end, steps):
    """linspace(0, end, steps) as the reference model builds it, in f32: step = end / (steps - 1), value i = i * step."""
    if steps == 1:
        return np.zeros(1, np.float32)
    step = np.float32(end) / np.float32(steps - 1)
    return (np.arange(steps, dtype=np.float32) * step).astype(np.float32)


def merge_order(h, w, merge):
    """(h * w, 2) patch (row, col) of one frame in merge-window order: windows row-major, the merge x merge patches of a window row-major."""
    out = []
    for bh in range(h // merge):
        for bw in range(w // merge):
            for ih in range(merge):
                for iw in range(merge):
                    out.append((bh * merge + ih, bw * merge + iw))
    return np.asarray(out, dtype=np.int64).reshape(-1, 2)


def vit_tables(grids, G, merge=2):
    """Per patch row, frames of a grid back to back and grids back to back: idx (4, N) int32 corner rows of the (G * G) table and wt (4, N) f32
    bilinear weights (floor = truncation of the f32 coordinate, ceil = floor + 1 clamped to G - 1), rowcol (N, 2), and the attention
    layout: every frame a segment on pages of its own -> page_of (N), slot_of (N), and per page (first row, rows)."""
    idx, wt, rowcol, page_of, slot_of, pages = [], [], [], [], [], []
    one = np.float32(1.0)
    row0 = 0
    for t, h, w in grids:
        rc = merge_order(h, w, merge)
        y, x = rc[:, 0], rc[:, 1]
        hv, wv = linspace_f32(G - 1, h), linspace_f32(G - 1, w)
        hf, wf = hv.astype(np.uint32).astype(np.int64), wv.astype(np.uint32).astype(np.int64)
        hc, wc = np.minimum(hf + 1, G - 1), np.minimum(wf + 1, G - 1)
        dh, dw = (hv - hf.astype(np.float32))[y], (wv - wf.astype(np.float32))[x]
        assert dh.dtype == np.float32 and dw.dtype == np.float32
        i4 = np.stack([hf[y] * G + wf[x], hf[y] * G + wc[x], hc[y] * G + wf[x], hc[y] * G + wc[x]])
        w4 = np.stack([(one - dh) * (one - dw), (one - dh) * dw, dh * (one - dw), dh * dw]).astype(np.float32)
        for _ in range(t):
            idx.append(i4), wt.append(w4), rowcol.append(rc)
            local = np.arange(h * w)
            page_of.append(len(pages) + local // PAGE_TOKENS)
            slot_of.append(local % PAGE_TOKENS)
            for p in range(0, h * w, PAGE_TOKENS):
                pages.append((row0 + p, min(PAGE_TOKENS, h * w - p)))
            row0 += h * w
    return dict(idx=np.concatenate(idx, 1).astype(np.int32), wt=np.concatenate(wt, 1), rowcol=np.concatenate(rowcol).astype(np.int32),
                page_of=np.concatenate(page_of).astype(np.int32), slot_of=np.concatenate(slot_of).astype(np.int32), pages=pages, N=row0)


def pos_embed_ref(x, table, idx, wt):
    """x + bilinear position embedding with every tensor op rounded to bf16: the weights cast to bf16, each corner product, each of the three
    adds, and the add onto x.  (A product of two bf16 values is exact in f32; an add is one f32 add, then the rounding.)"""
    w = bf(torch.from_numpy(np.ascontiguousarray(wt))).float()             # (4, N)
    e = table.float()[torch.from_numpy(np.ascontiguousarray(idx)).long()]  # (4, N, D)
    p = bf(e * w[..., None]).float()
    s = bf(p[0] + p[1]).float()
    s = bf(s + p[2]).float()
    s = bf(s + p[3]).float()
    return bf(x.float() + s)


def vit_inv_freq():
    """(18) f32: 1 / 10000^(2 j / 36), j < 18, in f32."""
    j = np.arange(VIT_HD // 4, dtype=np.float32)
    return torch.from_numpy((np.float32(1.0) / np.power(np.float32(10000.0), (np.float32(2.0) * j) / np.float32(VIT_HD // 2))).astype(np.float32))


def vit_rope_angles(rowcol, inv_freq):
    """(N, 36) f32: lanes < 18 follow the patch row, the others the column; one f32 multiply float(pos) * inv_freq[lane % 18]."""
    rc = torch.from_numpy(np.ascontiguousarray(rowcol)).to(torch.float32)
    return torch.cat([rc[:, :1] * inv_freq[None], rc[:, 1:] * inv_freq[None]], 1)


def vit_rope_table_ref(rowcol, inv_freq, f32_trig=False):
    """(N, 36, 2) f32 holding bf16 values: (cos, sin) of the f32 angle, from f64 cos / sin (f32_trig: torch's f32 ones)."""
    ang = vit_rope_angles(rowcol, inv_freq)
    if f32_trig:
        c, s = torch.cos(ang), torch.sin(ang)
    else:
        c, s = torch.cos(ang.double()).float(), torch.sin(ang.double()).float()
    return torch.stack([bf(c).float(), bf(s).float()], -1)


def rotate_half(u):
    h = u.shape[-1] // 2
    return torch.cat([-u[..., h:], u[..., :h]], -1)


def vit_rope_apply(u, tab):
    """u (N, nh, 72) bf16, tab (N, 36, 2) -> bf16(bf16(u * cos) + bf16(rotate_half(u) * sin)) with cos / sin = the 36 lanes twice."""
    c = torch.cat([tab[..., 0], tab[..., 0]], -1)[:, None, :]
    s = torch.cat([tab[..., 1], tab[..., 1]], -1)[:, None, :]
    uf = u.float()
    return bf(bf(uf * c).float() + bf(rotate_half(uf) * s).float())


class Pool:
    """n_pages pages of `elems` bf16 elements between two guard pages, all filled with the pattern; the logical pages are a seeded permutation
    of the physical ones.  host: the image before the call; upload() -> dev, ptrs (int64 device addresses in logical order)."""

    def __init__(self, n_pages, elems, seed):
        self.n, self.elems = n_pages, elems
        self.perm = torch.randperm(n_pages, generator=torch.Generator().manual_seed(seed))
        if n_pages > 1 and torch.equal(self.perm, torch.arange(n_pages)):
            self.perm = self.perm.flip(0)
        self.host = filled((n_pages + 2, elems))

    def upload(self):
        self.dev = self.host.cuda()
        self.ptrs = (self.dev.data_ptr() + (1 + self.perm) * self.elems * 2).to(torch.int64).cuda()
        return self.ptrs

    def phys(self, logical):
        return 1 + self.perm[torch.as_tensor(logical, dtype=torch.int64)]


def vit_pages_ref(pool, qkv, tab, tables, nh):
    """-> (q_out (N, nh, 96) bf16, the pool image after the call).  Real tokens: K dims 0..71 rotated, 72..95 zero; V dims 0..71, dim 72 =
    1.0, dims 73..79 zero.  Slots past a page's last token: V all zero, K as it was."""
    N = qkv.shape[0]
    q, k, v = (qkv[:, i * nh * VIT_HD:(i + 1) * nh * VIT_HD].reshape(N, nh, VIT_HD) for i in range(3))
    zq = torch.zeros(N, nh, VIT_DQK - VIT_HD, dtype=torch.bfloat16)
    q_out = torch.cat([vit_rope_apply(q, tab), zq], -1)
    k_row = torch.cat([vit_rope_apply(k, tab), zq], -1).reshape(N, nh * VIT_DQK)
    v_pad = torch.zeros(N, nh, VIT_DV - VIT_HD, dtype=torch.bfloat16)
    v_pad[..., 0] = 1.0
    v_row = torch.cat([v, v_pad], -1).reshape(N, nh * VIT_DV)
    el = kv_pages.slot_index_of(nh, VIT_DQK, VIT_DV)            # (64, nh * 176)
    image = pool.host.clone()
    pg = pool.phys(tables["page_of"])
    image[pg[:, None], el[torch.from_numpy(tables["slot_of"]).long()]] = torch.cat([k_row, v_row], 1)
    for p, (_, cnt) in enumerate(tables["pages"]):
        if cnt < PAGE_TOKENS:
            image[pool.phys(p), el[cnt:, nh * VIT_DQK:].reshape(-1)] = 0
    return q_out, image


# ---- audio staging -----------------------------------------------------------------------------------------------------------------------------
def unfold3(x_nchw):
    """3 x 3, stride 2, padding 1 patches of (B, C, H, W) -> (B * Ho * Wo, C, 9): rows (b, ho, wo), taps (kh, kw)."""
    B, C = x_nchw.shape[:2]
    u = torch.nn.functional.unfold(x_nchw.float(), 3, stride=2, padding=1)     # (B, C * 9, L), channel-major
    return u.reshape(B, C, 9, -1).permute(0, 3, 1, 2).reshape(-1, C, 9)


def audio_chunks(clips, win=100):
    """clips [(first column, frames), ...] -> the chunk table [(first column, frames, window index), ...], clip after clip."""
    return [(c0, F, i) for c0, F in clips for i in range((F + win - 1) // win)]


def audio_im2col1_ref(feat, clips, win=100):
    """feat (mels, ld) f32 -> (C * 64 * 50, 16) bf16: every window of every clip cast to bf16 and zero-padded to `win` frames ON ITS OWN (the
    next clip's frames lie right behind it), unfolded; columns 9..15 zero."""
    wins = []
    for c0, F in clips:
        for s in range(0, F, win):
            n = min(win, F - s)
            wins.append(torch.cat([bf(feat[:, c0 + s:c0 + s + n]), torch.zeros(feat.shape[0], win - n, dtype=torch.bfloat16)], 1))
    cols = unfold3(torch.stack(wins)[:, None])[:, 0]                       # (rows, 9)
    return bf(torch.cat([cols, torch.zeros(cols.shape[0], 7)], 1))


def im2col_nhwc_ref(x):
    """x (B, H, W, C) bf16 -> (B * Ho * Wo, 9 * C) bf16, columns (kh, kw, c)."""
    return bf(unfold3(x.permute(0, 3, 1, 2)).permute(0, 2, 1).reshape(-1, 9 * x.shape[3]))


def sinus_angles(T, d):
    """(T, d / 2) f32: p * w_i, w_i = 10000^(-2 i / d) rounded to f32, one f32 multiply."""
    i = np.arange(d // 2, dtype=np.float64)
    inv = torch.from_numpy(np.power(10000.0, -2.0 * i / d).astype(np.float32))
    return torch.arange(T, dtype=torch.float32)[:, None] * inv[None]


def sinus_table_ref(T, d):
    """(T, d) bf16: cat(sin, cos) of the f32 angles from f64 sin / cos."""
    a = sinus_angles(T, d).double()
    return bf(torch.cat([a.sin(), a.cos()], -1).float())


def kv_pack_ref(pool, src, k_off, v_off, nh, hd, slot_of=None):
    """The pool image after row n's K / V heads (columns k_off / v_off of src) went to cache slot slot_of[n] (None: n)."""
    N = src.shape[0]
    sn = torch.arange(N) if slot_of is None else torch.as_tensor(np.asarray(slot_of), dtype=torch.int64)
    el = kv_pages.slot_index_of(nh, hd, hd)
    image = pool.host.clone()
    image[pool.phys(sn // PAGE_TOKENS)[:, None], el[sn % PAGE_TOKENS]] = torch.cat([src[:, k_off:k_off + nh * hd], src[:, v_off:v_off + nh * hd]], 1)
    return image
