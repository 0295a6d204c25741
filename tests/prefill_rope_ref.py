"""Reference, inputs and page bookkeeping shared by tests/test_prefill_rope_gpu.py and tests/test_prefill_rope_cpu.py: the prefill's
rope table and q/k-norm + RoPE + paged KV write in torch f64 on the CPU.

  angle   = f32(pos[axis_map[i]]) * inv_freq[i], ONE f32 multiply (what rope_table_kernel and both rope kernels form), of the very f32
            inv_freq the kernels are handed;
  cos/sin = of that f32 angle in f64, rounded to f32 (the reference's cos / sin tensors are f32), then to bf16 (apply_rotary_pos_emb's cast);
  q, k    = tests/rope_ref.py's norm + rotate-half chain (bf16 at the norm's output, the two products, their sum);
  v       = passed through.
"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kv_pages  # noqa: E402
from oracle import qwen3 as oq  # noqa: E402
from rope_ref import Pool, norm_weights, prologue_rows_ref, rnd  # noqa: E402,F401

D = 128
EPS = 1e-6
THETA = 1e6
# (nh, kvh, skip_q): 6 head slots = one partial chunk of 8; exactly one chunk; a second chunk of 2; K only: one head = a half-filled chunk
# of 2; K only: a ragged last chunk of 2; five full chunks, and four with skip_q
HEAD_SHAPES = [(4, 2, 0), (6, 2, 0), (8, 2, 0), (8, 1, 1), (6, 3, 1), (32, 8, 0), (32, 8, 1)]
# (cache offset, S) of the host-offset form: the clamped tail of a 4-token wave; a full page, one row on the next; V pieces covered partly at
# both ends inside one page; into a new page after 3 rows; an aligned full page; mid-page entry over three pages; below 16 rows (the
# per-element kernel writing pages), the last across a page boundary
OFFSET_CASES = [(0, 16), (0, 17), (0, 19), (0, 64), (0, 65), (3, 16), (5, 30), (61, 16), (64, 64), (200, 77), (200, 130), (0, 1), (7, 5), (62, 15)]
TABLE_POSITIONS = list(range(300)) + list(range(4000, 4300)) + list(range(39900, 40200)) + list(range(131000, 131072))
PACKED_LENS = (37, 64, 1, 130)
PACKED_KV0 = (64, 0, 1024, 128)


def inv_freq():
    return oq.compute_default_rope_parameters(D, THETA).float().contiguous()


def axis_plain():
    return torch.zeros(64, dtype=torch.int32)


def axis_mixed():
    """An interleaved M-RoPE map (T, H, W, T, H, W, ... below slot 60, T above), as tests/test_ops_gpu.py::test_qknorm_rope uses."""
    a = torch.zeros(64, dtype=torch.int32)
    for i in range(60):
        a[i] = i % 3
    return a


def positions(S, shift=0):
    """(3, S) int32: the rows' T positions walk through four ranges (from 0, 4000, 39900 and 130000 on), so that every call, however short,
    sees angles near 4e4 and 1.3e5 rad; the H and W rows are the same walk started one and two ranges later."""
    bases = torch.tensor([0, 4000, 39900, 130000])
    i = torch.arange(S)
    q = (i * 4) // max(S, 1)
    return torch.stack([bases[(q + a + shift) % 4] + i for a in range(3)]).to(torch.int32).contiguous()


def angles_f32(pos, axis_map, inv):
    """(S, 64) f32: f32(pos[axis_map[i], s]) * inv[i] as one f32 multiply."""
    p = pos.to(torch.float32)[axis_map.long(), :].t().contiguous()      # exact: positions < 2^24
    assert inv.dtype == torch.float32 and p.dtype == torch.float32
    return p * inv[None, :]


def table_ref(pos, axis_map, inv, f32_trig=False):
    """(S, 128) bf16 cos[64] | sin[64].  f32_trig: torch's f32 cos / sin of the f32 angle instead of f64 rounded to f32 (the CPU cap checks)."""
    ang = angles_f32(pos, axis_map, inv)
    if f32_trig:
        c, s = torch.cos(ang), torch.sin(ang)
    else:
        c, s = torch.cos(ang.double()).float(), torch.sin(ang.double()).float()
    return torch.cat([c, s], 1).to(torch.bfloat16)


def rope_ref(qkv, qn, kn, tab, nh, kvh):
    """-> (q (S, nh * 128), k (S, kvh * 128), v (S, kvh * 128)) bf16 from the bf16 table `tab`."""
    S = qkv.shape[0]
    q, k, v = prologue_rows_ref(qkv, qn, kn, tab, nh, kvh, EPS)
    return q.reshape(S, nh * D), k.reshape(S, kvh * D), v.reshape(S, kvh * D).contiguous()


def bf16_ordinal(x):
    """bf16 -> int32 that counts representable values: consecutive bf16 numbers are 1 apart, -0 and +0 coincide."""
    v = x.contiguous().view(torch.int16).to(torch.int32)
    return torch.where(v < 0, -(v & 0x7FFF), v)


def worst_ulps(got, ref):
    """The figure assert_close_ulps bounds: the largest |got - ref| in bf16 ulps taken at max(|ref|, rms of ref)."""
    g, r = got.float(), ref.float()
    at = torch.maximum(r.abs(), r.pow(2).mean().sqrt())
    return float(((g - r).abs() / torch.pow(2.0, torch.floor(torch.log2(at.clamp_min(1e-30))) - 7)).max())


def exact_share(got, ref):
    return float((got.float() == ref.float()).float().mean())


def same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int16), b.contiguous().view(torch.int16))


# ---- pages -----------------------------------------------------------------------------------------------------------------------------
def token_elems(pool, r, toks):
    """(pool pages (n,), page elements (n, 2 * kvh * 128)) of cache tokens `toks` (a LongTensor) of the pool's sequence r: [k | v] per token."""
    toks = torch.as_tensor(toks, dtype=torch.int64)
    pages = pool.perm[pool.page0[r] + toks // 64]
    return pages, kv_pages.slot_index(pool.kvh)[toks % 64]


def read_tokens(image, pool, r, toks):
    """(k (n, kvh * 128), v (n, kvh * 128)) of cache tokens `toks` of sequence r out of a host image of the pool."""
    pages, el = token_elems(pool, r, toks)
    kv = image[pages[:, None], el]
    return kv[:, : pool.kvh * D].contiguous(), kv[:, pool.kvh * D:].contiguous()


def untouched_mask(pool, written):
    """Boolean (pages, page elements): True where no token of `written` = [(sequence, tokens), ...] lives."""
    m = torch.ones(pool.host.shape, dtype=torch.bool)
    for r, toks in written:
        pages, el = token_elems(pool, r, toks)
        m[pages[:, None], el] = False
    return m


def prefill_prefix(pool, r, n, seed, k_std=1.0):
    """Cache tokens 0 .. n - 1 of sequence r written with kv_pages.pack_pages before the call under test."""
    if n:
        pool.write(r, rnd((n, pool.kvh * D), seed, k_std), rnd((n, pool.kvh * D), seed + 1))


def packed_plan(lens, kv0s, page0s):
    """The rope kernel's view of a packed pass, as plan_packed_pass lays it out: the pages the pass WRITES (per segment, from its kv0 / 64-th
    page on) as one list -> (logical pool pages of that list, row_slot (S), page_rows (n_pages, 2), pos rows kv0 + i)."""
    pages, slot, prow, r0 = [], [], [], 0
    for ln, k0, p0 in zip(lens, kv0s, page0s):
        assert k0 % 64 == 0
        first = len(pages)
        for p in range((ln + 63) // 64):
            pages.append(p0 + k0 // 64 + p)
            prow.append((r0 + p * 64, min(64, ln - p * 64)))
        slot += [first * 64 + i for i in range(ln)]
        r0 += ln
    return pages, slot, prow
