"""Host mirror of the fragment-major KV page layout (aha_amd/csrc/common.h "KV page layout", kernels.h KvPages), for tests.

Written from the layout's description, not from the kernels' index expressions: a page holds 64 token slots of every kv head, the K
block [kvh][64 * 128] first and the V block [kvh][128 * 64] behind it.  One kv head's share of either block is a row of 1 KB (512
element) MFMA operand fragments; the 16-byte piece l of a fragment (8 elements) is what lane l = G * 16 + c of a wave feeds
v_mfma_f32_16x16x32_bf16:

  K: fragment (sub, k4), stored at index sub * KS + k4 (KS = head dim / 32): piece l = dims k4*32 + G*8 .. +8 of token sub*16 + c
  V: fragment (ds, kk), stored at index ds * 2 + kk:                         piece l = slots kk*32 + G*8 .. +8 of dim ds*16 + c

where a V "slot" is the token's position after the per-page permutation v_slot: token kk*32 + sub1*16 + G*4 + j sits in slot
kk*32 + G*8 + sub1*4 + j.
"""
import torch

PAGE_TOKENS = 64
HEAD_DIM = 128
HEAD_ELEMS = PAGE_TOKENS * HEAD_DIM   # one kv head's share of the K (or V) block of a page
FRAG_ELEMS = 512                      # 1 KB of bf16
PIECE_ELEMS = 8                       # 16 bytes of bf16


def v_slot(t):
    """Slot of token t (0..63) inside a V page."""
    kk, sub1, G, j = t // 32, (t // 16) % 2, (t // 4) % 4, t % 4
    return kk * 32 + G * 8 + sub1 * 4 + j


def kpage_elem(t, e, KS=4):
    """Element index, from the start of the kv head's K block, of dim e of token slot t."""
    sub, c = divmod(t, 16)
    k4, G, j = e // 32, (e % 32) // 8, e % 8
    return (sub * KS + k4) * FRAG_ELEMS + (G * 16 + c) * PIECE_ELEMS + j


def vpage_elem(t, e):
    """Element index, from the start of the kv head's V block, of dim e of token slot t."""
    s = v_slot(t)
    kk, G, j = s // 32, (s % 32) // 8, s % 8
    ds, c = divmod(e, 16)
    return (ds * 2 + kk) * FRAG_ELEMS + (G * 16 + c) * PIECE_ELEMS + j


def page_elems(kvh):
    return 2 * kvh * HEAD_ELEMS


_TABLES = {}


def slot_index(kvh):
    """(64, 2 * kvh * 128) int64: page element of [k (kvh * 128) | v (kvh * 128)] of every token slot."""
    if kvh not in _TABLES:
        ke = torch.tensor([[kpage_elem(t, e) for e in range(HEAD_DIM)] for t in range(PAGE_TOKENS)])
        ve = torch.tensor([[vpage_elem(t, e) for e in range(HEAD_DIM)] for t in range(PAGE_TOKENS)])
        heads = [ke + h * HEAD_ELEMS for h in range(kvh)] + [ve + (kvh + h) * HEAD_ELEMS for h in range(kvh)]
        _TABLES[kvh] = torch.cat(heads, 1)
    return _TABLES[kvh]


def page_elems_of(nh, dqk, dv):
    """Elements of a page whose K rows hold dqk dims (a multiple of 32: dqk / 32 fragments per 16 tokens) and whose V block holds dv dims (a
    multiple of 16): the K block [nh][64 * dqk], then the V block [nh][dv * 64].  The ViT's pages are 96 / 80, the audio tower's 64 / 64."""
    return nh * PAGE_TOKENS * (dqk + dv)


_TABLES_OF = {}


def slot_index_of(nh, dqk, dv):
    """(64, nh * (dqk + dv)) int64: page element of [k (nh * dqk) | v (nh * dv)] of every token slot of a (dqk, dv) page;
    slot_index_of(kvh, 128, 128) is slot_index(kvh)."""
    key = (nh, dqk, dv)
    if key not in _TABLES_OF:
        assert dqk % 32 == 0 and dv % 16 == 0
        ke = torch.tensor([[kpage_elem(t, e, dqk // 32) for e in range(dqk)] for t in range(PAGE_TOKENS)])
        ve = torch.tensor([[vpage_elem(t, e) for e in range(dv)] for t in range(PAGE_TOKENS)])
        heads = [ke + h * PAGE_TOKENS * dqk for h in range(nh)] + [ve + nh * PAGE_TOKENS * dqk + h * dv * PAGE_TOKENS for h in range(nh)]
        _TABLES_OF[key] = torch.cat(heads, 1)
    return _TABLES_OF[key]


def pack_pages(k, v, kvh, out=None):
    """Token-major k, v (L, kvh * 128) -> page images (ceil(L / 64), 2 * kvh * 64 * 128), token i in slot i % 64 of page i // 64.  `out`:
    the pre-filled images to write into (default: zeros); the slots of tokens >= L keep what it holds."""
    L = k.shape[0]
    assert k.shape == v.shape == (L, kvh * HEAD_DIM)
    npages = (L + PAGE_TOKENS - 1) // PAGE_TOKENS
    if out is None:
        out = torch.zeros(npages, page_elems(kvh), dtype=k.dtype)
    assert out.shape == (npages, page_elems(kvh))
    tok = torch.arange(L)
    out[(tok // PAGE_TOKENS)[:, None], slot_index(kvh)[tok % PAGE_TOKENS]] = torch.cat([k, v], 1).to(out.dtype)
    return out


def unpack_slot(page, kvh, t):
    """(k (kvh * 128), v (kvh * 128)) of token slot t of one page image."""
    kv = page[slot_index(kvh)[t].to(page.device)]
    return kv[: kvh * HEAD_DIM], kv[kvh * HEAD_DIM:]


def slot_mask(kvh, t):
    """Boolean mask over a page image: the 2 * kvh * 128 elements that belong to token slot t."""
    m = torch.zeros(page_elems(kvh), dtype=torch.bool)
    m[slot_index(kvh)[t]] = True
    return m
