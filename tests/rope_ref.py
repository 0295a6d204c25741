"""The q/k-norm + rotate-half RoPE chain in f64 with the model dtype's rounding points, and the garbage-filled page pool: shared by
tests/test_attn_decode_fused_gpu.py, tests/test_prefill_rope_gpu.py and their CPU tiers.  Plain helpers: no test, no GPU needed to import."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kv_pages  # noqa: E402

D = 128
SPARE_PAGES = 3


def rnd(shape, seed, std=1.0, mean=0.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) * std + mean).to(torch.bfloat16)


def _r(x):
    """One materialisation in the model dtype: f64 -> bf16 -> f64."""
    return x.to(torch.bfloat16).double()


def norm_rope_ref(h, w, cos, sin, eps):
    """RMSNorm over the head dim + rotate-half RoPE of heads h (..., 128) f64, cos / sin (64 values each, or any shape that broadcasts
    against h[..., :64]) f64 -> bf16.  Rounded at the model dtype's materialisation points: the norm's output, the two products, their sum."""
    cos, sin = torch.cat([cos, cos], -1), torch.cat([sin, sin], -1)
    h = _r(h / torch.sqrt(h.pow(2).mean(-1, keepdim=True) + eps) * w.double())
    rot = torch.cat([-h[..., 64:], h[..., :64]], -1)     # element i pairs with i + 64
    return _r(_r(h * cos) + _r(rot * sin)).to(torch.bfloat16)


def prologue_rows_ref(qkv, q_norm_w, k_norm_w, rope, nh, kvh, eps):
    """The chain for many rows: qkv (S, (nh + 2 kvh) * 128) bf16, rope (S, 128) cos[64] | sin[64] -> (q (S, nh, 128) bf16, k (S, kvh, 128)
    bf16, v (S, kvh, 128) bf16 = the rows' v heads as they are)."""
    S = qkv.shape[0]
    x = qkv.double()
    cos, sin = rope[:, None, :64].double(), rope[:, None, 64:].double()
    q = norm_rope_ref(x[:, : nh * D].view(S, nh, D), q_norm_w, cos, sin, eps)
    k = norm_rope_ref(x[:, nh * D: (nh + kvh) * D].view(S, kvh, D), k_norm_w, cos, sin, eps)
    return q, k, qkv[:, (nh + kvh) * D:].view(S, kvh, D)


def prologue_ref(qkv_row, q_norm_w, k_norm_w, rope_row, nh, kvh, eps):
    """-> (q (nh, 128) bf16, k_new (kvh, 128) bf16, v_new (kvh, 128) bf16 = the row's v heads as they are)."""
    q, k, v = prologue_rows_ref(qkv_row[None], q_norm_w, k_norm_w, rope_row[None], nh, kvh, eps)
    return q[0], k[0], v[0]


class Pool:
    """Pages of several sequences in one garbage-filled pool, addressed through a seeded permutation."""

    def __init__(self, kvh, lens, seed):
        self.kvh, self.lens = kvh, list(lens)
        self.npg = [(L + 63) // 64 for L in self.lens]              # pages of a sequence AFTER the append
        self.page0 = [int(x) for x in np.cumsum([0] + self.npg[:-1])]
        P = sum(self.npg) + SPARE_PAGES
        self.host = rnd((P, kv_pages.page_elems(kvh)), seed, 100.0)   # finite garbage everywhere
        self.perm = torch.randperm(P, generator=torch.Generator().manual_seed(seed + 1))

    def phys(self, r, i):
        return int(self.perm[self.page0[r] + i])

    def write(self, r, k_cache, v_cache):
        n = (k_cache.shape[0] + 63) // 64
        if n == 0:
            return
        pg = self.perm[self.page0[r]: self.page0[r] + n]
        self.host[pg] = kv_pages.pack_pages(k_cache, v_cache, self.kvh, out=self.host[pg])

    def upload(self):
        self.dev = self.host.to("cuda")
        self.before = self.dev.clone()
        self.ptrs = (self.dev.data_ptr() + self.perm.to(torch.int64) * self.host.shape[1] * 2).to("cuda")

    def restore(self):
        self.dev.copy_(self.before)

    def changed(self):
        """Flat indices (page * page_elems + element) of the pool elements whose bits differ from before the launch."""
        return torch.nonzero((self.dev.view(torch.int16) != self.before.view(torch.int16)).flatten()).flatten().cpu()

    def slot_elems(self, r):
        """(flat indices of the elements of the slot that row r appends to, the page, the slot)."""
        L = self.lens[r]
        pg, t = self.phys(r, (L - 1) // 64), (L - 1) % 64
        return pg * self.host.shape[1] + kv_pages.slot_index(self.kvh)[t], pg, t


def norm_weights():
    return rnd((D,), 8, 0.1, 1.0), rnd((D,), 9, 0.1, 1.0)
