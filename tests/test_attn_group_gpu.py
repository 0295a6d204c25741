"""-m gpu: attn_decode_group_kernel (kernels_attn_group.hip) at op level, through ops.attn_decode_group: the rows of one sequence in one pass
over its KV pages.  The contract is that of the draft-and-verify step it serves: every row gets the bits of attn_decode_rows_kernel
(ops.debug_attn_decode_rows form 1) on the same rows from the same pool image.

Shapes and runs are tests/spec_rows_ref.py's, all runs of RUNS in one call per head shape.  What they reach in this kernel: (0, 15) a row of
kv_len 1 and units without a page; (56, 15) later rows own a page that the earlier rows' columns must pass unchanged; (63, 1), (64, 3) the
page edge; (250, 15), (1020, 7), (4090, 15) the run is cut where the split count changes, and (4090, 15) takes both final merges (16 and 17
splits); (300, 0) a group of one.  g = 1: 16 rows in one tile; g = 3: five rows and an idle column per tile; g = 4: four tiles of four
rows; g = 16: a tile per row, every run cut into groups of four."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import spec_rows_ref as S  # noqa: E402
from spec_rows_ref import D, EPS, ORDERS, SHAPES, layout  # noqa: E402
from test_attn_decode_fused_gpu import ULPS  # noqa: E402
from test_ops_gpu import assert_close_ulps  # noqa: E402
from test_spec_rows_gpu import Launcher, bits, case, case2, differing_rows, on_device  # noqa: E402,F401

pytestmark = pytest.mark.gpu


class GroupLauncher(Launcher):
    def group(self, rows):
        """ops.attn_decode_group on `rows` -> the outputs in canonical row order on the CPU."""
        from aha_amd import ops
        c = self.c
        idx = torch.tensor([r.id for r in rows], device="cuda")
        o = ops.attn_decode_group(self.qkv[idx].contiguous(), self.qn, self.kn, self.rope[idx].contiguous(), self.pool.ptrs,
                                  [self.pool.page0[c.pool_seq[r.seq]] for r in rows], [r.kv_len for r in rows], c.nh, c.kvh, EPS, c.scale)
        torch.cuda.synchronize()
        out = torch.zeros(c.R, c.nh * D, dtype=torch.bfloat16)
        out[idx.cpu()] = o.cpu()
        return out


def check_bits(c, ln, start):
    """From the pool image `start`: the group call on all rows, both orders, twice each, against form 1; the pool against form 2's."""
    pool = c.pool
    for order in ORDERS:
        rows = layout(c.runs, order)[0]
        pool.dev.copy_(start)
        ln.run(rows, 2)
        appended = pool.dev.clone()
        pool.dev.copy_(start)
        want = ln.run(rows, 1)
        for rep in range(2):
            pool.dev.copy_(start)
            got = ln.group(rows)
            bad = differing_rows(c, got, want)
            assert not bad, f"{order} order, call {rep}: (run, row) whose grouped output differs from the row-by-row launch: {bad}"
            assert torch.equal(bits(pool.dev), bits(appended)), f"{order} order: the pool differs from the pool after the append alone"


@pytest.mark.parametrize("nh,kvh", SHAPES)
def test_group_bits_equal_the_row_by_row_launch(gpu, on_device, nh, kvh):
    c, pool = case(nh, kvh), on_device(nh, kvh)
    check_bits(c, GroupLauncher(c), pool.before)


@pytest.mark.parametrize("nh,kvh", SHAPES)
def test_group_rows_against_the_f64_reference(gpu, on_device, nh, kvh):
    """Every row against fused_ref over the tokens the append left in the pool, at the project's decode-attention bound."""
    c, pool = case(nh, kvh), on_device(nh, kvh)
    g = nh // kvh
    o = GroupLauncher(c).group(layout(c.runs, "consecutive")[0])
    image = pool.dev.cpu()
    first = S.first_ids(c.runs)
    for s, (L0, k) in enumerate(c.runs):
        k_all, v_all = pool.tokens(s, L0 + k, image)
        ref = S.run_ref(c, s, k_all, v_all)
        for i in range(k + 1):
            r = first[s] + i
            got, want = o[r], ref[r].to(torch.bfloat16)
            assert_close_ulps(got.view(nh, D), want.view(nh, D), ULPS, None, f"run {(L0, k)} row {i}, per head", row_scale=True)
            assert_close_ulps(got, want, ULPS, None, f"run {(L0, k)} row {i}, row rms")
            if L0 + i == 0:   # kv_len 1: p = 1 and sum = 1, the output IS the new v
                v_new = c.ref_v[r].view(kvh, 1, D).expand(kvh, g, D).contiguous()
                assert torch.equal(bits(got.view(kvh, g, D)), bits(v_new)), "kv_len 1 must return the new v bit for bit"


@pytest.mark.parametrize("nh,kvh", SHAPES)
def test_group_second_step_over_a_rejected_run(gpu, on_device, nh, kvh):
    """Step 1 (grouped) leaves 16 appended tokens behind (56, 15) and (250, 15); step 2 starts at L0 + 3 with other rows and 7 drafts over
    the stale slots: the bits again."""
    c1, pool = case(nh, kvh), on_device(nh, kvh)
    GroupLauncher(c1).group(layout(c1.runs, "consecutive")[0])
    c2 = case2(nh, kvh)
    check_bits(c2, GroupLauncher(c2), pool.dev.clone())
