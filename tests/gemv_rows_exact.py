"""Inputs whose dot products are exact, and what the batched decode matvec (gemv_rows: csrc/gemv_rows_body.h, the merge and argmax kernels
of csrc/kernels_batch.hip) must give on them, bit for bit.  No kernel of this project is called here: everything is torch, on whatever
device the caller names.  The method is tests/gemv_exact.py's, for up to 32 activation rows at once:

Weights are gemv_exact.make_inputs' -- small integers times a power of two per 32-column block, exactly representable in bf16, E4M3 and
(fp4) E2M1 -- and the activations are nonzero integers +-1 .. +-8, so that dropping any single k changes an output.  Under the
precondition  max over (r, n) of sum_k |x_rk * W_nk| < 2^22  (asserted on the inputs, never on a kernel's output) every partial sum in any
order is a multiple of 2^-2 below 2^22 and exact in f32: one fixed bit pattern whatever the summation order, the chunks per wave, the K
split or the weight form.  The same holds for the accumulator of v_mfma_f32_16x16x32_bf16: products of two bf16 integers are exact, all
addends are multiples of 2^-2 (2^-12 with the SiLU shift) below 2^22, so any accumulator that keeps 24 bits after aligning to the largest
exponent loses nothing.

ROWS_SHAPES select every launch gemv_rows_plan can reach -- <CW, NRT> in {1, 2} x {1, 2} with 1, 2 and >= 3 K splits -- and the edge code
inside each: the min(n0 + c, N - 1) row clamp (ragged N), the K - 8 re-read of a ragged last chunk with x zeroed past K, waves whose chunks
lie past the end of K, and a last K split that is nearly empty.
"""
import torch

import gemv_exact as gx
from gemv_exact import LOGITS, RESIDUAL, SILU_MUL, SILU_SHIFT, STORE

MAX_ROWS = 32                         # activation rows of a case; a call with R rows reads the first R (row isolation)
ROW_COUNTS = (1, 15, 16, 17, 31, 32)  # one and two row tiles, full and ragged
MERGE_COLS = 256                      # output columns of a merge block = of one (max, index) partial
ARGMAX_STRIDE = 256                   # argmax_rows_kernel: thread t reads partials t, t + 256, ...

# (N, K): what the shape reaches.  (cw, nks) of each is held to PLANS below by the CPU tier, through the library's own plan query.
ROWS_SHAPES = [
    (40, 8),           # smallest K: one fragment, everything else clamped and zeroed (bf16 only)
    (40, 32),          # smallest MX K
    (40, 160),         # ragged N, partial last chunk, two idle waves
    (40, 264),         # K % 32 == 8: the bf16 K - 8 re-read (bf16 only)
    (96, 1024),        # fallback to CW = 1 with 2 splits
    (64, 1032),        # fallback, 3 splits, the last split one partial chunk (bf16 only)
    (72, 4128),        # fallback, 9 splits, ragged N
    (8192, 1024),      # CW = 2, one split
    (8200, 672),       # CW = 2, one split, ragged N; one wave's chunks past the end, another with a partial second chunk
    (4096, 2048),      # CW = 2, 2 splits
    (4104, 2080),      # CW = 2, 3 splits, the last split nearly empty, ragged N
    (680, 12288),      # CW = 2, 12 splits: the longest sum
    (65800, 64),       # LOGITS only: more than 256 merge tiles, ragged last tile
]
PLANS = {(40, 8): (1, 1), (40, 32): (1, 1), (40, 160): (1, 1), (40, 264): (1, 1), (96, 1024): (1, 2), (64, 1032): (1, 3), (72, 4128): (1, 9),
         (8192, 1024): (2, 1), (8200, 672): (2, 1), (4096, 2048): (2, 2), (4104, 2080): (2, 3), (680, 12288): (2, 12), (65800, 64): (1, 1)}
LOGITS_ONLY = {(65800, 64)}
TIE_SHAPES = [(65800, 64), (8200, 672), (296, 160)]          # every relation; no stride relation; a small ragged one of two merge blocks
GAUSSIAN_SHAPES = [(40, 160), (72, 4128), (8200, 672), (4104, 2080)]          # one per plan branch, all ragged
# the plan query's sweep: every K, N around the threshold nb * nks = 256 of the CW = 2 launch, a small matrix and the widest
SWEEP_N = (8, 8160, 8161, 65800)
PROBE_KS = (0, 7, 8, 31, 32, 127, 128, 511, 512)          # and K - 33, K - 32, K - 9, K - 8, K - 1


def seed_of(N, K, fp4=False):
    return 104729 * int(fp4) + 31 * N + K


def epilogues(N, K):
    """The epilogues a shape runs: SILU_MUL's fused layout comes in whole 32-row blocks."""
    if (N, K) in LOGITS_ONLY:
        return (LOGITS,)
    return (STORE, RESIDUAL, SILU_MUL, LOGITS) if N % 32 == 0 else (STORE, RESIDUAL, LOGITS)


def forms(K):
    """The weight forms a shape runs: an MX block is 32 columns."""
    return ("bf16", "mxfp8", "mxfp4") if K % 32 == 0 else ("bf16",)


def nks_class(nks):
    return min(nks, 3)          # 1, 2, >= 3 K splits


def launches(plan, shapes=ROWS_SHAPES):
    """{(cw, nrt, nks class)} the shapes' cases launch, by a plan query (N, K) -> (cw, nks)."""
    return {(plan(N, K)[0], 1 + (R > 16), nks_class(plan(N, K)[1])) for N, K in shapes for R in ROW_COUNTS}


def reachable(plan):
    """{(cw, nks class)} over every K the entries take and SWEEP_N."""
    return {(cw, nks_class(nks)) for N in SWEEP_N for K in range(8, 32768 + 8, 8) for cw, nks in (plan(N, K),)}


# ---- inputs -----------------------------------------------------------------------------------------------------------------------------
def sums_of(c):
    """(x W^T, |x| |W|^T) in float64, (32, N), a block of weight rows at a time."""
    W, x = c["W"], c["x"].double()
    N, K = W.shape
    s = torch.empty(x.shape[0], N, dtype=torch.float64, device=W.device)
    sa = torch.empty_like(s)
    step = max(1, (1 << 25) // K)
    for n0 in range(0, N, step):
        Wd = W[n0:n0 + step].double()
        s[:, n0:n0 + step] = x @ Wd.T
        sa[:, n0:n0 + step] = x.abs() @ Wd.abs().T
    return s, sa


def check_rows_preconditions(c):
    """On the inputs alone: the integer ranges, no zero activation, sum_k |x_rk * W_nk| < 2^22 for every (r, n), every sum a multiple of
    2^-2.  Fills c["sums"] (32, N) float64, the exact dot products."""
    mag = c["ints"].abs()
    assert int(mag.max()) <= (6 if c["fp4"] else 8) and not (c["fp4"] and bool((mag == 5).any()))
    assert int(c["j"].min()) >= gx.BLOCK_SHIFTS[0] and int(c["j"].max()) <= gx.BLOCK_SHIFTS[-1]
    x, res = c["x"].double(), c["res"].double()
    assert x.shape == (MAX_ROWS, c["K"]) and res.shape == (MAX_ROWS, c["rows"])
    assert bool((x == x.round()).all()) and float(x.abs().min()) >= 1 and float(x.abs().max()) <= 8
    assert bool((res == res.round()).all()) and float(res.abs().max()) <= 128
    c["sums"], sabs = sums_of(c)
    assert float(sabs.max()) < gx.EXACT_BOUND, f"sum |x W| reaches {float(sabs.max())}"
    assert bool((c["sums"] * 4 == (c["sums"] * 4).round()).all())
    return c


def make_rows_case(N, K, fp4=False, seed=0, device="cpu"):
    """{rows = N, K, fp4, ints (N, K) int8, j (N, ceil(K / 32)) int8, W = ints * 2^j bf16 (gemv_exact.make_inputs'), x (32, K) bf16 nonzero
    integers +-1 .. +-8, res (32, N) bf16 integers -128 .. 128, sums (32, N) float64 = x W^T exactly}; the preconditions asserted."""
    dev = torch.device(device)
    c = {k: v for k, v in gx.make_inputs(N, K, fp4, device, seed).items() if k in ("rows", "K", "fp4", "ints", "j", "W")}
    g = torch.Generator(device=dev).manual_seed(seed + 1000003)
    mag = torch.randint(1, 9, (MAX_ROWS, K), generator=g, device=dev)
    sign = torch.randint(0, 2, (MAX_ROWS, K), generator=g, device=dev) * 2 - 1
    c["x"] = (mag * sign).to(torch.bfloat16)
    c["res"] = torch.randint(-128, 129, (MAX_ROWS, N), generator=g, device=dev).to(torch.bfloat16)
    return check_rows_preconditions(c)


def probe_ks(K):
    """The probed k of a matrix with K columns: those of the list that exist, each once, ascending."""
    return sorted({k for k in PROBE_KS + (K - 33, K - 32, K - 9, K - 8, K - 1) if 0 <= k < K})


def probe_rows(K, device="cpu"):
    """(ks, x): x (len(ks), K) bf16, row i the unit vector e_ks[i].  Output row i of a matvec is column ks[i] of W, as bf16, exactly: a
    differing probe names the misplaced k."""
    ks = probe_ks(K)
    x = torch.zeros(len(ks), K, dtype=torch.bfloat16, device=device)
    x[torch.arange(len(ks)), torch.tensor(ks)] = 1
    return ks, x


# ---- what the kernels must give ---------------------------------------------------------------------------------------------------------
def first_max(lin):
    """The first maximal index of every row of a (R, N) tensor."""
    N = lin.shape[1]
    idx = torch.arange(N, device=lin.device).expand_as(lin)
    return torch.where(lin == lin.max(dim=1, keepdim=True).values, idx, N).min(dim=1).values


def epilogue(s, res, epi):
    """Float64 sums (R, N) -> the epilogue's output, bf16 round-to-nearest-even at the reference's op boundaries (the merge kernel's
    comments cite them): STORE bf16(sum); RESIDUAL bf16(res + bf16(sum)); SILU_MUL (the sums of the weights scaled by 2^SILU_SHIFT, fused
    16-row gate / up blocks) bf16(bf16(silu(bf16(gate))) * bf16(up)); LOGITS (f32 of bf16(sum), the first maximal index of every row)."""
    if epi == SILU_MUL:
        assert s.shape[1] % 32 == 0
        gi, ui = gx.gate_up_rows(s.shape[1])
        gate, up = s[:, gi.to(s.device)].contiguous(), s[:, ui.to(s.device)].contiguous()
        lin = gx.bf16_rne(gate)
        prod = gx.bf16_rne(lin / (1.0 + torch.exp(-lin))) * gx.bf16_rne(up)
        # gemv_exact.silu_mul, and the sign of a zero product kept: bf16_rne returns +0 for -0, but a gate or up sum of exactly 0 next to a
        # negative partner gives -0 in the reference's bf16 multiply, and a bit comparison sees it
        return gx.as_bf16(torch.where(prod == 0, prod, gx.silu_mul(gate, up)))
    lin = gx.bf16_rne(s)
    if epi == STORE:
        return gx.as_bf16(lin)
    if epi == RESIDUAL:
        return gx.as_bf16(gx.bf16_rne(res.double() + lin))
    assert epi == LOGITS
    return gx.as_f32(lin), first_max(lin)


def expected_rows(c, R, epi):
    """What a call with the first R activation rows must give.  SILU_MUL reads gemv_exact.weights(c, SILU_SHIFT) (or its MX encodings with
    that shift): the gates are O(1), the sums as exact."""
    s = c["sums"][:R]
    return epilogue(s * 2.0 ** SILU_SHIFT if epi == SILU_MUL else s, c["res"][:R], epi)


def assert_rows(got, want, epi, what=""):
    """Zero tolerance: every bit of the bf16 / f32 outputs, and for LOGITS the argmax of every row."""
    if epi != LOGITS:
        return assert_bits_2d(got, want, what)
    assert_bits_2d(got[0], want[0], what)
    bad = torch.nonzero(got[1].cpu() != want[1].cpu()).flatten()
    assert bad.numel() == 0, (f"{what}: argmax of row {int(bad[0])} is {int(got[1][bad[0]])}, the first maximal index is "
                              f"{int(want[1][bad[0]])} ({bad.numel()} rows differ)")


def assert_bits_2d(got, want, what=""):
    assert got.dim() == 2
    bad = gx.mismatches(got.reshape(-1), want.reshape(-1))
    if bad.numel():
        r, n = divmod(int(bad[0]), got.shape[1])
        cols = sorted({int(b) % got.shape[1] for b in bad[:4096]})
        raise AssertionError(f"{what}: {bad.numel()} of {got.numel()} outputs differ; first at row {r}, column {n}: got {float(got[r, n])!r}, "
                             f"want {float(want[r, n])!r}; columns {cols[:8]}{' ...' if len(cols) > 8 else ''}")


def assert_probes(got, W, ks, what=""):
    """Output row i of the probe launch against column ks[i] of W (got f32 or bf16; W bf16)."""
    want = W[:, ks].T.contiguous().to(got.dtype)
    bad = torch.nonzero((gx.bits(got) != gx.bits(want.to(got.device))).any(dim=1)).flatten().tolist()
    assert not bad, f"{what}: the probes of k = {[ks[i] for i in bad]} do not return their column of W"


# ---- planted argmax ties ----------------------------------------------------------------------------------------------------------------
# The logits epilogue's (max, first index) goes through the merge kernel's 256-column blocks, argmax_rows_kernel's stride-256 loop over the
# blocks' partials, and the final pick.  A relation is a pair of columns (p < q) that both hold their activation row's maximum.
RELATIONS = {
    "same merge block": lambda p, q, N: p // MERGE_COLS == q // MERGE_COLS and p // 32 != q // 32,
    "neighbouring merge blocks": lambda p, q, N: q == p + 1 and q % MERGE_COLS == 0,
    "same argmax thread": lambda p, q, N: q // MERGE_COLS > p // MERGE_COLS and (q // MERGE_COLS - p // MERGE_COLS) % ARGMAX_STRIDE == 0,
    "last column": lambda p, q, N: q == N - 1,
    "two MFMA tiles of a block": lambda p, q, N: p // 32 == q // 32 and p // 16 != q // 16,
}


def tie_pairs(N):
    """{relation: (p, q)} where the ties are planted: the relations that exist for N, on columns no other relation uses."""
    want = {"same merge block": (3, min(200, N - 2)),
            "neighbouring merge blocks": (MERGE_COLS - 1, MERGE_COLS),
            "same argmax thread": (MERGE_COLS + 5, (ARGMAX_STRIDE + 1) * MERGE_COLS + 5),
            "last column": (20, N - 1),
            "two MFMA tiles of a block": (7, 23)}
    out, used = {}, set()
    for name, (p, q) in want.items():
        if 0 <= p < q < N and RELATIONS[name](p, q, N) and not {p, q} & used:
            out[name] = (p, q)
            used |= {p, q}
    return out


def max_columns(c):
    """Per activation row, the columns that hold the row's largest logit (of the final inputs)."""
    lin = gx.bf16_rne(c["sums"])
    top = lin == lin.max(dim=1, keepdim=True).values
    return [torch.nonzero(top[r]).flatten().tolist() for r in range(lin.shape[0])]


def relations_achieved(c):
    """{relation: [activation rows whose maximum is attained at a pair of columns in that relation]}, from c's inputs as they are."""
    N = c["rows"]
    out = {name: [] for name in RELATIONS}
    for r, cols in enumerate(max_columns(c)):
        for name, rel in RELATIONS.items():
            if any(rel(p, q, N) for i, p in enumerate(cols) for q in cols[i + 1:]):
                out[name].append(r)
    return {k: v for k, v in out.items() if v}


def plant_row_ties(c, pairs=None):
    """For each relation of tie_pairs (or `pairs`), one activation row of its own: the weight row (output column) that holds the row's
    maximum is moved to both columns of the pair (what stood in the first goes where the maximum was), in ints, j and W alike, so every
    weight form sees it.  Then the sums are recomputed and the preconditions asserted again.  Returns relations_achieved(c): computed from
    the final inputs, as the expected argmax is (expected_rows: the reference's first maximal index), never from what was copied."""
    pairs = tie_pairs(c["rows"]) if pairs is None else pairs
    taken = {col for pq in pairs.values() for col in pq}
    r = 0
    for name, (p, q) in pairs.items():
        while True:          # the next activation row whose maximum stands alone on a column no relation uses
            assert r < MAX_ROWS, "out of activation rows"
            cols = max_columns(c)[r]
            r += 1
            if len(cols) == 1 and cols[0] not in taken:
                break
        m = cols[0]
        for key in ("ints", "j", "W"):
            old = c[key][p].clone()
            c[key][p] = c[key][m]
            c[key][q] = c[key][m]
            c[key][m] = old
        taken.add(m)
        c["sums"], _ = sums_of(c)
    check_rows_preconditions(c)
    assert torch.equal(c["W"], gx.weights(c))
    return relations_achieved(c)


# ---- Gaussian inputs: non-trivial mantissas against the f64 chain -----------------------------------------------------------------------
def gaussian_rows_case(N, K, R, device="cpu", seed=0):
    dev = torch.device(device)
    g = torch.Generator(device=dev).manual_seed(seed)
    return dict(W=(torch.randn(N, K, generator=g, device=dev) * 0.02).to(torch.bfloat16),
                x=torch.randn(R, K, generator=g, device=dev).to(torch.bfloat16),
                res=torch.randn(R, N, generator=g, device=dev).to(torch.bfloat16))


def gaussian_rows_expected(c, epi):
    """The f64 chain rounded at the op boundaries: bf16 values (LOGITS: the f32 logits alone)."""
    c = dict(c, sums=sums_of(c)[0])
    out = epilogue(c["sums"], c["res"], epi)
    return out[0] if epi == LOGITS else out
