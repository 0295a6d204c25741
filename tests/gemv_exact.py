"""Inputs whose dot products are exact, and what the single-sequence matvec must give on them, bit for bit.  No kernel of this project is
called here: everything is torch, on whatever device the caller names (the CPU tier runs it on the CPU).

Weights are small integers times a power of two per 32-column block, activations small integers.  Every product is then a multiple of
2^-2, and under the precondition  sum_k |x_k * W_nk| < 2^22  (asserted on the inputs, never on a kernel's output) every partial sum in
any order is a multiple of 2^-2 below 2^22: 24 significant bits, exact in f32.  The f32 accumulator of a correct kernel therefore holds
the mathematical sum whatever its summation order, rows per wave, chunks per item, grid or weight format, and the output is a fixed
value that can be compared with zero tolerance.  A dropped, duplicated or misplaced element changes it, and so does a rounding that is
not bf16 round-to-nearest-even at the reference's op boundaries.

The same weights are exactly representable in all four forms the matvec reads: bf16, MXFP8 (E4M3 holds the integers -8 .. 8), MXFP4
(E2M1 holds 0, +-1, +-2, +-3, +-4, +-6) and the 13-bit copies (every weight within 8 binades).  encode_mxfp8 / encode_mxfp4 write the
codes and scale bytes directly -- an integer's code, the block's own exponent -- so a kernel's input does not pass through the
quantiser either; tests/test_gemv_exact_cpu.py holds them to aha_amd/quant.py's dequantisers and shows that the quantisers round-trip
these matrices exactly.

The norm prologue is exact as well: |x_k| = 2 with random signs, integer norm weights -4 .. 4, eps = 0.  The sum of squares is 4K
(exact), 4K / K = 4, 1.0f / sqrtf(4.0f) = 0.5 (no fast-math), and h_k = bf16(x_k * 0.5 * nw_k) = +-nw_k.
"""
import torch

STORE, RESIDUAL, SILU_MUL, LOGITS, PARTIAL_F32 = 0, 1, 2, 3, 4
EXACT_BOUND = 2.0 ** 22
SILU_SHIFT = -10                      # SILU_MUL reads W * 2^-10: the gates are O(1), the sums as exact
FP4_VALUES = (0, 1, 2, 3, 4, 6, -1, -2, -3, -4, -6)
BLOCK_SHIFTS = (-2, -1, 0, 1, 2)      # a 32-column block is its integers times 2^j: the MX scale bytes differ from block to block

# (rows the plan sees, K) of the bf16 kernel's cases; SILU_MUL reads two matrices of that many rows (the entry's N is twice the rows).
# Rows per wave R by the rows: 1 below 8185, 2 below 16369, then 4 (gate+up: 1 / 2).  Chunks per item U by K.  K = 512 * U: FAST with the
# straight-line prologue; + 8: the general form with a partial last chunk; past 8192 (with norm weights) / 16384 (without): FAST with the
# general prologue.  16416 rows: 1026 tiles (gate+up: 2052) on 768 blocks, the persistent walk; 100000: uneven rounds in the general form.
BF16_SHAPES = [(40, 160), (40, 264), (64, 512), (64, 1024), (64, 1032), (64, 2048), (64, 2056), (64, 4096), (64, 4104), (64, 8192),
               (64, 8200), (64, 10240), (32, 12288), (32, 16384), (32, 16896), (32, 20480), (4100, 512), (4096, 4096), (3080, 1536),
               (8224, 160), (8224, 512), (8224, 520), (8224, 1024), (8224, 1032), (8224, 2048), (8224, 2056), (8224, 4096), (8224, 4104),
               (8224, 8200), (8224, 12288), (8224, 20480),
               (16416, 160), (16416, 512), (16416, 520), (16416, 1024), (16416, 1032), (16416, 2048), (16416, 2056), (16416, 4096),
               (16416, 10240), (16416, 18432), (100000, 64)]
# the FAST forms with more tiles than blocks, for every epilogue, with and without norm weights
BF16_MULTI_TILE_FAST = [(16416, 512), (16416, 1024), (16416, 2048), (16416, 4096), (16416, 10240), (16416, 18432)]
# the plan query's sweep: every K, rows at and around the two thresholds of R (and a small matrix)
SWEEP_ROWS = (8, 8184, 8185, 16368, 16369)
# one Gaussian case per R (non-trivial 1 / rms values), held to tests/test_ops_gpu.py test_gemv's bound
GAUSSIAN_SHAPES = [(152, 264), (8224, 520), (16416, 1024)]


def instantiation(epi, plan):
    """(R, U, epi, FAST, PRO) of a plan query's (R, U, grid, form)."""
    r, u, _, form = plan
    return r, u, epi, int(form != 0), max(form - 1, 0)


def bf16_reachable(plan, epis=(STORE, RESIDUAL, SILU_MUL, LOGITS)):
    """Every instantiation the bf16 launch can select, by a sweep of the library's query (plan(N, K, epi, norm) -> (R, U, grid, form),
    N the entry's: twice the rows for SILU_MUL) over every K and the rows at and around the thresholds of R."""
    return {instantiation(epi, plan(2 * rows if epi == SILU_MUL else rows, K, epi, norm))
            for K in range(8, 32768 + 8, 8) for rows in SWEEP_ROWS for epi in epis for norm in (False, True)}


def bf16_covered(plan, epis=(STORE, RESIDUAL, SILU_MUL, LOGITS)):
    """The instantiations BF16_SHAPES' cases run."""
    return {instantiation(epi, plan(2 * rows if epi == SILU_MUL else rows, K, epi, norm))
            for rows, K in BF16_SHAPES for epi in epis for norm in (False, True)}


def assert_multi_tile_fast(plan):
    """BF16_MULTI_TILE_FAST: more tiles than blocks in a FAST form, for every epilogue, with and without norm weights."""
    assert set(BF16_MULTI_TILE_FAST) <= set(BF16_SHAPES)
    for rows, K in BF16_MULTI_TILE_FAST:
        for epi in (STORE, RESIDUAL, SILU_MUL, LOGITS, PARTIAL_F32):
            for norm in (False, True):
                r, u, grid, form = plan(2 * rows if epi == SILU_MUL else rows, K, epi, norm)
                assert -(-rows // (4 * r)) > grid and form != 0, (rows, K, epi, norm, r, u, grid, form)


def bf16_case_count(rows):
    """(epilogue, norm) cases of one bf16 shape: STORE, RESIDUAL, LOGITS, PARTIAL_F32, SILU_MUL on separate gate / up matrices, and
    SILU_MUL on the fused layout where its 16-row blocks are whole (the entry refuses N % 32 != 0); each with and without norm weights."""
    return 2 * (5 + (rows % 16 == 0))


def mx_case_count(N):
    """The MX forms and their shapes' N (the entry's): STORE, RESIDUAL, LOGITS, and SILU_MUL where N % 32 == 0; with and without norm."""
    return 2 * (3 + (N % 32 == 0))


# ---- rounding and comparing -------------------------------------------------------------------------------------------------------------
def bf16_rne(v):
    """float64 -> the nearest bf16 value, ties to even, as float64: on the bits of the double, not through torch's own conversions."""
    assert v.dtype == torch.float64
    a = v.abs().contiguous().view(torch.int64)          # sign cleared: a non-negative integer, ordered like the magnitude
    q, rem = a >> 45, a & ((1 << 45) - 1)               # bf16 keeps 7 of the 52 mantissa bits
    q = q + ((rem > (1 << 44)) | ((rem == (1 << 44)) & ((q & 1) == 1))).to(torch.int64)      # a carry runs into the exponent by itself
    mag = (q << 45).view(torch.float64)
    assert bool(((mag == 0) | ((mag >= 2.0 ** -126) & (mag < 2.0 ** 128))).all()), "outside bf16's normal range"
    return torch.where(v < 0, -mag, mag)


def bits(t):
    """The bit patterns of a bf16 / f32 tensor."""
    t = t.contiguous()
    return t.view(torch.int16) if t.dtype == torch.bfloat16 else t.view(torch.int32) if t.dtype == torch.float32 else t


def as_bf16(v):
    """A float64 tensor of bf16 values (bf16_rne's output) as bf16: the conversion is exact."""
    out = v.to(torch.bfloat16)
    assert bool((out.double() == v).all())
    return out


def as_f32(v):
    out = v.to(torch.float32)
    assert bool((out.double() == v).all())
    return out


def mismatches(got, want):
    """Indices where got and want differ in any bit."""
    assert got.shape == want.shape and got.dtype == want.dtype, (got.shape, want.shape, got.dtype, want.dtype)
    return torch.nonzero(bits(got) != bits(want.to(got.device))).flatten()


def assert_same_bits(got, want, what=""):
    bad = mismatches(got, want)
    if bad.numel():
        i = int(bad[0])
        raise AssertionError(f"{what}: {bad.numel()} of {got.numel()} outputs differ; first at row {i}: got {float(got[i])!r}, "
                             f"want {float(want[i])!r}")


def assert_logits(got, want, what=""):
    """(logits f32, argmax) against (expected logits, the first maximal index)."""
    assert_same_bits(got[0], want[0], what)
    assert int(got[1]) == int(want[1]), f"{what}: argmax {int(got[1])}, the first maximal index is {int(want[1])}"


# ---- inputs -----------------------------------------------------------------------------------------------------------------------------
def make_inputs(rows, K, fp4=False, device="cpu", seed=0):
    """{ints (rows, K) int8, j (rows, ceil(K / 32)) int8, W = ints * 2^j bf16, x, res, xn, nw}: seeded, no kernel involved."""
    dev = torch.device(device)
    g = torch.Generator(device=dev).manual_seed(seed)
    nb = (K + 31) // 32
    if fp4:
        table = torch.tensor(FP4_VALUES, dtype=torch.int8, device=dev)
        ints = table[torch.randint(0, len(FP4_VALUES), (rows, nb * 32), generator=g, device=dev)]
    else:
        ints = torch.randint(-8, 9, (rows, nb * 32), generator=g, device=dev, dtype=torch.int8)
    j = torch.randint(BLOCK_SHIFTS[0], BLOCK_SHIFTS[-1] + 1, (rows, nb), generator=g, device=dev, dtype=torch.int8)
    c = dict(rows=rows, K=K, fp4=fp4, ints=ints[:, :K].contiguous(), j=j)
    c["W"] = weights(c)
    c["x"] = torch.randint(-8, 9, (K,), generator=g, device=dev).to(torch.bfloat16)
    c["res"] = torch.randint(-128, 129, (rows,), generator=g, device=dev).to(torch.bfloat16)
    c["xn"] = (torch.randint(0, 2, (K,), generator=g, device=dev) * 4 - 2).to(torch.bfloat16)          # |x| = 2
    c["nw"] = torch.randint(-4, 5, (K,), generator=g, device=dev).to(torch.bfloat16)
    return c


def weights(c, shift=0):
    """ints * 2^(j + shift) as bf16 (exact: at most four significant bits)."""
    rows, K = c["ints"].shape
    out = torch.empty(rows, K, dtype=torch.bfloat16, device=c["ints"].device)
    step = max(1, (1 << 26) // K)
    for r0 in range(0, rows, step):
        s = torch.exp2(c["j"][r0:r0 + step].float() + shift).repeat_interleave(32, dim=1)[:, :K]
        out[r0:r0 + step] = (c["ints"][r0:r0 + step].float() * s).to(torch.bfloat16)
    return out


def activations(c):
    """(K, 2) float64: column 0 the plain x, column 1 h = RMSNorm(xn; nw, eps = 0) = sign(xn) * nw."""
    return torch.stack([c["x"].double(), torch.sign(c["xn"].double()) * c["nw"].double()], dim=1)


def row_sums(W, acts):
    """(W @ acts, |W| @ |acts|) in float64, a block of rows at a time."""
    rows, K = W.shape
    s = torch.empty(rows, acts.shape[1], dtype=torch.float64, device=W.device)
    sa = torch.empty_like(s)
    step = max(1, (1 << 26) // K)
    for r0 in range(0, rows, step):
        Wd = W[r0:r0 + step].double()
        s[r0:r0 + step] = Wd @ acts
        sa[r0:r0 + step] = Wd.abs() @ acts.abs()
    return s, sa


def check_preconditions(c):
    """On the inputs alone: the integer ranges, |xn| = 2, and sum_k |act_k * W_nk| < 2^22 for every row and both activation vectors.
    Fills c["sums"] (rows, 2) float64, the exact dot products."""
    mag = c["ints"].abs()
    assert int(mag.max()) <= (6 if c["fp4"] else 8) and not (c["fp4"] and bool((mag == 5).any()))
    assert int(c["j"].min()) >= BLOCK_SHIFTS[0] and int(c["j"].max()) <= BLOCK_SHIFTS[-1]
    x, xn, nw, res = (c[k].double() for k in ("x", "xn", "nw", "res"))
    assert bool((x == x.round()).all()) and float(x.abs().max()) <= 8
    assert bool((xn.abs() == 2).all()) and float((xn * xn).sum()) == 4.0 * c["K"]
    assert bool((nw == nw.round()).all()) and float(nw.abs().max()) <= 4
    assert bool((res == res.round()).all()) and float(res.abs().max()) <= 128
    c["sums"], sabs = row_sums(c["W"], activations(c))
    assert float(sabs.max()) < EXACT_BOUND, f"sum |x W| reaches {float(sabs.max())}"
    assert bool((c["sums"] * 4 == (c["sums"] * 4).round()).all())
    return c


# ---- planted argmax ties ----------------------------------------------------------------------------------------------------------------
def tie_targets(m, rows, R, grid):
    """Rows that get a copy of row m, by the plan (R rows per wave, 4 waves per tile, tile t on block t % grid): a later row of the same
    wave, another wave of the same tile, a later tile of the same block, another block, the last row.  Only those that exist."""
    T = 4 * R
    tile, wave, r = m // T, (m % T) // R, m % R
    want = {"same wave": m + 1 if r < R - 1 else None,
            "other wave": tile * T + ((wave + 1) % 4) * R + r,
            "same block": m + grid * T,
            "other block": m + T if m + T < rows else m - T,
            "last row": rows - 1}
    return {k: v for k, v in want.items() if v is not None and 0 <= v < rows and v != m}


def plant_ties(c, R, grid):
    """Copies the row holding the largest logit to tie_targets' rows, for the plain and then for the normed activations (whose targets
    skip the rows the first round took; its last row is the last one still free).  Returns [{name: row}, {name: row}]."""
    planted, taken = [], set()
    for col in (0, 1):
        s, _ = row_sums(c["W"], activations(c))
        lin = bf16_rne(s[:, col])
        m = int(torch.nonzero(lin == lin.max()).flatten()[0])
        t = tie_targets(m, c["rows"], R, grid)
        if t.get("last row") in taken:
            free = [r for r in range(c["rows"] - 1, -1, -1) if r not in taken and r != m]
            t["last row"] = free[0]
        t = {k: v for k, v in t.items() if v not in taken and v != m}
        for v in t.values():
            for key in ("ints", "j", "W"):
                c[key][v] = c[key][m]
        taken |= set(t.values()) | {m}
        planted.append(dict(t, source=m))
    return planted


def make_case(rows, K, fp4=False, device="cpu", seed=0, tie_plan=None):
    """Inputs, planted ties (tie_plan = (R, grid) of the LOGITS launch), the preconditions asserted, the exact sums."""
    c = make_inputs(rows, K, fp4, device, seed)
    c["ties"] = plant_ties(c, *tie_plan) if tie_plan is not None else None
    return check_preconditions(c)


# ---- what the kernel must give ----------------------------------------------------------------------------------------------------------
def expected(c, epi, norm):
    """Float64 sums with bf16 round-to-nearest-even at the reference's op boundaries.  STORE / RESIDUAL -> bf16 (rows);
    LOGITS -> (f32 (rows), the first maximal index); PARTIAL_F32 -> f32 (rows)."""
    s = c["sums"][:, 1 if norm else 0]
    if epi == PARTIAL_F32:
        return as_f32(s)
    lin = bf16_rne(s)                                          # the Linear's output tensor
    if epi == STORE:
        return as_bf16(lin)
    if epi == RESIDUAL:
        return as_bf16(bf16_rne(c["res"].double() + lin))
    assert epi == LOGITS
    return as_f32(lin), int(torch.nonzero(lin == lin.max()).flatten()[0])


def silu_mul(gate, up):
    """bf16(bf16(silu(bf16(gate))) * bf16(up)) in float64 (a bf16 product of two bf16 values is exact in float64)."""
    lin = bf16_rne(gate)
    g = bf16_rne(lin / (1.0 + torch.exp(-lin)))
    return bf16_rne(g * bf16_rne(up))


def gate_up_rows(n_fused):
    """Row indices of the gate and of the up rows in the fused layout: 16-row blocks alternating gate / up."""
    idx = torch.arange(n_fused)
    return idx[(idx % 32) < 16], idx[(idx % 32) >= 16]


def expected_silu_fused(c, norm):
    """c's matrix read as the fused gate / up layout, scaled by 2^SILU_SHIFT -> float64 (rows / 2) of bf16 values."""
    s = c["sums"][:, 1 if norm else 0] * 2.0 ** SILU_SHIFT
    gi, ui = gate_up_rows(c["rows"])
    return silu_mul(s[gi.to(s.device)], s[ui.to(s.device)])


def expected_silu_separate(c, norm):
    """Gate matrix = c's W, up matrix = its rows rolled by one (up row n = W row n - 1), both scaled by 2^SILU_SHIFT."""
    s = c["sums"][:, 1 if norm else 0] * 2.0 ** SILU_SHIFT
    return silu_mul(s, torch.roll(s, 1, 0))


def fuse_gate_up(Wg, Wu):
    """(I, K) gate and up matrices, I % 16 == 0 -> the (2I, K) fused layout."""
    I, K = Wg.shape
    assert I % 16 == 0
    return torch.stack([Wg.reshape(I // 16, 16, K), Wu.reshape(I // 16, 16, K)], dim=1).reshape(2 * I, K).contiguous()


def tie_fraction(c):
    """The share of rows whose exact sum lies half way between two bf16 values."""
    s = c["sums"][:, 0]
    a = s.abs().contiguous().view(torch.int64)
    return float(((a & ((1 << 45) - 1)) == (1 << 44)).double().mean())


# ---- the MX encodings of these weights, written directly --------------------------------------------------------------------------------
E4M3_OF_INT = (0x00, 0x38, 0x40, 0x44, 0x48, 0x4a, 0x4c, 0x4e, 0x50)       # 0 .. 8: 2^(E - 7) * (1 + M / 8), code E << 3 | M
E2M1_OF_INT = (0, 2, 4, 5, 6, -1, 7)                                      # 0, 1, 2, 3, 4, (5 has no code), 6: the index into E2M1's grid


def encode_mxfp8(c, shift=0):
    """(q (rows, K) uint8, scales (rows, K / 32) uint8) holding ints * 2^(j + shift): each integer's E4M3 code, the block's exponent."""
    assert c["K"] % 32 == 0
    a = c["ints"].to(torch.int64)
    q = torch.tensor(E4M3_OF_INT, dtype=torch.uint8, device=a.device)[a.abs()] | ((a < 0).to(torch.uint8) << 7)
    return q.contiguous(), (c["j"].to(torch.int16) + 127 + shift).to(torch.uint8).contiguous()


def encode_mxfp4(c, shift=0):
    """(q (rows, K / 2) uint8 packed E2M1 codes, even k in the low nibble, scales (rows, K / 32) uint8)."""
    assert c["K"] % 32 == 0 and c["fp4"]
    a = c["ints"].to(torch.int64)
    code = torch.tensor(E2M1_OF_INT, dtype=torch.int16, device=a.device)[a.abs()]
    assert int(code.min()) >= 0
    code = code.to(torch.uint8) | ((a < 0).to(torch.uint8) << 3)
    q = code[:, 0::2] | (code[:, 1::2] << 4)
    return q.contiguous(), (c["j"].to(torch.int16) + 127 + shift).to(torch.uint8).contiguous()


# ---- Gaussian inputs: the f64 chain with non-trivial 1 / rms ----------------------------------------------------------------------------
def gaussian_case(rows, K, device="cpu", seed=0):
    dev = torch.device(device)
    g = torch.Generator(device=dev).manual_seed(seed)
    return dict(W=(torch.randn(rows, K, generator=g, device=dev) * 0.02).to(torch.bfloat16), x=torch.randn(K, generator=g, device=dev).to(torch.bfloat16),
                nw=(1.0 + 0.02 * torch.randn(K, generator=g, device=dev)).to(torch.bfloat16),
                res=torch.randn(rows, generator=g, device=dev).to(torch.bfloat16))


def gaussian_expected(c, norm, residual, eps):
    """bf16 values as float64: h = bf16(x / rms * nw) or x, y = bf16(W h), then bf16(res + y)."""
    x = c["x"].double()
    h = bf16_rne(x / torch.sqrt((x * x).mean() + eps) * c["nw"].double()) if norm else x
    y = bf16_rne(row_sums(c["W"], h[:, None])[0][:, 0])
    return bf16_rne(c["res"].double() + y) if residual else y
