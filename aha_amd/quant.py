"""MXFP8 and MXFP4 weight quantisation on the caller's side of aha_hip_model_quantize_weights: the reference quantiser in plain torch on the CPU.

OCP microscaling FP8 with E4M3 elements (include/aha_hip.h states the definition): a bf16 matrix W (N, K), K % 32 == 0, is cut into blocks
of 32 consecutive k per row.  Per block, amax = max |w|, e = the smallest integer in [-117, 120] with amax <= 448 * 2^e (an all-zero block:
-117), the scale byte is e + 127 (E8M0) and q = e4m3fn(w / 2^e), round to nearest even, one byte per element.  W' = q * 2^e has at most 4
significant bits and an exponent bf16 holds, so it is exact in bf16; |w' - w| <= max(2^-4 |w|, 2^-10 * 2^e), and quantising W' gives W'
again (the bytes may differ: a block whose amax rounded down takes e - 1 with doubled q).

The library's quantiser kernel (csrc/kernels_gemv_rows_fp8.hip) computes the same bytes; tests/test_weights_fp8_gpu.py compares the two.
Weights must be finite and below 1.9375 * 2^127 in magnitude: from there on w / 2^120 rounds to 256 and W' would be 2^128.

MXFP4 (quantize_mxfp4 / dequantize_mxfp4; include/aha_hip.h states the definition) keeps the blocks and the scale bytes and changes the
elements to OCP E2M1: the magnitudes {0, 0.5, 1, 1.5, 2, 3, 4, 6}, code = sign << 3 | index.  Per block e = the smallest integer in
[-125, 125] with amax <= 6 * 2^e (an all-zero block: -125) -- the no-saturation convention of the FP8 path above, not the OCP text's
floor(log2 amax) - 2.  With v = w / 2^e (exact) the element is the nearest code, a tie to the even code: 0.25 -> 0, 0.75 -> 1, 1.25 -> 1,
1.75 -> 2, 2.5 -> 2, 3.5 -> 4, 5 -> 4.  The sign bit is kept, so the code 0x8 (-0) occurs (the hardware conversion returns -0.0 for it, and
so does dequantize_mxfp4).  q is packed two codes to a byte: byte (n, k / 2) holds even k in bits 0..3 and odd k in bits 4..7.  The bounds
on e keep every non-zero w' = q * 2^e at 2^-126 or above and finite, and q has two significant bits, so W' is exact in bf16;
|w' - w| <= max(|w| / 4, 2^(e - 2)), and quantising W' gives W' again (the bytes may differ: a block whose amax rounded down to 3 * 2^e
takes e - 1 with doubled q).  Weights must be finite and at most 1.5 * 2^127 in magnitude: beyond it w / 2^125 rounds past 6.  The
library's kernel is csrc/kernels_gemv_rows_fp4.hip; tests/test_weights_fp4_gpu.py compares the two.  Nothing here needs a torch float4 dtype.
"""
from typing import List, Tuple

import torch

BLOCK = 32
EXP_MIN, EXP_MAX = -117, 120
E4M3_MAX = 448.0


def _blocks(W: torch.Tensor) -> torch.Tensor:
    if W.dim() != 2 or W.shape[1] % BLOCK:
        raise ValueError(f"quantize_mxfp8 wants a (N, K) matrix with K a multiple of {BLOCK}")
    if W.dtype != torch.bfloat16:
        raise ValueError("quantize_mxfp8 wants bf16 weights")
    return W.detach().cpu().float().reshape(W.shape[0], W.shape[1] // BLOCK, BLOCK)


def block_exponents(W: torch.Tensor) -> torch.Tensor:
    """(N, K / 32) int32: every block's e."""
    amax = _blocks(W).abs().amax(-1)
    if not bool(torch.isfinite(amax).all()):
        raise ValueError("quantize_mxfp8: non-finite weight")
    # amax = f * 2^x with f in [0.5, 1); 448 = 0.875 * 2^9: amax <= 448 * 2^e  <=>  e >= x - 9 (+ 1 when f > 0.875)
    f, x = torch.frexp(amax)
    e = x.to(torch.int32) - 9 + (f > 0.875).to(torch.int32)
    e = torch.where(amax == 0, torch.full_like(e, EXP_MIN), e)
    return e.clamp(EXP_MIN, EXP_MAX)


def quantize_mxfp8(W: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """W (N, K) bf16 -> (q (N, K) uint8 E4M3 codes, scales (N, K / 32) uint8 E8M0 bytes, W' (N, K) bf16), all on the CPU."""
    b = _blocks(W)
    e = block_exponents(W)
    v = b * torch.exp2(-e.float())[..., None]          # exact: a power-of-two scale (an underflow is far below E4M3's grid)
    q8 = v.to(torch.float8_e4m3fn)                     # round to nearest even; |v| <= 448: nothing saturates
    q = q8.view(torch.uint8).reshape(W.shape)
    wr = (q8.float() * torch.exp2(e.float())[..., None]).reshape(W.shape)
    wb = wr.bfloat16()
    if not bool((wb.float() == wr).all()):
        raise ValueError("quantize_mxfp8: a weight of 1.9375 * 2^127 or more in magnitude does not survive the round trip")
    return q.contiguous(), (e + 127).to(torch.uint8).contiguous(), wb.contiguous()


def dequantize_mxfp8(q: torch.Tensor, scales: torch.Tensor) -> torch.Tensor:
    """(q (N, K) uint8, scales (N, K / 32) uint8) -> W' (N, K) bf16 (exact)."""
    N, K = q.shape
    v = q.cpu().contiguous().view(torch.float8_e4m3fn).float().reshape(N, K // BLOCK, BLOCK)
    e = scales.cpu().to(torch.int32) - 127
    return (v * torch.exp2(e.float())[..., None]).reshape(N, K).bfloat16()


E2M1_GRID = (0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0)
EXP4_MIN, EXP4_MAX = -125, 125
E2M1_MAX = 6.0


def _blocks4(W: torch.Tensor) -> torch.Tensor:
    if W.dim() != 2 or W.shape[1] % BLOCK:
        raise ValueError(f"quantize_mxfp4 wants a (N, K) matrix with K a multiple of {BLOCK}")
    if W.dtype != torch.bfloat16:
        raise ValueError("quantize_mxfp4 wants bf16 weights")
    b = W.detach().cpu().double().reshape(W.shape[0], W.shape[1] // BLOCK, BLOCK)
    if not bool(torch.isfinite(b).all()):
        raise ValueError("quantize_mxfp4: non-finite weight")
    if bool((b.abs() > 1.5 * 2.0 ** 127).any()):
        raise ValueError("quantize_mxfp4: a weight above 1.5 * 2^127 in magnitude would round past 6 * 2^125")
    return b


def block_exponents_mxfp4(W: torch.Tensor) -> torch.Tensor:
    """(N, K / 32) int32: every block's MXFP4 e."""
    amax = _blocks4(W).abs().amax(-1)
    # amax = f * 2^x with f in [0.5, 1); 6 = 0.75 * 2^3: amax <= 6 * 2^e  <=>  e >= x - 3 (+ 1 when f > 0.75)
    f, x = torch.frexp(amax)
    e = x.to(torch.int32) - 3 + (f > 0.75).to(torch.int32)
    e = torch.where(amax == 0, torch.full_like(e, EXP4_MIN), e)
    return e.clamp(EXP4_MIN, EXP4_MAX)


def pack_nibbles(codes: torch.Tensor) -> torch.Tensor:
    """(N, K) uint8 codes 0..15 -> (N, K / 2) uint8: even k in bits 0..3, odd k in bits 4..7."""
    c = codes.cpu().to(torch.uint8)
    return (c[:, 0::2] | (c[:, 1::2] << 4)).contiguous()


def unpack_nibbles(q: torch.Tensor) -> torch.Tensor:
    """The inverse of pack_nibbles: (N, K / 2) uint8 -> (N, K) uint8 codes."""
    q = q.cpu()
    return torch.stack((q & 0xf, q >> 4), dim=-1).reshape(q.shape[0], -1).contiguous()


def quantize_mxfp4(W: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """W (N, K) bf16 -> (q (N, K / 2) uint8 packed E2M1 codes, scales (N, K / 32) uint8 E8M0 bytes, W' (N, K) bf16), all on the CPU."""
    b = _blocks4(W)                                     # float64: w * 2^-e and q * 2^e below are exact
    e = block_exponents_mxfp4(W)
    s = torch.exp2(e.double())[..., None]
    v = b.abs() / s
    # the index of the nearest magnitude; a value half way between two goes to the even index, so odd-to-even midpoints count as reached
    idx = ((v > 0.25).to(torch.uint8) + (v >= 0.75).to(torch.uint8) + (v > 1.25).to(torch.uint8) + (v >= 1.75).to(torch.uint8) +
           (v > 2.5).to(torch.uint8) + (v >= 3.5).to(torch.uint8) + (v > 5.0).to(torch.uint8))
    neg = torch.signbit(b)
    codes = (idx | (neg.to(torch.uint8) << 3)).reshape(W.shape)
    mag = torch.tensor(E2M1_GRID, dtype=torch.float64)[idx.long()] * s
    wr = torch.where(neg, -mag, mag).reshape(W.shape)   # -0.0 where a negative weight rounds to 0
    wb = wr.bfloat16()
    assert bool((wb.double() == wr).all())              # two significant bits, 2^-126 <= |w'| <= 6 * 2^125 or 0
    return pack_nibbles(codes), (e + 127).to(torch.uint8).contiguous(), wb.contiguous()


def dequantize_mxfp4(q: torch.Tensor, scales: torch.Tensor) -> torch.Tensor:
    """(q (N, K / 2) uint8, scales (N, K / 32) uint8) -> W' (N, K) bf16 (exact; the code 0x8 gives -0.0)."""
    codes = unpack_nibbles(q)
    N, K = codes.shape
    mag = torch.tensor(E2M1_GRID, dtype=torch.float64)[(codes & 7).long()].reshape(N, K // BLOCK, BLOCK)
    e = scales.cpu().to(torch.int32) - 127
    w = (mag * torch.exp2(e.double())[..., None]).reshape(N, K)
    return torch.where((codes & 8) != 0, -w, w).bfloat16()


def scales_to_kernel(scales: torch.Tensor) -> torch.Tensor:
    """Reference order (N, K / 32) uint8 -> the kernels' (N, ceil(K / 128)) int32 words: word (n, c) = blocks 4c .. 4c + 3 of row n, block
    4c + g in bits 8g .. 8g + 7; bytes of blocks past K are 127."""
    N, nb = scales.shape
    nc = (nb + 3) // 4
    s = torch.full((N, nc * 4), 127, dtype=torch.uint8)
    s[:, :nb] = scales.cpu()
    return s.view(torch.int32).reshape(N, nc).contiguous()   # little-endian: byte g = bits 8g .. 8g + 7


def scales_from_kernel(words: torch.Tensor, K: int) -> torch.Tensor:
    """The inverse of scales_to_kernel for a matrix with K columns."""
    N = words.shape[0]
    return words.cpu().contiguous().view(torch.uint8).reshape(N, -1)[:, :K // BLOCK].contiguous()


# ---- exact 13-bit copies (aha_amd/csrc/kernels_gemv_pk13.hip) ----------------------------------------------------------------------------
# A bf16 weight is s | E(8) | m(7).  The copy keeps the low byte (E & 1) | m and the sign, and recodes E >> 1 to a 4-bit code h with one
# base bh per matrix: h = 0 means E >> 1 == 0 (+-0, subnormals, E = 1), h = 1 .. 15 means E >> 1 == bh + h.  Nothing is rounded: unpack_pk13
# gives W back bit for bit.  The device kernels (aha_hip_pack_pk13) equal check_pk13 / pack_pk13 byte for byte.
PK13_UNIT_K = 4096        # columns of a unit: eight 512-column chunks of one row; a lane owns k = chunk * 512 + lane * 8 .. + 7 of each
PK13_UNIT_BYTES = 6656    # 4 x 1 KiB low bytes, 2 x 1 KiB codes, 512 B signs
PK13_OFF_H, PK13_OFF_S = 4096, 6144


def _bf16_bits(W: torch.Tensor) -> torch.Tensor:
    assert W.dtype == torch.bfloat16 and W.dim() == 2
    return W.contiguous().view(torch.int16).to(torch.int32) & 0xffff


def check_pk13(W: torch.Tensor) -> Tuple[int, int]:
    """(bh, bad): the base the matrix maximum gives -- max(0, max of E >> 1 over the finite weights - 15) -- and the number of weights the
    format cannot hold: Inf / NaN, and non-zero E >> 1 at or below bh (more than 30 binades below the maximum).  Pack only if bad == 0."""
    bits = _bf16_bits(W)
    e2 = (bits >> 8) & 0x7f
    nonfinite = (bits & 0x7f80) == 0x7f80
    finite_e2 = e2[~nonfinite]
    bh = max(int(finite_e2.max()) - 15, 0) if finite_e2.numel() else 0
    bad = int(nonfinite.sum()) + int((~nonfinite & (e2 != 0) & (e2 <= bh)).sum())
    return bh, bad


def pack_pk13(W: torch.Tensor, bh: int) -> torch.Tensor:
    """(N, K / 4096, 6656) uint8: per unit, lane-linear pieces --
       bytes    0 .. 4095  low bytes: piece p (1 KiB), lane l, 16 bytes = chunk 2p elements 0..7, then chunk 2p + 1 elements 0..7
       bytes 4096 .. 6143  codes: piece q (1 KiB), lane l, 4 dwords = chunks 4q .. 4q + 3; byte i of a dword = h[e = i] | h[e = i + 4] << 4
       bytes 6144 .. 6655  signs: lane l, 2 dwords; in dword w (chunks 4w .. 4w + 3) byte e & 3 holds the sign of element e of chunk c at
                           bit (c & 3) * 2 + (e >> 2)"""
    N, K = W.shape
    assert K % PK13_UNIT_K == 0 and 0 <= bh <= 112
    J = K // PK13_UNIT_K
    bits = _bf16_bits(W).reshape(N, J, 8, 64, 8)            # [row, unit, chunk, lane, element]
    lo, e2, sg = bits & 0xff, (bits >> 8) & 0x7f, bits >> 15
    h = torch.where(e2 == 0, torch.zeros_like(e2), (e2 - bh) & 15)
    a = lo.reshape(N, J, 4, 2, 64, 8).permute(0, 1, 2, 4, 3, 5).reshape(N, J, 4 * 64 * 16)
    nib = h[..., 0:4] | (h[..., 4:8] << 4)                  # [row, unit, chunk, lane, byte]
    hp = nib.reshape(N, J, 2, 4, 64, 4).permute(0, 1, 2, 4, 3, 5).reshape(N, J, 2 * 64 * 16)
    s5 = sg.reshape(N, J, 2, 4, 64, 2, 4)                   # [row, unit, dword, chunk & 3, lane, e >> 2, e & 3]
    sb = torch.zeros(N, J, 2, 64, 4, dtype=torch.int32, device=W.device)
    for cc in range(4):
        for half in range(2):
            sb |= s5[:, :, :, cc, :, half, :] << (cc * 2 + half)
    sp = sb.permute(0, 1, 3, 2, 4).reshape(N, J, 64 * 8)
    return torch.cat([a, hp, sp], dim=2).to(torch.uint8)


PK13_MAX_ROWS = 16        # rows of a matrix the matvec may read from bf16 (aha_hip_pack_pk13_rows)


def _below_window(W: torch.Tensor, bh: int) -> torch.Tensor:
    bits = _bf16_bits(W)
    e2 = (bits >> 8) & 0x7f
    return ((bits & 0x7f80) != 0x7f80) & (e2 != 0) & (e2 <= bh)


def check_pk13_rows(W: torch.Tensor) -> Tuple[int, int, List[int]]:
    """(bh, nonfinite, rows): check_pk13's base, the number of Inf / NaN, and the rows of W (ascending) that hold a finite weight below the
    window -- the exception rows the matvec reads from W itself.  Pack if nonfinite == 0 and len(rows) <= PK13_MAX_ROWS."""
    bh, _ = check_pk13(W)
    bits = _bf16_bits(W)
    nonfinite = int(((bits & 0x7f80) == 0x7f80).sum())
    rows = torch.nonzero(_below_window(W, bh).any(dim=1)).flatten().tolist()
    return bh, nonfinite, rows


def packable_pk13_rows(nonfinite: int, rows) -> bool:
    """The rule of model_pack_weights and aha_hip_pack_pk13_rows: no Inf / NaN, at most PK13_MAX_ROWS exception rows."""
    return nonfinite == 0 and len(rows) <= PK13_MAX_ROWS


def pack_pk13_rows(W: torch.Tensor, bh: int) -> torch.Tensor:
    """pack_pk13 of W with every finite weight below the window taken as +0: what the copy holds there is never used."""
    Wz = W.clone()
    Wz[_below_window(W, bh)] = 0.0
    return pack_pk13(Wz, bh)


def unpack_pk13_rows(P: torch.Tensor, bh: int, W: torch.Tensor, rows) -> torch.Tensor:
    """The matrix the matvec computes with: unpack_pk13 of the copy, the exception rows taken from W.  Equals W bit for bit."""
    out = unpack_pk13(P, bh).clone()
    for r in rows:
        out[r] = W[r]
    return out


def unpack_pk13(P: torch.Tensor, bh: int) -> torch.Tensor:
    """The bf16 matrix (N, K) a copy holds: pack_pk13's inverse, bit for bit."""
    N, J, B = P.shape
    assert B == PK13_UNIT_BYTES
    P = P.to(torch.int32)
    lo = P[:, :, :PK13_OFF_H].reshape(N, J, 4, 64, 2, 8).permute(0, 1, 2, 4, 3, 5).reshape(N, J, 8, 64, 8)
    nib = P[:, :, PK13_OFF_H:PK13_OFF_S].reshape(N, J, 2, 64, 4, 4).permute(0, 1, 2, 4, 3, 5).reshape(N, J, 8, 64, 4)
    h = torch.cat([nib & 15, nib >> 4], dim=-1)
    sb = P[:, :, PK13_OFF_S:].reshape(N, J, 64, 2, 4).permute(0, 1, 3, 2, 4)       # [row, unit, dword, lane, e & 3]
    sg = torch.zeros(N, J, 2, 4, 64, 2, 4, dtype=torch.int32)
    for cc in range(4):
        for half in range(2):
            sg[:, :, :, cc, :, half, :] = (sb >> (cc * 2 + half)) & 1
    sg = sg.reshape(N, J, 8, 64, 8)
    e2 = torch.where(h == 0, torch.zeros_like(h), h + bh)
    bits = (sg << 15) | (e2 << 8) | lo
    return bits.reshape(N, J * PK13_UNIT_K).to(torch.int16).view(torch.bfloat16)
