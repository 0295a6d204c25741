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
from typing import Tuple

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
