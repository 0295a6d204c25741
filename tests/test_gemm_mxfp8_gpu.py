"""-m gpu: the MXFP8 prefill GEMM (aha_hip_gemm_mxfp8, v_mfma_scale_f32_16x16x128_f8f6f4) and its activation row quantiser at op level.

1. Exact: E4M3 codes of integers in [-7, 7] and block exponents in {-1, 0, 1} on both sides make every product a multiple of 2^-2 below
   2^10 units, so for K <= 1024 every partial sum is below 2^20 units and exact in f32 in any order: the kernel must equal the f64 product
   of the dequantised operands rounded to bf16, bit for bit.  One 256 x 128 tile kernel ships (3 LDS stages), so the ragged sizes are
   M in {1, 17, 255, 257} and N in {16, 112, 144, 272} (tile - 16, tile + 16: N is a multiple of 16), K = one step, two, stages + 1, 8.
   dense=False keeps one nonzero block per row (the scale-association probe: a lane reading a neighbour's scale byte fails it).
2. Random data: errors against the f64 product pushed through the epilogue in f64, at most 2 x those of the bf16 ops.gemm on the same
   (bf16-exact) dequantised operands.  The gate+up epilogue needs N % 32 == 0, so it runs at N = 288, not 272.
3. ops.quantize_mxfp8_rows equals quant.quantize_mxfp8 byte for byte.
"""
import pytest
import torch

from aha_amd import _lib

pytestmark = pytest.mark.gpu

TILE_M, TILE_N, STAGES = 256, 128, 3


def bf16_bits(t):
    return t.contiguous().view(torch.int16)


def exact_operand(rows, K, seed, dense):
    """(codes (rows, K) uint8, scales (rows, K / 32) uint8): integers in [-7, 7] as E4M3, block exponents in {-1, 0, 1}."""
    g = torch.Generator().manual_seed(seed)
    v = torch.randint(-7, 8, (rows, K), generator=g).float()
    if not dense:
        blk = torch.arange(K)[None, :] // 32 == (torch.arange(rows)[:, None] % (K // 32))
        v = v * blk
    s = (torch.randint(-1, 2, (rows, K // 32), generator=g) + 127).to(torch.uint8)
    return v.to(torch.float8_e4m3fn).view(torch.uint8), s


@pytest.mark.parametrize("dense", [False, True])
@pytest.mark.parametrize("K", [128, 256, 128 * (STAGES + 1), 1024])
@pytest.mark.parametrize("N", [16, TILE_N - 16, TILE_N + 16, 272])
@pytest.mark.parametrize("M", [1, 17, TILE_M - 1, TILE_M + 1])
def test_exact_products_bit_for_bit(gpu, M, N, K, dense):
    from aha_amd import ops, quant
    (aq, sa), (wq, sw) = exact_operand(M, K, 1000 + M + K, dense), exact_operand(N, K, 2000 + N + K, dense)
    want = (quant.dequantize_mxfp8(aq, sa).double() @ quant.dequantize_mxfp8(wq, sw).double().T).float().bfloat16()
    dev = [t.to(gpu) for t in (aq, sa, wq, sw)]
    got = ops.gemm_mxfp8(*dev)
    assert torch.equal(bf16_bits(got.cpu()), bf16_bits(want))
    res = torch.randint(-8, 9, (M, N), generator=torch.Generator().manual_seed(M + N)).bfloat16()
    out = res.to(gpu)
    ops.gemm_mxfp8(*dev, residual=out, out=out)   # the residual aliases C
    assert torch.equal(bf16_bits(out.cpu()), bf16_bits((want.double() + res.double()).float().bfloat16()))
    assert ops.plan_gemm_mxfp8(M, N, K) == (TILE_M, TILE_N, -(-M // TILE_M) * -(-N // TILE_N), STAGES)


@pytest.mark.parametrize("act,N", [(_lib.ACT_NONE, 272), (_lib.ACT_SILU_MUL_PAIRS, 288)])
def test_random_data_against_f64(gpu, act, N):
    from aha_amd import ops, quant
    M, K = 257, 1024
    g = torch.Generator().manual_seed(5)
    A = (torch.randn(M, K, generator=g) * torch.exp2(torch.randint(-3, 4, (M, 1), generator=g).float())).bfloat16().to(gpu)
    W = (torch.randn(N, K, generator=g) * torch.exp2(torch.randint(-3, 4, (N, 1), generator=g).float()) * 0.03).bfloat16().to(gpu)
    aq, sa = ops.quantize_mxfp8_rows(A)
    wq, sw, _ = ops.quantize_mxfp8(W)
    Ad, Wd = quant.dequantize_mxfp8(aq.cpu(), sa.cpu()), quant.dequantize_mxfp8(wq.cpu(), sw.cpu())
    ref = Ad.double() @ Wd.double().T
    if act == _lib.ACT_SILU_MUL_PAIRS:   # 16 gate rows, then their 16 up rows
        p = ref.reshape(M, N // 32, 2, 16)
        ref = (p[:, :, 0] * torch.sigmoid(p[:, :, 0]) * p[:, :, 1]).reshape(M, N // 2)
    err = {}
    for name, got in (("fp8", ops.gemm_mxfp8(aq, sa, wq, sw, act=act)), ("bf16", ops.gemm(Ad.to(gpu), Wd.to(gpu), act=act))):
        d = got.cpu().double() - ref
        err[name] = (float(d.abs().max()), float(d.pow(2).mean().sqrt()))
    print(f"act {act}: max / rms error against f64: fp8 {err['fp8']}, bf16 {err['bf16']}")
    assert err["fp8"][0] <= 2 * err["bf16"][0] and err["fp8"][1] <= 2 * err["bf16"][1], err


@pytest.mark.parametrize("K", [128, 1152])
@pytest.mark.parametrize("M", [1, 5, 130])
def test_row_quantiser_equals_reference(gpu, M, K):
    from aha_amd import ops, quant
    g = torch.Generator().manual_seed(M + K)
    wide = (torch.randn(M, K + 64, generator=g) * torch.exp2(torch.randint(-12, 6, (M, 1), generator=g).float())).bfloat16()
    A = wide[:, 8:8 + K]                                  # strided rows: lda = K + 64
    A[0, 0:32] = 0.0                                      # an all-zero block
    A[0, 32:64] = 0.0
    A[0, 33] = 1e-39                                      # a bf16 subnormal alone in its block
    A[M - 1, 64:96] = torch.tensor([448.0, 17.0, 19.0, -21.0] * 8).bfloat16()   # e = 0; 17, 19, 21 are ties of the step-2 grid
    A[M - 1, 96] = torch.tensor([0x7f77], dtype=torch.int16).view(torch.bfloat16)[0]   # just under the limit
    q, s, _ = quant.quantize_mxfp8(A.contiguous())
    gq, gs = ops.quantize_mxfp8_rows(wide.to(gpu)[:, 8:8 + K])
    assert torch.equal(gs.cpu(), s) and torch.equal(gq.cpu(), q)
