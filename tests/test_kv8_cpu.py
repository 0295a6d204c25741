"""The KV8 reference quantiser (aha_amd/quant.py quantize_kv: one 128-dim vector = 128 E4M3 codes + one E8M0 scale byte) against a scalar
restatement of the format's definition, and the page layout's pack / unpack."""
import math

import pytest
import torch

from aha_amd import quant

# value of every non-negative finite E4M3 code: normal 2^(ex - 7) * (1 + man / 8), subnormal man * 2^-9
GRID = [(2.0 ** ((b >> 3) - 7) * (1 + (b & 7) / 8)) if b >> 3 else (b & 7) * 2.0 ** -9 for b in range(0x7f)]


def scalar_quantize(vals):
    """Finite Python floats (bf16 values; every step below is exact in doubles) -> (codes, scale byte)."""
    amax = max(abs(v) for v in vals)
    e = -117
    while amax > 448 * 2.0 ** e:      # the smallest e in [-117, 120] with amax <= 448 * 2^e
        e += 1
    codes = []
    for v in vals:
        x = abs(v) / 2.0 ** e
        b = min(range(0x7f), key=lambda c: (abs(GRID[c] - x), c & 1))   # nearest code, a tie to the even one
        codes.append(b | (0x80 if math.copysign(1.0, v) < 0 else 0))
    return codes, e + 127


def vectors():
    g = torch.Generator().manual_seed(3)
    rows = [torch.randn(128, generator=g) * 2.0 ** s for s in range(-20, 21, 5)]        # magnitudes 2^-20 .. 2^20
    rows.append(torch.zeros(128))                                                       # an all-zero block
    r = torch.randn(128, generator=g)
    r[::3] = 0.0                                                                        # zeros inside a block, one of them negative
    r[3] = -0.0
    rows.append(r)
    # amax = 448 exactly (e = 0): E4M3 ties 17 (16 | 18), 19 (18 | 20), 2^-10 (0 | 2^-9), 3 * 2^-10, and 27.5 / 28.5 that are no ties
    rows.append(torch.tensor([448.0, 17.0, -19.0, 2.0 ** -10, -3 * 2.0 ** -10, 27.5, 28.5, 2.0 ** -11] + [1.0] * 120))
    rows.append(torch.tensor([450.0] + [0.5] * 127))                                    # the next bf16 above 448: e = 1
    rows.append(torch.tensor([-448.0 * 2.0 ** 7] + [13.0] * 127))                       # on the saturation edge of e = 7
    return torch.stack(rows).to(torch.bfloat16)


def test_quantize_kv_against_the_scalar_restatement():
    x = vectors()
    q, s = quant.quantize_kv(x)
    for i in range(x.shape[0]):
        codes, sb = scalar_quantize(x[i].double().tolist())
        assert int(s[i]) == sb, f"vector {i}: scale byte {int(s[i])}, expected {sb}"
        assert q[i].tolist() == codes, f"vector {i}: codes differ"
    deq = quant.dequantize_kv(q, s)
    exact = torch.tensor(GRID, dtype=torch.float64)[(q & 0x7f).long()] * torch.exp2(s.double() - 127)[:, None]
    assert torch.equal(deq.double().abs(), exact), "the dequantised values are not exact in bf16"
    assert torch.equal(deq.view(torch.int16) < 0, q >= 0x80)


def test_quantize_kv_saturates_and_keeps_nan():
    x = torch.ones(2, 128, dtype=torch.bfloat16)
    x[0, 0], x[0, 1], x[0, 2] = float("inf"), float("-inf"), float("nan")
    x[1, 0] = float("nan")
    q, s = quant.quantize_kv(x)
    assert q[0, :3].tolist() == [0x7e, 0xfe, 0x7f] and int(s[0]) == 247 and int(q[0, 3]) == 0      # 1 / 2^120 is below the grid
    assert int(q[1, 0]) == 0x7f and q[1, 1:].tolist() == quant.quantize_kv(torch.ones(1, 128, dtype=torch.bfloat16))[0][0, 1:].tolist()


@pytest.mark.parametrize("kvh", [1, 2, 8])
def test_pack_unpack_round_trip(kvh):
    g = torch.Generator().manual_seed(kvh)
    kq, vq = (torch.randint(0, 256, (3, 64, kvh, 128), generator=g, dtype=torch.uint8) for _ in range(2))
    ks, vs = (torch.randint(0, 256, (3, 64, kvh), generator=g, dtype=torch.uint8) for _ in range(2))
    pages = quant.pack_kv8_pages(kq, ks, vq, vs)
    assert pages.shape == (3, 16512 * kvh)
    idx = torch.cat([i.flatten() for i in quant._kv8_index(kvh)])
    assert torch.equal(idx.sort().values, torch.arange(16512 * kvh)), "the layout is not a bijection onto the page"
    for got, want in zip(quant.unpack_kv8_pages(pages, kvh), (kq, ks, vq, vs)):
        assert torch.equal(got, want)
