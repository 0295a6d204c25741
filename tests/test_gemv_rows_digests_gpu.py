"""GPU tier: gemv_rows in its three weight forms (bf16, MXFP8, MXFP4) and the library's two MX quantisers give, bit for bit, what the
library gave while the three matvec kernels were separate texts (tests/gemv_rows_digests.py; tests/golden/gemv_rows_parent_digests.json
was recorded on an MI355X).  The MX-equals-bf16 tests compare the shared body with itself; this one holds the body to its past."""
import json
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gemv_rows_digests  # noqa: E402

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gemv_rows_parent_digests.json")


def test_matvec_forms_and_quantisers_match_the_parent_digests(gpu):
    with open(GOLDEN) as f:
        want = json.load(f)
    got = gemv_rows_digests.compute()
    assert sorted(got) == sorted(want)
    for name in sorted(want):
        assert got[name] == want[name], name
    # what the table must cover: four forms x four shapes x four row counts x the epilogues (no SiLU.mul for N = 40), two quantisers x
    # two matrices
    forms = ("bf16_on_mxfp8", "bf16_on_mxfp4", "mxfp8", "mxfp4")
    n = 0
    for N, K in gemv_rows_digests.SHAPES:
        for R in gemv_rows_digests.ROWS:
            for epi in gemv_rows_digests.EPILOGUES:
                if epi == "silu_mul" and N % 32:
                    continue
                for form in forms:
                    assert len(want[f"{form}/{N}x{K}/R{R}/{epi}"]) == 64
                    n += 1
                # each MX form equals the bf16 form on its own W'
                assert want[f"mxfp8/{N}x{K}/R{R}/{epi}"] == want[f"bf16_on_mxfp8/{N}x{K}/R{R}/{epi}"]
                assert want[f"mxfp4/{N}x{K}/R{R}/{epi}"] == want[f"bf16_on_mxfp4/{N}x{K}/R{R}/{epi}"]
    assert n == 4 * (4 * 4 * 4 - 4)
    for fmt in ("mxfp8", "mxfp4"):
        for N, K in gemv_rows_digests.QUANTISER_SHAPES:
            assert len(want[f"quantize_{fmt}/{N}x{K}"]) == 64
    assert len(want) == n + 4
