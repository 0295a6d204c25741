"""-m gpu: the decode matvec and the fused decode attention after their prologue inputs, the first weight tile and the first KV page
became unconditional requests from clamped indices (aha_amd/csrc/gemv_body.h, attn_decode_body.h).  Requests moved, no arithmetic did:
every output bit must be the parent commit's.  tests/golden/decode_prologue_parent_digests.json holds the parent's digests (computed
once on an MI355X) of the cases of tests/decode_prologue_digests.py -- the shapes at which a clamped request differs from the
conditional one it replaces, which the older goldens do not reach: fewer rows than a tile, a ragged last tile, a K tail, K beyond the
preloaded range; cache lengths 1 (no old page), 2, 64, 65 (the append opens a page) and 257 (a whole block without a page), both head
shapes, table and linear form.
"""
import json
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import decode_prologue_digests as dpd  # noqa: E402

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "decode_prologue_parent_digests.json")


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def models(gpu):
    ms = {hs: dpd.make_model(*hs) for hs in dpd.HEAD_SHAPES}
    yield ms
    for m in ms.values():
        m.close()


def test_golden_holds_exactly_these_cases(golden):
    want = [dpd.gemv_key(N, K, n, e) for N, K in dpd.GEMV_SHAPES for n in (False, True) for e in ("store", "residual", "silu_mul")]
    want += [dpd.attn_key(f, h, k, L) for f in (dpd.LINEAR, dpd.TABLE) for h, k in dpd.HEAD_SHAPES for L in dpd.CACHE_LENS]
    assert sorted(golden) == sorted(want)


@pytest.mark.parametrize("N,K", dpd.GEMV_SHAPES)
def test_matvec_digests_match_the_parent_commit(gpu, golden, N, K):
    got = dpd.gemv_case(N, K)
    assert len(got) == 6
    assert {k: golden[k] for k in got} == got


@pytest.mark.parametrize("L", dpd.CACHE_LENS)
@pytest.mark.parametrize("heads,kv_heads", dpd.HEAD_SHAPES)
def test_table_form_digest_matches_the_parent_commit(gpu, golden, heads, kv_heads, L):
    assert dpd.attn_table_case(heads, kv_heads, L) == golden[dpd.attn_key(dpd.TABLE, heads, kv_heads, L)]


@pytest.mark.parametrize("L", dpd.CACHE_LENS)
@pytest.mark.parametrize("heads,kv_heads", dpd.HEAD_SHAPES)
def test_linear_form_digest_matches_the_parent_commit(models, golden, heads, kv_heads, L):
    dig, form, n = dpd.attn_linear_case(models[(heads, kv_heads)], L)
    assert form == dpd.LINEAR and n == L
    assert dig == golden[dpd.attn_key(dpd.LINEAR, heads, kv_heads, L)]
