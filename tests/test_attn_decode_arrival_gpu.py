"""-m gpu: the fused decode attention after its splits were put in reverse dispatch order, the new token's score moved in front of the
page loop and the final merge of up to 16 splits lost its LDS pass (aha_amd/csrc/attn_decode_body.h, kernels_attn.hip).  All three
only move when and where the same operations are issued, so every output bit must stay.

  * bit for bit against the library before the change: tests/golden/attn_decode_arrival_parent_digests.json holds the digests of
    tests/attn_decode_digests.py's two-layer tiny models (heads / kv heads 4 / 2 and 8 / 2), forward_initial + decode_greedy(.., 8),
    computed once on the parent commit on an MI355X, at the split counts the older golden does not reach (its cases stop at 5):
      prompt 1600:  26 pages, 7 splits (the count of the benchmark's step); the eight steps stay inside 26 pages;
      prompt 3900:  61 - 62 pages, 16 splits: the upper edge of the final merge's register path;
      prompt 4200:  66 pages, 17 splits: the path through LDS; the cache has outgrown its first slab of 64 pages: the table form.
    (one block per 4 pages; the model's cap of 64 splits is not reached.)
  * debug_attn_decode_form() reports the linear form for 1600 and 3900 and the table form for 4200;
  * 1600 with debug_scramble_pages(True) -- the table form at 7 splits -- gives the digest of the linear run.
"""
import json
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import attn_decode_digests as add  # noqa: E402

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "attn_decode_arrival_parent_digests.json")
LINEAR, TABLE = 1, 0
PROMPTS = (1600, 3900, 4200)
FORMS = {1600: LINEAR, 3900: LINEAR, 4200: TABLE}


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def models(gpu):
    ms = {hs: add.make_model(*hs) for hs in add.HEAD_SHAPES}
    yield ms
    for m in ms.values():
        m.close()


def test_golden_holds_exactly_these_cases(golden):
    assert sorted(golden) == sorted(add.key(h, k, n) for h, k in add.HEAD_SHAPES for n in PROMPTS)


@pytest.mark.parametrize("n_prompt", PROMPTS)
@pytest.mark.parametrize("heads,kv_heads", add.HEAD_SHAPES)
def test_digest_matches_the_parent_commit(models, golden, heads, kv_heads, n_prompt):
    m = models[(heads, kv_heads)]
    toks, last = add.run_case(m, n_prompt)
    assert m.debug_attn_decode_form() == FORMS[n_prompt]
    assert m.cache_len() == n_prompt + add.STEPS
    assert add.sha(toks, last) == golden[add.key(heads, kv_heads, n_prompt)]


@pytest.mark.parametrize("heads,kv_heads", add.HEAD_SHAPES)
def test_scrambled_pages_at_seven_splits_give_the_same_bits(golden, gpu, heads, kv_heads):
    m = add.make_model(heads, kv_heads)
    m.debug_scramble_pages(True)   # before the first slab exists: its pages are handed out in a shuffled order
    try:
        toks, last = add.run_case(m, 1600)
        assert m.debug_attn_decode_form() == TABLE
        assert add.sha(toks, last) == golden[add.key(heads, kv_heads, 1600)]
    finally:
        m.close()
