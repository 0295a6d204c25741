"""-m gpu: the fused decode attention after its page addresses became arithmetic (linear form), its in-block merge image was re-laid
and the new token's score reads LDS in 16- and 8-byte pieces.

  * bit for bit against the library before the change: tests/golden/attn_decode_parent_digests.json (tests/attn_decode_digests.py, run
    once on that commit on an MI355X) against the same digests recomputed here -- two head shapes x five prompt lengths, see the helper;
  * the table form (debug_scramble_pages) gives the digests of the linear run, case by case;
  * a cache that outgrows its first slab inside decode_greedy (the launch form switches between steps) gives the tokens and logits of
    the same request on a model that reserved both slabs up front;
  * clear_cache() followed by the same request gives the same digest and the linear form again (the free-list order it relies on);
  * debug_attn_decode_form() reports the form the last step launched: linear in the default cases, table when scrambled or past the
    first slab -- so the fast path cannot go unused silently.
"""
import json
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import attn_decode_digests as add  # noqa: E402

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "attn_decode_parent_digests.json")
LINEAR, TABLE = 1, 0
SLAB_TOKENS = 64 * 64   # pages per slab (model.hip) x tokens per page


@pytest.fixture(scope="module")
def linear_runs(gpu):
    """{key: (digest, form of the last step)} of every case on fresh models, computed once."""
    out = {}
    for heads, kv_heads in add.HEAD_SHAPES:
        m = add.make_model(heads, kv_heads)
        assert m.debug_attn_decode_form() == -1
        for n in add.PROMPTS:
            toks, last = add.run_case(m, n)
            out[add.key(heads, kv_heads, n)] = (add.sha(toks, last), m.debug_attn_decode_form())
        m.close()
    return out


def test_digests_match_the_parent_commit(linear_runs):
    with open(GOLDEN) as f:
        want = json.load(f)
    assert sorted(linear_runs) == sorted(want)
    diff = {k: (linear_runs[k][0][:12], want[k][:12]) for k in want if linear_runs[k][0] != want[k]}
    assert not diff, f"outputs differ from the parent commit's: {diff}"


def test_default_cases_launch_the_linear_form(linear_runs):
    assert {k: f for k, (_, f) in linear_runs.items() if f != LINEAR} == {}


@pytest.mark.parametrize("heads,kv_heads", add.HEAD_SHAPES)
def test_scrambled_pages_take_the_table_form_and_give_the_same_bits(linear_runs, heads, kv_heads):
    m = add.make_model(heads, kv_heads)
    m.debug_scramble_pages(True)
    try:
        for n in add.PROMPTS:
            toks, last = add.run_case(m, n)
            assert m.debug_attn_decode_form() == TABLE, n
            assert add.sha(toks, last) == linear_runs[add.key(heads, kv_heads, n)][0], n
    finally:
        m.close()


@pytest.mark.parametrize("heads,kv_heads", add.HEAD_SHAPES)
def test_clear_cache_and_the_same_request_again(linear_runs, heads, kv_heads):
    m = add.make_model(heads, kv_heads)
    try:
        for n in (1100, 300, 300):   # a longer request first: its pages go back to the free list and are taken again in order
            toks, last = add.run_case(m, n)
            assert m.debug_attn_decode_form() == LINEAR, n
            assert add.sha(toks, last) == linear_runs[add.key(heads, kv_heads, n)][0], n
    finally:
        m.close()


def test_second_slab_during_decode_switches_the_form_and_keeps_the_bits(gpu):
    """Prompt of SLAB_TOKENS - 6: steps 1 .. 6 append into the first slab's last page (linear form), steps 7 and 8 into the first page
    of another slab (table form)."""
    n = SLAB_TOKENS - 6
    ids = add.prompt_ids(n)
    got = {}
    for name, reserve in (("tight", SLAB_TOKENS), ("ample", 2 * SLAB_TOKENS)):
        m = add.make_model(8, 2, kv_reserve_tokens=reserve)
        try:
            _, tok = m.forward_initial(ids, 0, want_logits=False)
            toks = m.decode_greedy(tok, n, 4)
            form_a = m.debug_attn_decode_form()
            toks += m.decode_greedy(toks[-1], n + 4, 4)
            got[name] = (np.asarray([int(tok)] + toks, np.uint32), m.last_logits(), form_a, m.debug_attn_decode_form())
            assert m.cache_len() == n + 8
        finally:
            m.close()
    for name in got:
        assert got[name][2] == LINEAR and got[name][3] == TABLE, (name, got[name][2:])
    assert np.array_equal(got["tight"][0], got["ample"][0])
    assert np.array_equal(got["tight"][1].view(np.uint32), got["ample"][1].view(np.uint32))
