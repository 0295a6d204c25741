"""GPU tier: every batch generation entry and the engine's four submit entries, each through its own Python method, give the tokens,
logits, logprob structs, launch counts and model-level refusals the library gave before the entries shared one options struct and one
implementation (tests/gen_entry_digests.py; tests/golden/gen_entries_parent_digests.json was recorded on an MI355X)."""
import json
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gen_entry_digests  # noqa: E402

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gen_entries_parent_digests.json")


def test_entries_match_the_parent_digests(gpu):
    with open(GOLDEN) as f:
        want = json.load(f)
    got = gen_entry_digests.compute()
    assert sorted(got) == sorted(want)
    for name in want:
        assert got[name] == want[name], name
    # what the table must cover: the seven entries and the engine, their launch counts, and the refusals that need a model
    for e in ("generate_batch", "generate_batch_sampled", "generate_batch_mm", "generate_batch_logprobs", "generate_batch_adjusted",
              "generate_batch_masked", "generate_batch_spec", "engine"):
        assert len(want[e]) == 64 and set(want[e + "/launches"]) == set(gen_entry_digests.CLASSES), e
        assert want[e + "/launches"]["gemv_rows"] > 0
    assert want["generate_batch_logprobs/launches"]["logprob_rows_stage1"] > 0 and want["generate_batch_sampled/launches"]["sample_rows_stage1"] > 0
    for e in ("generate_batch", "generate_batch_sampled", "generate_batch_mm", "generate_batch_logprobs", "generate_batch_adjusted",
              "generate_batch_masked", "generate_batch_spec"):
        assert "generate_batch: empty batch" in want[f"refused/{e}/n_seqs_0"][1]
        assert "generate_batch: max_new must be at least 1" in want[f"refused/{e}/max_new_0"][1]
        assert "token id out of range in sequence 1 at position 2" in want[f"refused/{e}/id_at_vocab"][1]
    for e in ("generate_batch_adjusted", "generate_batch_masked"):
        assert "generate_batch_adjusted: adjust of sequence 1: " in want[f"refused/{e}/bias_id_at_vocab"][1]
    for e in ("engine_submit_adjusted", "engine_submit_masked"):
        assert "engine_submit_adjusted: adjust: " in want[f"refused/{e}/bias_id_at_vocab"][1]
    assert "engine_submit_masked: the mask has 31 words" in want["refused/engine_submit_masked/wrong_word_count"][1]
    assert "generate_batch_masked: the mask callback" in want["refused/generate_batch_masked/callback_returns_minus_3"][1]
    assert want["refused/generate_batch_masked/callback_returns_minus_3"][0] == want["refused/generate_batch/engine_owns_the_cache"][0] == -7
