"""CPU tier: every refusal of the generate_batch* / engine_submit* / sample_rows* entries that is decided before a model, an engine or the
device is touched keeps its return code and its aha_hip_last_error() text byte for byte -- the entry name in front of the message and the
order of the checks included (tests/entry_errors.py; the table was recorded before the entries shared one checker per family)."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import entry_errors  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "entry_errors_parent.json")


def test_refusals_match_the_parent_table(hip_lib):
    with open(GOLDEN) as f:
        want = json.load(f)
    got = entry_errors.compute(hip_lib)
    assert sorted(got) == sorted(want)
    for name in want:
        assert got[name] == want[name], name
    assert got == want


def test_the_table_says_what_the_entries_promise(hip_lib):
    """The recorded table itself: the prefixes and the order of checks that callers rely on."""
    with open(GOLDEN) as f:
        t = json.load(f)
    assert len(t) >= 90
    for name, (rc, msg) in t.items():
        assert rc < 0 and msg, name
    # parameters before the model handle; which entry names the message
    assert t["generate_batch_sampled/null_params"][1] == "generate_batch_sampled: null params"
    for e in ("mm", "logprobs", "adjusted", "masked", "masked_null_fn"):
        assert t[f"generate_batch_{e}/null_params"][1] == "null model"
        assert t[f"generate_batch_{e}/null_model"][1] == "null model"
    for e in ("sampled", "mm", "logprobs", "adjusted", "masked"):
        assert t[f"generate_batch_{e}/bad_params_seq0"][1].startswith(f"generate_batch_{e}: params of sequence 0: ")
        assert t[f"generate_batch_{e}/bad_params_seq1"][1].startswith(f"generate_batch_{e}: params of sequence 1: ")
    for e in ("logprobs", "adjusted", "masked"):
        assert t[f"generate_batch_{e}/bad_params_and_bad_top"][1].startswith(f"generate_batch_{e}: params of sequence 1: ")
        assert t[f"generate_batch_{e}/bad_pairing_and_bad_top"][1].startswith(f"generate_batch_{e}: ") and "top_logprobs of" not in \
            t[f"generate_batch_{e}/bad_pairing_and_bad_top"][1]
        assert t[f"generate_batch_{e}/top_over_max_seq1"][1].startswith(f"generate_batch_{e}: top_logprobs of sequence 1 ")
    # _logprobs wants both, _adjusted / _masked both or neither
    assert t["generate_batch_logprobs/top_and_out_null"][1] == "generate_batch_logprobs: null top_logprobs / logprobs_out"
    assert t["generate_batch_adjusted/top_and_out_null"][1] == "null model" and t["generate_batch_masked/top_and_out_null"][1] == "null model"
    # a null mask_fn is exactly _adjusted, prefix included
    for case in ("bad_params_seq0", "top_without_out", "out_without_top", "top_minus_2"):
        assert t[f"generate_batch_masked_null_fn/{case}"] == t[f"generate_batch_adjusted/{case}"], case
        assert t[f"generate_batch_masked_null_fn/{case}"][1].startswith("generate_batch_adjusted: ")
    # _spec: the config first
    assert t["generate_batch_spec/bad_max_draft_and_pairing"][1].startswith("generate_batch_spec: max_draft")
    assert "prediction_lens" in t["generate_batch_spec/predictions_without_lens"][1]
    assert t["generate_batch_spec/null_model"][1] == "null model"
    # the engine: -1 is refused by _logprobs alone
    assert t["engine_submit_logprobs/top_minus_1"][1].startswith("engine_submit_logprobs: top_logprobs must be 0 .. ")
    for e in ("engine_submit", "engine_submit_adjusted", "engine_submit_masked"):
        assert t[f"{e}/top_minus_1"][1] == f"{e}: null engine"
    for e in ("engine_submit_logprobs", "engine_submit_adjusted", "engine_submit_masked"):
        assert t[f"{e}/bad_params_and_bad_top"][1].startswith(f"{e}: params: ")
        assert t[f"{e}/top_over_max"][1].startswith(f"{e}: top_logprobs must be ") and t[f"{e}/top_over_max"][1].endswith(", got 21")
    assert t["sample_rows_adjusted/null_adj_offsets"][1] == "sample_rows_adjusted: null adj_offsets"
    assert t["sample_rows_masked/null_mask_rows"][1] == "sample_rows_masked: null mask_rows"
    assert t["sample_rows_masked/row_names_a_mask_null_masks"][1].startswith("sample_rows_masked: row 0 ")
