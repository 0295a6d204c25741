"""GPU tier: every path through the prefill layer stack (forward_initial fresh and continued, the 64-row attention form with q not
fused, embed, embed_batch across passes, Qwen3-VL with DeepStack in both stacks, Qwen3-ASR, context parallel, tensor parallel in both
modes, the engine's chunked prefill) gives the logits, tokens, hidden rows and per-class launch / byte / FLOP sums the library gave
before the stack, the decode row table and the packed-pass setup were each folded into one copy (tests/prefill_digests.py;
tests/golden/prefill_stack_parent_digests.json was recorded on an MI355X from the library before that change)."""
import json
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import prefill_digests  # noqa: E402

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "prefill_stack_parent_digests.json")

CASES = ["forward_initial/1", "forward_initial/5", "forward_initial/64", "forward_initial/65", "forward_initial/130", "continuation",
         "q_not_fused", "embed", "embed_batch", "embed_batch/one_pass", "vl/forward_initial", "vl/generate_batch_mm", "asr/forward_initial",
         "engine_chunked"]
RANK_CASES = ["cp/one_launch", "cp/launcher_fallback", "tp/allreduce", "tp/seq_parallel"]


def test_prefill_stack_matches_the_parent_digests(gpu):
    with open(GOLDEN) as f:
        want = json.load(f)
    got = prefill_digests.compute()
    assert sorted(got) == sorted(want)
    for name in sorted(want):
        assert got[name] == want[name], name
    # what the table must cover: a digest and the five classes' sums per case (per rank for the sharded ones)
    names = CASES + [f"{c}/rank{r}" for c in RANK_CASES for r in range(2)]
    assert sorted(want) == sorted(names + [n + "/profile" for n in names])
    for n in names:
        assert len(want[n]) == 64, n
        assert set(want[n + "/profile"]) == set(prefill_digests.CLASSES), n
        for c in prefill_digests.CLASSES:
            assert set(want[n + "/profile"][c]) == {"launches", "bytes", "flops"}
    layers = 2
    for n in (5, 64, 65, 130):
        p = want[f"forward_initial/{n}/profile"]
        assert p["gemm"]["launches"] >= 4 * layers and p["attn_prefill"]["launches"] == layers and p["gemv_rows"]["launches"] == 0
    assert want["forward_initial/1/profile"]["gemm"]["launches"] == 0            # the step path
    assert want["embed_batch/profile"]["attn_prefill"]["launches"] == 2 * layers   # two passes
    assert want["embed_batch/one_pass/profile"]["attn_prefill"]["launches"] == layers
    assert want["vl/generate_batch_mm/profile"]["attn_decode_batch"]["launches"] > 0 and want["vl/generate_batch_mm/profile"]["gemv_rows"]["launches"] > 0
    assert want["engine_chunked/profile"]["attn_prefill"]["launches"] == 4 * layers   # 200 tokens in chunks of 64
    assert want["engine_chunked/profile"]["attn_decode_batch"]["launches"] > 0
    for r in range(2):   # a rank's two chunks in one attention call per layer
        assert want[f"cp/one_launch/rank{r}/profile"]["attn_prefill"]["launches"] == layers
    assert want["tp/allreduce/rank0"] == want["tp/allreduce/rank1"] == want["tp/seq_parallel/rank0"] == want["tp/seq_parallel/rank1"]
    assert want["cp/one_launch/rank0"] == want["cp/one_launch/rank1"]
