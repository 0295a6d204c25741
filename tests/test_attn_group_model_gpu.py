"""-m gpu: the group attention inside the model (aha_hip_debug_rows_group / HipInferenceModel.debug_rows_group): generate_batch_spec and an
engine request that drafts give the bits they give with the switch at 0, the group kernel is launched once per layer in every step with
drafts and only there, and the split-arrival counters stand where later steps expect them (a plain request in the same engine slot)."""
import os
import sys

import numpy as np
import pytest

from aha_amd.speculative import SpecConfig

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_engine_spec_gpu import Req, drive  # noqa: E402
from test_generate_spec_gpu import prompts_for, tied_weights  # noqa: E402

pytestmark = pytest.mark.gpu
CLASSES = ("kv_append_rows", "attn_decode_group", "attn_decode_batch")


@pytest.fixture(scope="module")
def tied(gpu):
    """the decisive tied Qwen3 of the spec tests: 3 layers, g = 2"""
    from aha_amd.model import HipInferenceModel
    cfg, w = tied_weights()
    m = HipInferenceModel(cfg, w)
    yield cfg, m
    m.close()


def predictions(truth, vocab):
    """fully right, every other token wrong, fully wrong"""
    wrong = [[(t + 1) % vocab for t in o] for o in truth]
    return {"right": truth, "half": [[w if i % 2 else t for i, (t, w) in enumerate(zip(o, ow))] for o, ow in zip(truth, wrong)], "wrong": wrong}


def profiled(m, fn):
    m.set_profiling(False)
    m.set_profiling(True)
    out = fn()
    prof = {k: m.get_profile(k)["launches"] for k in CLASSES}
    m.set_profiling(False)
    return out, prof


@pytest.mark.parametrize("kind", ["right", "half", "wrong"])
def test_generate_batch_spec_keeps_its_bits(tied, kind):
    """Prompts of 60 and 250 tokens: the runs cross a page (64) and the 1 -> 2 split change (256), where a run is cut into two groups."""
    cfg, m = tied
    L = cfg.num_hidden_layers
    prompts, max_new = prompts_for([60, 250, 7], 81, 2000), 24
    pred = predictions(m.generate_batch(prompts, max_new), cfg.vocab_size)[kind]
    try:
        for D in (3, 15):
            spec = SpecConfig(D, 1, 3)
            m.debug_rows_group(0)
            (base, lb, _), prof0 = profiled(m, lambda: m.generate_batch_spec(prompts, max_new, spec, pred, want_logits=True, want_stats=True))
            assert prof0["attn_decode_group"] == 0
            m.debug_rows_group(2)
            (got, lg, info), prof = profiled(m, lambda: m.generate_batch_spec(prompts, max_new, spec, pred, want_logits=True, want_stats=True))
            assert got == base, f"max_draft {D}: tokens differ from the switch at 0"
            assert np.array_equal(lg.view(np.uint32), lb.view(np.uint32)), f"max_draft {D}: logits differ from the switch at 0"
            draft_steps = prof["kv_append_rows"] // L
            assert draft_steps > 0 and prof["kv_append_rows"] == prof0["kv_append_rows"]
            assert prof["attn_decode_group"] == L * draft_steps, prof
            assert prof["attn_decode_batch"] == L * (info["stats"].decode_steps - draft_steps), prof
    finally:
        m.debug_rows_group(0)


def test_engine_request_keeps_its_bits_and_the_slot_its_counters(tied):
    """One request that drafts (its prompt of 250 tokens crosses the split change), then a plain request in the same slot (max_running 1):
    the second request's split merge runs on the counters the grouped steps left behind."""
    cfg, m = tied
    prompts = prompts_for([250, 300], 82, 2000)
    truth = m.generate_batch(prompts, 24)
    runs = {}
    try:
        for on in (0, 2):
            m.debug_rows_group(on)
            for kind, pred in predictions(truth[:1], cfg.vocab_size).items():
                reqs = [Req(prompts[0], 24, SpecConfig(7, 1, 3), pred[0]), Req(prompts[1], 24)]
                (out, _, _), prof = profiled(m, lambda: drive(m, reqs, max_running=1, kv_pages=8))
                assert [out[i]["toks"] for i in (0, 1)] == truth, (on, kind)
                assert (prof["attn_decode_group"] > 0) == (on == 2) and prof["attn_decode_group"] in (0, prof["kv_append_rows"])
                runs[on, kind] = out
        for kind in ("right", "half", "wrong"):
            for i in (0, 1):
                a, b = runs[0, kind][i]["lg"], runs[2, kind][i]["lg"]
                assert len(a) == len(b) and all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(a, b)), (kind, i)
    finally:
        m.debug_rows_group(0)
