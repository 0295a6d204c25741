"""Draft-and-verify requests in the engine (aha_hip_engine_submit_spec), without a GPU: the four entries are wired through every layer,
the header states the event contract and the scheduler, the Python mirror of the scheduler (aha_amd/speculative.py engine_step_drafts)
gives hand-worked steps, and the submit-time checks that need no engine answer before any device work."""
import ctypes as C
import os
import re

from aha_amd.speculative import EngineRow, SpecConfig, engine_step_drafts, row_budget

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
AHA_ERR_INVALID = -1
SYMBOLS = ("aha_hip_engine_submit_spec", "aha_hip_engine_max_events", "aha_hip_engine_spec_stats", "aha_hip_engine_request_spec")


def _c_args(header, name):
    decl = re.search(r"^(?:int|size_t) %s\((.*?)\);" % name, header, re.S | re.M).group(1)
    return len([a for a in decl.split(",") if a.strip()])


def _rust_args(src, name):
    decl = re.search(r"pub fn %s\((.*?)\)" % name, src, re.S).group(1)
    return len([a for a in decl.split(",") if a.strip()])


def test_symbols_in_every_layer(hip_lib):
    from aha_amd import _lib
    header = open(os.path.join(ROOT, "include", "aha_hip.h")).read()
    src = open(os.path.join(ROOT, "rust", "aha-hip", "src", "lib.rs")).read()
    for name in SYMBOLS:
        assert hasattr(hip_lib, name), name   # exported
        n = len(_lib.SIGNATURES[name][1])
        assert _c_args(header, name) == n and _rust_args(src, name) == n, name
    assert _lib.SIGNATURES["aha_hip_engine_max_events"][0] is C.c_size_t
    for method in ("pub fn submit_spec(", "pub fn max_events(", "pub fn spec_stats(", "pub fn request_spec("):
        assert method in src, method
    from aha_amd.model import HipEngine
    for method in ("max_events", "spec_stats", "request_spec"):
        assert callable(getattr(HipEngine, method))


def test_header_states_the_event_contract_and_the_scheduler():
    header = re.sub(r"\s*\n \*\s*", " ", open(os.path.join(ROOT, "include", "aha_hip.h")).read())
    for phrase in ("up to 1 + max_draft token events in one step",
                   "consecutive and in generation order",
                   "among the decode tokens in submission order",
                   "STOP / LENGTH can only be on the last of them",
                   "tokens behind a stop token inside an accepted run are dropped",
                   "the verify row that confirmed it",
                   "extra = row_budget(R) - R",
                   "k = min(|propose(...)|, extra, max_new - t - 1)",
                   "Speculation never adds a pass over the weights",
                   "row_budget(max_running) + pending cancellations",
                   "until the next step begins",
                   "params/chat.rs:105"):
        assert phrase in header, phrase
    # the sentence tests/test_logprobs_cpu.py reads is still there
    assert "logprobs in aha_hip_generate_batch_spec" in header


def test_null_handles_and_bad_configs_answer_before_any_device_work(hip_lib):
    from aha_amd import _lib
    rid = C.c_uint64()
    ids = (C.c_uint32 * 2)(1, 2)

    def submit(spec):
        return hip_lib.aha_hip_engine_submit_spec(None, ids, 2, None, 4, spec, None, 0, C.byref(rid))

    for spec, message in ((None, b"engine_submit_spec: null spec"),
                          (_lib.SpecConfig(16, 1, 3), b"engine_submit_spec: max_draft must be in 0..15"),
                          (_lib.SpecConfig(-1, 1, 3), b"engine_submit_spec: max_draft must be in 0..15"),
                          (_lib.SpecConfig(4, 0, 3), b"n-gram bounds must satisfy 1 <= ngram_min <= ngram_max <= 8"),
                          (_lib.SpecConfig(4, 3, 2), b"n-gram bounds must satisfy 1 <= ngram_min <= ngram_max <= 8"),
                          (_lib.SpecConfig(4, 1, 9), b"n-gram bounds must satisfy 1 <= ngram_min <= ngram_max <= 8"),
                          (_lib.SpecConfig(4, 1, 3), b"engine_submit_spec: null engine")):
        assert submit(None if spec is None else C.byref(spec)) == AHA_ERR_INVALID
        assert message in hip_lib.aha_hip_last_error(), (message, hip_lib.aha_hip_last_error())
    assert hip_lib.aha_hip_engine_max_events(None) == 0
    st = _lib.SpecStats()
    assert hip_lib.aha_hip_engine_spec_stats(None, C.byref(st)) == AHA_ERR_INVALID
    n = C.c_size_t()
    assert hip_lib.aha_hip_engine_request_spec(None, 1, C.byref(n), C.byref(n)) == AHA_ERR_INVALID


# ---- the scheduler mirror against hand-worked steps --------------------------------------------------------------------------------
def _row(t, max_new, spec=None, prediction=None, prompt=(900, 901, 902)):
    """a request with t generated tokens 0 .. t-1 behind a prompt that shares no token with them"""
    return EngineRow(list(prompt) + list(range(t)), len(prompt), max_new, spec, prediction)


PRED = list(range(100))   # aligned with the generated tokens 0, 1, 2, ...: rule 1 drafts prediction[t : t + D]


def test_row_budget_at_1_32_33_requests():
    spec = SpecConfig(15, 1, 3)
    # 1 request: 31 rows to give, the request takes its 15
    assert engine_step_drafts([_row(1, 40, spec, PRED)]) == [PRED[1:16]]
    # 32 requests fill the group: nobody drafts
    assert engine_step_drafts([_row(1, 40, spec, PRED) for _ in range(32)]) == [[]] * 32
    # 33 requests: the budget is 64, 31 rows to give: 15 + 15 + 1, then nothing
    d = engine_step_drafts([_row(1, 40, spec, PRED) for _ in range(33)])
    assert [len(x) for x in d] == [15, 15, 1] + [0] * 30 and d[2] == [1]
    assert 33 + sum(len(x) for x in d) == row_budget(33) == 64


def test_cut_to_max_new():
    spec = SpecConfig(7, 1, 3)
    # t = 3 of max_new = 6: t + 1 + |draft| <= max_new leaves 2
    assert engine_step_drafts([_row(3, 6, spec, PRED)]) == [[3, 4]]
    # the step's own token is the last one: no draft
    assert engine_step_drafts([_row(5, 6, spec, PRED)]) == [[]]
    # what one request does not take stays for the next: 31 - 2 = 29 >= 7
    assert engine_step_drafts([_row(3, 6, spec, PRED), _row(2, 40, spec, PRED)]) == [[3, 4], [2, 3, 4, 5, 6, 7, 8]]


def test_grant_order_is_submission_order_among_spec_requests():
    s15, s7 = SpecConfig(15, 1, 3), SpecConfig(7, 1, 3)
    plain = _row(1, 40)
    # 4 requests, 28 rows to give: the plain request and the one with max_draft 0 take none, the first spec request 15, the second
    # the 13 that are left
    rows = [plain, _row(1, 40, s15, PRED), _row(1, 40, SpecConfig(0, 1, 3), PRED), _row(2, 40, s15, PRED)]
    d = engine_step_drafts(rows)
    assert [len(x) for x in d] == [0, 15, 0, 13] and d[3] == PRED[2:15]
    # a silent proposer (no prediction, nothing repeats) takes nothing from the requests behind it
    rows = [_row(4, 40, s7), _row(4, 40, s7, PRED)]
    assert engine_step_drafts(rows) == [[], [4, 5, 6, 7, 8, 9, 10]]
    # prompt lookup: the context repeats, no prediction needed
    q = EngineRow([5, 6, 7, 8, 5, 6], 4, 40, s7)
    assert engine_step_drafts([q]) == [[7, 8, 5, 6]]


def test_first_tokens_of_the_step_draw_on_the_event_cap():
    spec = SpecConfig(15, 1, 3)
    one = [_row(1, 40, spec, PRED)]
    # max_running 32: a step with 1 decoding request and F first tokens emits at most 32 events, so it drafts at most 32 - F - 1 rows
    assert len(engine_step_drafts(one, max_running=32, n_first=0)[0]) == 15
    assert len(engine_step_drafts(one, max_running=32, n_first=20)[0]) == 11
    assert len(engine_step_drafts(one, max_running=32, n_first=31)[0]) == 0
    # without first tokens the cut never binds: row_budget(max_running) - R >= row_budget(R) - R
    for R in (1, 5, 31, 32, 33, 64):
        rows = [_row(1, 40, spec, PRED) for _ in range(R)]
        assert engine_step_drafts(rows, max_running=64) == engine_step_drafts(rows)
