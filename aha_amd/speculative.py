"""Draft proposer of draft-and-verify greedy decoding (aha_hip_generate_batch_spec): the definition the C side must equal
(csrc/spec_host.hip, aha_hip_spec_propose; tests/test_generate_spec_cpu.py), in plain Python.

Predicted Outputs (the request's `prediction`, params/chat.rs:105) plus prompt-lookup drafting.  A draft is only ever a guess: the
verify step keeps the longest prefix greedy decoding confirms, so a wrong draft costs rows of a step, never a token."""
from __future__ import annotations

from dataclasses import dataclass
from typing import List, Optional, Sequence


@dataclass
class SpecConfig:
    """aha_spec_config: max_draft 1..15 draft tokens per sequence per step (0 = speculation off); the n-gram rules try suffix lengths
    ngram_max down to ngram_min (1 <= ngram_min <= ngram_max <= 8)."""
    max_draft: int = 7
    ngram_min: int = 1
    ngram_max: int = 3

    def check(self) -> None:
        if not 0 <= self.max_draft <= 15:
            raise ValueError("max_draft must be in 0..15")
        if not 1 <= self.ngram_min <= self.ngram_max <= 8:
            raise ValueError("n-gram bounds must satisfy 1 <= ngram_min <= ngram_max <= 8")


@dataclass
class SpecStats:
    """aha_spec_stats: decode steps, rows run over all steps, draft tokens proposed / accepted."""
    decode_steps: int
    rows: int
    proposed: int
    accepted: int


def propose(spec: SpecConfig, context: Sequence[int], n_prompt: int, prediction: Optional[Sequence[int]] = None) -> List[int]:
    """The draft for one sequence: context = prompt + generated (the first n_prompt ids are the prompt).  The first rule that yields a
    non-empty draft wins:
      1. aligned prediction: generated == prediction[:t]                      -> prediction[t : t + D]
      2. n-gram in the prediction: k = ngram_max .. ngram_min, s = c[n-k:],   the EARLIEST i with p[i:i+k] == s and i + k < len(p)
                                                                               -> p[i+k : i+k+D]
      3. prompt lookup: the same k loop over c itself,                        the LATEST i < n - k with c[i:i+k] == s
                                                                               -> c[i+k : min(i+k+D, n)]
    An empty list: no draft, the sequence runs one row."""
    spec.check()
    c = list(context)
    n, D = len(c), spec.max_draft
    if n == 0 or not 0 <= n_prompt <= n:
        raise ValueError("an empty context or n_prompt > n_context")
    if D == 0:
        return []
    p = list(prediction) if prediction is not None else []
    t = n - n_prompt
    if p:
        if t < len(p) and c[n_prompt:] == p[:t]:
            return p[t:t + D]
        for k in range(spec.ngram_max, spec.ngram_min - 1, -1):
            if k > n:
                continue
            s = c[n - k:]
            for i in range(0, len(p) - k):   # i + k < len(p)
                if p[i:i + k] == s:
                    return p[i + k:i + k + D]
    for k in range(spec.ngram_max, spec.ngram_min - 1, -1):
        if k >= n:
            continue
        s = c[n - k:]
        for i in range(n - k - 1, -1, -1):
            if c[i:i + k] == s:
                return c[i + k:min(i + k + D, n)]
    return []


def row_budget(n_active: int, group: int = 32) -> int:
    """Rows a step may have: the next multiple of the gemv_rows group at or above its unfinished sequences (speculation never adds a
    pass over the weights)."""
    return (n_active + group - 1) // group * group


@dataclass
class EngineRow:
    """One decoding request of an engine step, as the scheduler of aha_hip_engine_step sees it: context = prompt + generated (the first
    n_prompt ids are the prompt), its max_new, and for a request of aha_hip_engine_submit_spec its SpecConfig and prediction (spec None:
    a request that never drafts)."""
    context: Sequence[int]
    n_prompt: int
    max_new: int
    spec: Optional[SpecConfig] = None
    prediction: Optional[Sequence[int]] = None


def engine_step_drafts(rows: Sequence[EngineRow], max_running: int = 0, n_first: int = 0) -> List[List[int]]:
    """The draft rows of one engine decode step (include/aha_hip.h, "scheduler"), a pure function of the step's state: rows are the R
    requests that decode, in submission order.  extra = row_budget(R) - R; drafts are granted in that order among the requests with a
    spec: k = min(len(propose(...)), extra, max_new - t - 1) for a request with t tokens so far, extra -= k.  A step whose prefill gave
    n_first first tokens grants at most row_budget(max_running) - n_first - R rows (max_running 0: no such cut; none when n_first = 0).
    Returns one draft (possibly empty) per request; the step runs R + sum(len) rows."""
    R = len(rows)
    extra = row_budget(R) - R
    if max_running:
        extra = max(0, min(extra, row_budget(max_running) - n_first - R))
    out: List[List[int]] = []
    for q in rows:
        t = len(q.context) - q.n_prompt
        room = min(extra, q.max_new - t - 1)
        if q.spec is None or q.spec.max_draft == 0 or room <= 0:
            out.append([])
            continue
        d = propose(q.spec, q.context, q.n_prompt, q.prediction)[:room]
        extra -= len(d)
        out.append(d)
    return out
