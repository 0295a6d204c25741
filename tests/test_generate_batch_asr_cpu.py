"""CPU tier: batched Qwen3-ASR generation -- aha_hip_logmel_batch is wired through every layer (header, export, ctypes table, Rust shim,
ops), its argument checks and generate_batch_mm's run before any device work, and sampling.generate_asr_batch applies the ASR loop's own
rules (qwen3_asr/generate.rs:130-186) to the batch's rows: a fake model stands in for the library."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_logmel_batch_in_every_layer(hip_lib):
    from aha_amd import _lib, ops
    header = open(os.path.join(ROOT, "include", "aha_hip.h")).read()
    assert re.search(r"int aha_hip_logmel_batch\(const float\* samples, const int64_t\* n_samples, size_t n_clips, float\* out, "
                     r"void\* stream\);", header)
    assert hasattr(hip_lib, "aha_hip_logmel_batch")
    assert len(_lib.SIGNATURES["aha_hip_logmel_batch"][1]) == 5
    src = open(os.path.join(ROOT, "rust", "aha-hip", "src", "lib.rs")).read()
    ext = src[src.index('extern "C" {'):]
    ext = ext[:ext.index("\n    }\n")]
    assert re.search(r"pub fn aha_hip_logmel_batch\(\s*samples: \*const f32,\s*n_samples: \*const i64,\s*n_clips: usize,"
                     r"\s*out: \*mut f32,\s*stream: \*mut std::ffi::c_void,?\s*\) -> i32;", ext)
    assert re.search(r"pub unsafe fn logmel_batch\(", src)
    assert callable(ops.logmel_batch)


def test_logmel_batch_argument_checks_before_device_work(hip_lib):
    """Null pointers, no clips and a clip of at most 400 samples are refused before anything touches a device (this machine may have
    none): the pointers below are never dereferenced."""
    from aha_amd import _lib
    lib = _lib.lib()
    fake = C.c_void_p(16)
    n_ok = np.asarray([16000, 8000], dtype=np.int64)
    assert lib.aha_hip_logmel_batch(None, n_ok.ctypes.data, 2, fake, None) == -1
    assert lib.aha_hip_logmel_batch(fake, None, 2, fake, None) == -1
    assert lib.aha_hip_logmel_batch(fake, n_ok.ctypes.data, 0, fake, None) == -1
    assert lib.aha_hip_logmel_batch(fake, n_ok.ctypes.data, 2, None, None) == -1
    n_bad = np.asarray([16000, 400], dtype=np.int64)
    assert lib.aha_hip_logmel_batch(fake, n_bad.ctypes.data, 2, fake, None) == -1
    assert b"clip 1" in lib.aha_hip_last_error()


def test_generate_batch_mm_docstrings_mention_audio():
    from aha_amd import model
    assert "audio" in model.HipInferenceModel.generate_batch_mm.__doc__
    header = open(os.path.join(ROOT, "include", "aha_hip.h")).read()
    assert "audio input is not supported" not in header


# ---- generate_asr_batch's host rules on a fake model ------------------------------------------------------------------------------
STOPS = [90, 91, 92]   # the ASR loop stops on the first two only; the batch on all three


class FakeAsr:
    """Each prompt's first id picks a scripted token stream.  forward_initial / forward_step walk it (generate_asr's serial loop);
    generate_batch_mm mirrors the library's rule: the first token never stops a row, later any stop id does, or max_new."""

    class text_cfg:
        vocab_size = 128

    def __init__(self, scripts):
        self.scripts = scripts
        self.batch_calls = []
        self.serial_prompts = []
        self._cur = None

    def stop_token_ids(self):
        return list(STOPS)

    def forward_initial(self, ids, offset, data=None, want_logits=True):
        self.serial_prompts.append(list(ids))
        self._cur = iter(self.scripts[ids[0]])
        return None, next(self._cur)

    def forward_step(self, tok, offset, want_logits=True):
        return None, next(self._cur)

    def clear_cache(self):
        self._cur = None

    def generate_batch_mm(self, prompts, data, max_new, params=None, max_tokens_per_pass=0, want_step_logits=False):
        self.batch_calls.append(([list(p) for p in prompts], list(data), max_new, params))
        out = []
        for p in prompts:
            s = self.scripts[p[0]]
            row = [s[0]]
            while len(row) < max_new:
                row.append(s[len(row)])
                if row[-1] in STOPS:
                    break
            out.append(row)
        return out


def _chunk(key, n):
    return ([key] + [5] * (n - 1), f"clip{key}")


def test_generate_asr_batch_host_rules_greedy():
    from aha_amd import sampling as hs
    scripts = {
        1: [90, 3, 4, 5, 6, 7, 8, 9],          # eos as the FIRST token: cut there (the batch row goes on)
        2: [3, 4, 92, 5, 91, 6, 7, 8],         # the batch stops on the third stop id: the chunk runs again on its own
        3: [3, 4, 5, 6, 7, 8, 9, 10],          # max_tokens
        4: [6, 91, 7, 8, 9, 10, 11, 12],       # a regular eos
        5: [7, 7, 90, 1, 1, 1, 1, 1],
    }
    m = FakeAsr(scripts)
    reqs = [[_chunk(1, 4)], [_chunk(2, 7), _chunk(3, 3)], [_chunk(4, 5), _chunk(5, 2), _chunk(1, 9)]]
    got = hs.generate_asr_batch(m, reqs, temperature=0.0, max_tokens=6)
    assert len(m.batch_calls) == 1
    prompts, data, max_new, params = m.batch_calls[0]
    assert max_new == 6 and params is None
    assert [p[0] for p in prompts] == [1, 2, 3, 4, 5, 1] and data == ["clip1", "clip2", "clip3", "clip4", "clip5", "clip1"]
    assert [p[0] for p in m.serial_prompts] == [2]          # only the chunk the batch ended on the third stop id
    want = []
    for chunks in reqs:
        ref = FakeAsr(scripts)
        want.append(hs.generate_asr(ref, chunks, temperature=0.0, max_tokens=6))
    assert got == want
    assert got[0] == ([90], 4)
    assert got[1] == ([3, 4, 92, 5, 91] + [3, 4, 5, 6, 7, 8], 10)
    assert got[2] == ([6, 91] + [7, 7, 90] + [90], 16)


def test_generate_asr_batch_sampled_rules(monkeypatch):
    """Sampled: a single-chunk request rides the batch with SamplingParams(temperature, top_p, top_k None, penalty 1, seed); a multi-chunk
    request runs serially through generate_asr (its chunks share one RNG stream there)."""
    from aha_amd import sampling as hs
    scripts = {1: [3, 90, 0, 0], 2: [4, 4, 91, 0], 3: [5, 5, 5, 5]}
    m = FakeAsr(scripts)
    serial = []

    def fake_generate_asr(model, chunks, temperature, top_p=None, seed=34562, max_tokens=1024):
        serial.append(([c[1] for c in chunks], temperature, top_p, seed, max_tokens))
        return [77] * len(chunks), sum(len(c[0]) for c in chunks)

    monkeypatch.setattr(hs, "generate_asr", fake_generate_asr)
    reqs = [[_chunk(1, 3)], [_chunk(2, 2), _chunk(3, 4)], [_chunk(3, 5)]]
    got = hs.generate_asr_batch(m, reqs, temperature=0.7, top_p=0.9, seed=11, max_tokens=4)
    assert serial == [(["clip2", "clip3"], 0.7, 0.9, 11, 4)]
    prompts, data, max_new, params = m.batch_calls[0]
    assert [p[0] for p in prompts] == [1, 3] and max_new == 4
    assert isinstance(params, hs.SamplingParams)
    assert params.temperature == pytest.approx(0.7) and params.top_p == pytest.approx(0.9) and params.top_k is None
    assert params.repeat_penalty in (None, 1.0) and params.seed == 11
    assert got == [([3, 90], 3), ([77, 77], 6), ([5, 5, 5, 5], 5)]


def test_generate_asr_batch_empty():
    from aha_amd import sampling as hs
    m = FakeAsr({})
    assert hs.generate_asr_batch(m, [], temperature=0.0) == []
    assert hs.generate_asr_batch(m, [[]], temperature=0.0) == [([], 0)]
    assert m.batch_calls == []
