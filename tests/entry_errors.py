"""(return code, aha_hip_last_error() text) of refused calls to the batch generation, engine submit and sample_rows entries, every one of
them refused before a model, an engine or the device is touched: the handle is null and the checks that come before it decide.
tests/golden/entry_errors_parent.json holds the table as the library gave it before the entries were folded onto one checker per family
(`python tests/entry_errors.py OUT.json`, no GPU needed); tests/test_entry_errors_cpu.py recomputes it and asserts equality, so the code,
the message, the entry name in front of it and the order of the checks all stay what they were."""
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def compute(lib=None) -> dict:
    from aha_amd import _lib
    lib = lib or _lib.lib()
    out = {}

    def rec(name, rc):
        assert name not in out, name
        assert rc < 0, f"{name}: the call was not refused (rc {rc})"
        out[name] = [int(rc), lib.aha_hip_last_error().decode()]

    SP = _lib.SamplingParams
    good = SP(0.7, 1.0, 0, 1.1, 64, 0, 5)
    bad_nan, bad_last_n = SP(float("nan"), 1.0, 0, 1.0, 64, 0, 5), SP(0.7, 1.0, 0, 1.0, -1, 0, 5)
    params = {"ok": (SP * 2)(good, good), "bad0": (SP * 2)(bad_nan, good), "bad1": (SP * 2)(good, bad_last_n), "null": None}
    MAXTOP = _lib.AHA_MAX_TOP_LOGPROBS
    tops = {"ok": np.asarray([3, -1], np.int32), "m2": np.asarray([-2, 3], np.int32), "over1": np.asarray([0, MAXTOP + 1], np.int32)}
    ids, lens = np.asarray([1, 2, 3, 4, 5], np.uint32), np.asarray([2, 3], np.uint64)
    toks, n_out = np.zeros(2 * 4, np.uint32), np.zeros(2, np.uint64)
    lp_buf = (_lib.TokenLogprobs * 8)()
    cb = _lib.TOKEN_MASK_FN(lambda *a: 0)
    cb_p = C.cast(cb, C.c_void_p)
    head = (None, ids.ctypes.data, lens.ctypes.data, 2)      # null model, two sequences
    tail = (toks.ctypes.data, n_out.ctypes.data, None)       # tokens_out, n_out, no logits

    def top_p(key):
        return None if key is None else tops[key].ctypes.data

    # entry -> call(params, top_logprobs key or None, logprobs_out or None); the entries without logprobs ignore the last two
    batch = {
        "generate_batch_sampled": lambda p, t, lp: lib.aha_hip_generate_batch_sampled(*head, p, 4, 0, *tail),
        "generate_batch_mm": lambda p, t, lp: lib.aha_hip_generate_batch_mm(*head, None, p, 4, 0, *tail),
        "generate_batch_logprobs": lambda p, t, lp: lib.aha_hip_generate_batch_logprobs(*head, None, p, top_p(t), 4, 0, *tail, lp),
        "generate_batch_adjusted": lambda p, t, lp: lib.aha_hip_generate_batch_adjusted(*head, None, p, None, top_p(t), 4, 0, *tail, lp),
        "generate_batch_masked": lambda p, t, lp: lib.aha_hip_generate_batch_masked(*head, None, p, None, top_p(t), 4, 0, cb_p, None, *tail, lp),
        "generate_batch_masked_null_fn": lambda p, t, lp: lib.aha_hip_generate_batch_masked(*head, None, p, None, top_p(t), 4, 0, None, None,
                                                                                         *tail, lp),
    }
    for name, call in batch.items():
        # _logprobs refuses a call without top_logprobs / logprobs_out: give it both where the case is about something else
        t, lp = ("ok", lp_buf) if name == "generate_batch_logprobs" else (None, None)
        rec(f"{name}/bad_params_seq0", call(params["bad0"], t, lp))
        rec(f"{name}/bad_params_seq1", call(params["bad1"], t, lp))
        rec(f"{name}/null_params", call(None, t, lp))            # refused by _sampled as such, by the others for the null model
        rec(f"{name}/null_model", call(params["ok"], t, lp))
        if name in ("generate_batch_sampled", "generate_batch_mm"):
            continue
        rec(f"{name}/top_without_out", call(params["ok"], "ok", None))
        rec(f"{name}/out_without_top", call(params["ok"], None, lp_buf))
        rec(f"{name}/top_and_out_null", call(params["ok"], None, None))
        rec(f"{name}/top_minus_2", call(params["ok"], "m2", lp_buf))
        rec(f"{name}/top_over_max_seq1", call(params["ok"], "over1", lp_buf))
        rec(f"{name}/bad_params_and_bad_top", call(params["bad1"], "m2", lp_buf))
        rec(f"{name}/bad_pairing_and_bad_top", call(params["ok"], "m2", None))
    rec("generate_batch/null_model", lib.aha_hip_generate_batch(*head, 4, 0, *tail))

    # _spec: the config, then the predictions / prediction_lens pairing, then the model
    SC = _lib.SpecConfig
    pred, plen = np.asarray([1, 2], np.uint32), np.asarray([1, 1], np.uint64)

    def spec(cfg, p, pl):
        return lib.aha_hip_generate_batch_spec(*head, 4, 0, None if cfg is None else C.byref(cfg), p, pl, *tail, None, None, None)
    rec("generate_batch_spec/null_config", spec(None, pred.ctypes.data, None))
    rec("generate_batch_spec/bad_max_draft_and_pairing", spec(SC(16, 1, 3), pred.ctypes.data, None))
    rec("generate_batch_spec/bad_ngram_and_pairing", spec(SC(4, 3, 2), None, plen.ctypes.data))
    rec("generate_batch_spec/predictions_without_lens", spec(SC(4, 1, 3), pred.ctypes.data, None))
    rec("generate_batch_spec/lens_without_predictions", spec(SC(4, 1, 3), None, plen.ctypes.data))
    rec("generate_batch_spec/null_model", spec(SC(4, 1, 3), pred.ctypes.data, plen.ctypes.data))

    # the engine's submit entries (null engine): params, then top_logprobs, then the handle
    rid = C.c_uint64()
    words = np.ones(4, np.uint32)
    eh = (None, ids.ctypes.data, 2, None)
    submit = {
        "engine_submit": lambda p, t: lib.aha_hip_engine_submit(*eh, p, 4, C.byref(rid)),
        "engine_submit_logprobs": lambda p, t: lib.aha_hip_engine_submit_logprobs(*eh, p, 4, t, C.byref(rid)),
        "engine_submit_adjusted": lambda p, t: lib.aha_hip_engine_submit_adjusted(*eh, p, None, 4, t, C.byref(rid)),
        "engine_submit_masked": lambda p, t: lib.aha_hip_engine_submit_masked(*eh, p, None, words.ctypes.data, 4, 4, t, C.byref(rid)),
    }
    for name, call in submit.items():
        rec(f"{name}/bad_params", call(C.byref(bad_nan), 0))
        rec(f"{name}/bad_params_and_bad_top", call(C.byref(bad_last_n), MAXTOP + 1))
        rec(f"{name}/top_minus_1", call(C.byref(good), -1))      # refused by _logprobs as such, by the others for the null engine
        rec(f"{name}/top_minus_2", call(C.byref(good), -2))
        rec(f"{name}/top_over_max", call(C.byref(good), MAXTOP + 1))
        rec(f"{name}/null_engine", call(C.byref(good), 0))
        rec(f"{name}/null_params_null_engine", call(None, 0))

    # sample_rows*: what is refused before any device work; the device pointers are never dereferenced
    k, t, p, off = np.asarray([1], np.int32), np.zeros(1, np.float32), np.ones(1, np.float32), np.zeros(2, np.uint64)
    fake = C.c_void_p(256)
    rows = (64, 1, 64, k.ctypes.data, t.ctypes.data, p.ctypes.data, None, off.ctypes.data)
    outs = (fake, fake, fake, None)
    mr = np.asarray([0], np.int32)
    rec("sample_rows/null_logits", lib.aha_hip_sample_rows(None, *rows, *outs))
    rec("sample_rows_adjusted/null_logits", lib.aha_hip_sample_rows_adjusted(None, *rows, None, None, off.ctypes.data, *outs))
    rec("sample_rows_adjusted/null_adj_offsets", lib.aha_hip_sample_rows_adjusted(fake, *rows, None, None, None, *outs))
    rec("sample_rows_masked/null_mask_rows", lib.aha_hip_sample_rows_masked(fake, *rows, None, None, None, None, None, *outs))
    rec("sample_rows_masked/null_mask_rows_with_masks", lib.aha_hip_sample_rows_masked(fake, *rows, None, None, None, fake, None, *outs))
    rec("sample_rows_masked/row_names_a_mask_null_masks", lib.aha_hip_sample_rows_masked(fake, *rows, None, None, None, None, mr.ctypes.data, *outs))
    rec("sample_rows_masked/row_names_a_mask_null_masks_with_adj_offsets",
        lib.aha_hip_sample_rows_masked(fake, *rows, None, None, off.ctypes.data, None, mr.ctypes.data, *outs))
    del cb
    return out


if __name__ == "__main__":
    res = compute()
    print(json.dumps(res, indent=1))
    if len(sys.argv) > 1:
        os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
        with open(sys.argv[1], "w") as f:
            json.dump(res, f, indent=1, sort_keys=True)
