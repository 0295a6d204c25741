"""-m gpu: bench.py end to end on the tiny workload -- the plain run (setup, warmup, the timed steps) and the --full run compute the
same timed steps, and --dump-outputs writes what those steps computed."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run_bench(out_dir, *extra):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--workload", "tiny", "--steps", "6", "--warmup", "2",
           "--dump-outputs", str(out_dir), *extra]
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


def test_plain_and_full_runs_dump_the_same_timed_steps(gpu, tmp_path):
    from aha_amd.configs import tiny_qwen3
    vocab = tiny_qwen3(layers=2, hidden=512, heads=4, kv_heads=2, inter=1024, vocab=2048).vocab_size
    plain = run_bench(tmp_path / "plain")
    full = run_bench(tmp_path / "full", "--full", "--no-cpu-baseline")
    for j in (plain, full):
        assert j["steps"] == 6 and j["warmup"] == 2 and j["ms_per_step"] > 0 and j["unit"] == "tokens/s" and j["dtype"] == "bf16"
        assert abs(j["value"] - 1e3 / j["ms_per_step"]) / j["value"] < 0.01     # tokens/s of one rank = 1 / seconds per step
    assert "roofline" not in plain and "prefill_tok_s" not in plain     # the plain run measures the headline figure only
    assert "roofline" in full and full["prefill_tok_s"] > 0
    got = {}
    for name in ("plain", "full"):
        tok = np.load(tmp_path / name / "tokens.npy")
        lg = np.load(tmp_path / name / "logits.npy")
        assert tok.dtype == np.float64 and tok.shape == (6,) and lg.dtype == np.float32 and lg.shape == (vocab,)
        assert np.all(tok == np.round(tok)) and tok.min() >= 0 and tok.max() < vocab and np.isfinite(lg).all()
        assert int(np.argmax(lg)) == int(tok[-1])                        # greedy: the last step's token is its logits' argmax
        got[name] = (tok, lg)
    # one prefill (plain) or four (full, timed) before the steps: the same cache, the same tokens and logits bit for bit
    assert np.array_equal(got["plain"][0], got["full"][0]) and np.array_equal(got["plain"][1], got["full"][1])
