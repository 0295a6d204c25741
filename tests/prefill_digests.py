"""Output digests and profile sums of every path through the prefill layer stack, the batched decode step's row table and the packed
prefill pass of the generation entries.  tests/golden/prefill_stack_parent_digests.json holds them as computed by the library before
the two copies of the prefill layer, the three row-table writers and the two packed-pass setups were folded into one each
(`python tests/prefill_digests.py OUT.json` on an MI355X); tests/test_prefill_stack_gpu.py recomputes them and asserts equality.

Per case: a sha256 over the returned logits / tokens / hidden rows, and with profiling on the launches, bytes and FLOPs of the classes
gemm, attn_prefill, elem, gemv_rows and attn_decode_batch (get_profile is visible behaviour: no launch gained, lost or re-accounted)."""
import hashlib
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

CLASSES = ("gemm", "attn_prefill", "elem", "gemv_rows", "attn_decode_batch")


def sha(*arrays) -> str:
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def flat(toks):
    return np.asarray([t for row in toks for t in row], np.uint32), np.asarray([len(row) for row in toks], np.uint64)


def profile_of(m) -> dict:
    """The profile sums, exactly: bytes and FLOPs are sums of integer-valued doubles far below 2^53 (any other value goes down as the
    double's hex form)."""
    def exact(x):
        return int(x) if x == int(x) else float(x).hex()
    out = {}
    for c in CLASSES:
        p = m.get_profile(c)
        out[c] = {"launches": int(p["launches"]), "bytes": exact(p["bytes"]), "flops": exact(p["flops"])}
    return out


def profiled(out, name, m, fn):
    m.set_profiling(False)
    m.set_profiling(True)
    res = fn()
    out[name + "/profile"] = profile_of(m)
    m.set_profiling(False)
    return res


def rnd_ids(seed, n, hi):
    return [int(x) for x in np.random.default_rng(seed).integers(0, hi, size=n)]


def text_cases(out):
    from aha_amd.configs import tiny_qwen3
    from aha_amd.model import HipEngine, HipInferenceModel
    from aha_amd.weights import qwen3_text_weights
    cfg = tiny_qwen3(layers=2, hidden=256, heads=4, kv_heads=2, inter=512, vocab=1024)
    w = qwen3_text_weights(cfg, seed=11)
    V = cfg.vocab_size
    m = HipInferenceModel(cfg, w)
    # forward_initial into a fresh cache at the page boundaries (length 1 delegates to the step path)
    for n in (1, 5, 64, 65, 130):
        m.clear_cache()
        lg, tok = profiled(out, f"forward_initial/{n}", m, lambda: m.forward_initial(rnd_ids(100 + n, n, V), 0))
        out[f"forward_initial/{n}"] = sha(lg, np.uint32(tok))
    # continuation: the cache holds the 130-token prompt (kv_off > 0), then two steps

    def cont():
        a, t0 = m.forward_initial(rnd_ids(7, 70, V), 130)
        b, t1 = m.forward_step(t0, 200)
        c, t2 = m.forward_step(t1, 201)
        return sha(a, b, c, np.asarray([t0, t1, t2], np.uint32))
    out["continuation"] = profiled(out, "continuation", m, cont)
    m.clear_cache()
    # embed (hidden_only) and embed_batch (the packed pass) over the same texts; 140 tokens per pass: {5, 64} | {130}
    texts = [rnd_ids(200 + n, n, V) for n in (5, 64, 130)]
    out["embed"] = sha(*profiled(out, "embed", m, lambda: [m.embed_one(t) for t in texts]))
    out["embed_batch"] = sha(profiled(out, "embed_batch", m, lambda: m.embed_batch(texts, max_tokens_per_pass=140)))
    out["embed_batch/one_pass"] = sha(profiled(out, "embed_batch/one_pass", m, lambda: m.embed_batch(texts)))
    # the engine's chunked prefill: 200 tokens in 64-token chunks (a step budget of 100 tokens) beside a 5-token prompt
    eng = HipEngine(m, max_running=4, kv_pages=16, max_tokens_per_step=100)
    try:
        def run():
            rids = [eng.submit(rnd_ids(31, 200, V), 4), eng.submit(rnd_ids(32, 5, V), 4)]
            evs, lgs = [], []
            for _ in range(16):
                if all(eng.finished(r) for r in rids):
                    break
                e, lg_ = eng.step(want_logits=True)
                evs += [(ev.req_id - rids[0], ev.token, ev.first, ev.stop, ev.length, ev.cancelled) for ev in e]
                lgs.append(lg_)
            assert all(eng.finished(r) for r in rids)
            # the long prompt's first token comes with its fourth chunk; the short one's came with the first
            firsts = [i for i, ev in enumerate(evs) if ev[2]]
            assert [evs[i][0] for i in firsts] == [1, 0] and firsts[1] >= 3, evs
            return sha(np.asarray(evs, np.int64), np.concatenate(lgs), *flat([eng.tokens(r) for r in rids]))
        out["engine_chunked"] = profiled(out, "engine_chunked", m, run)
    finally:
        eng.close()
    m.close()


def unfused_case(out):
    """32 / 8 heads, 2900 tokens: ceil(2900 / 256) * 32 = 384 blocks of 256 rows x heads, the threshold of the 64-row causal attention
    form (kernels_attn.hip attn_prefill_form), which does not norm and rotate Q itself: the rope kernel handles the q heads too."""
    from aha_amd.configs import tiny_qwen3
    from aha_amd.model import HipInferenceModel
    from aha_amd.weights import qwen3_text_weights
    S, heads, kvh, layers, H = 2900, 32, 8, 2, 256
    assert -(-S // 256) * heads >= 384 > -(-2816 // 256) * heads
    cfg = tiny_qwen3(layers=layers, hidden=H, heads=heads, kv_heads=kvh, inter=512, vocab=1024)
    m = HipInferenceModel(cfg, qwen3_text_weights(cfg, seed=12))
    lg, tok = profiled(out, "q_not_fused", m, lambda: m.forward_initial(rnd_ids(40, S, cfg.vocab_size), 0))
    # the rope launches carried the q heads: embedding gather + first norm + per layer S * (nq + 2 nkv) * 4 bytes; with q fused the class
    # would hold layers * S * nq * 4 bytes less
    nq, nkv = heads * 128, kvh * 128
    assert out["q_not_fused/profile"]["elem"]["bytes"] >= 2 * S * H * 4 + layers * S * (nq + 2 * nkv) * 4
    out["q_not_fused"] = sha(lg, np.uint32(tok))
    m.close()


def vl_case(out):
    from aha_amd.configs import tiny_qwen3vl
    from aha_amd.model import HipInferenceModel, MultiModalData
    from aha_amd.weights import qwen3vl_weights
    from tests.test_vl_gpu import make_request
    cfg = tiny_qwen3vl()
    m = HipInferenceModel(cfg, qwen3vl_weights(cfg, seed=0))
    _, pv, grid, ids = make_request(cfg, [(96, 160)], 9, 11)
    data = MultiModalData(pv.to(torch.bfloat16), grid)
    lg, tok = profiled(out, "vl/forward_initial", m, lambda: m.forward_initial(ids, 0, data))
    out["vl/forward_initial"] = sha(lg, np.uint32(tok))
    m.clear_cache()
    text = rnd_ids(50, 40, 1900)
    toks, step = profiled(out, "vl/generate_batch_mm", m, lambda: m.generate_batch_mm([ids, text], [data, None], 4, want_step_logits=True))
    out["vl/generate_batch_mm"] = sha(*flat(toks), step)
    m.close()


def asr_case(out):
    from aha_amd.configs import tiny_qwen3_asr
    from aha_amd.model import HipInferenceModel
    from aha_amd.weights import qwen3_asr_weights
    from tests.test_generate_batch_asr_gpu import audio_request
    cfg = tiny_qwen3_asr()
    m = HipInferenceModel(cfg, qwen3_asr_weights(cfg, seed=0))
    ids, data, _ = audio_request(cfg, 40000, 12)
    lg, tok = profiled(out, "asr/forward_initial", m, lambda: m.forward_initial(ids, 0, data))
    out["asr/forward_initial"] = sha(lg, np.uint32(tok))
    m.close()


def cp_cases(out):
    """Context parallel, two ranks on the one GPU (the callback gather of tests/test_cp_gpu.py), S = 1100: a rank's two chunks go out as
    ONE attention call per layer (AttnPrefillArgs::S2), which with 16 / 8 heads is one kernel launch and with 4 / 2 heads the
    launcher's two-launch fallback."""
    from aha_amd import ops
    from aha_amd.configs import tiny_qwen3
    from aha_amd.weights import qwen3_text_weights
    from tests.test_cp_gpu import Gather, make_ranks
    from tests.test_tp_gpu import run_ranks
    S = 1100
    old = os.environ.get("AHA_CP_MIN_ROWS")
    os.environ["AHA_CP_MIN_ROWS"] = "64"
    ops.gemm_plan(256, 1)
    try:
        for name, heads, kvh in (("cp/one_launch", 16, 8), ("cp/launcher_fallback", 4, 2)):
            cfg = tiny_qwen3(layers=2, hidden=256, heads=heads, kv_heads=kvh, inter=512, vocab=1024)
            w = qwen3_text_weights(cfg, seed=13)
            ids = rnd_ids(S, S, cfg.vocab_size)
            g = Gather(2)
            ranks = make_ranks(cfg, w, 2, g)
            for m in ranks:
                m.set_profiling(True)
            got = run_ranks([lambda m=m: m.forward_initial(ids, 0) for m in ranks])
            assert g.calls == cfg.num_hidden_layers + 1
            for r, m in enumerate(ranks):
                out[f"{name}/rank{r}"] = sha(got[r][0], np.uint32(got[r][1]))
                out[f"{name}/rank{r}/profile"] = profile_of(m)
                m.close()
    finally:
        ops.gemm_plan(0, 0)
        if old is None:
            del os.environ["AHA_CP_MIN_ROWS"]
        else:
            os.environ["AHA_CP_MIN_ROWS"] = old


def tp_cases(out):
    """Tensor parallel, two ranks on the one GPU (the in-process sum of tests/test_tp_gpu.py), S = 300: the all-reduce mode and the
    sequence-parallel mode (reduce-scatter / all-gather around the norms: the spr > 0 branch)."""
    from aha_amd.configs import tiny_qwen3
    from aha_amd.model import HipInferenceModel
    from aha_amd.weights import qwen3_text_weights
    from tests.test_tp_gpu import TwoRankSum, run_ranks
    cfg = tiny_qwen3()
    w = qwen3_text_weights(cfg, seed=0)
    S = 300
    ids = rnd_ids(S, S, cfg.vocab_size)
    for name, sp in (("tp/allreduce", False), ("tp/seq_parallel", True)):
        red = TwoRankSum()
        ranks = [HipInferenceModel(cfg, w, tp_rank=r, tp_size=2, allreduce=lambda p, n, r=r: red.allreduce(r, p, n),
                                   reduce_scatter=(lambda p, n, r=r: red.reduce_scatter(r, p, n)) if sp else None,
                                   all_gather=(lambda p, n, r=r: red.all_gather(r, p, n)) if sp else None) for r in range(2)]
        for m in ranks:
            m.set_profiling(True)
        got = run_ranks([lambda m=m: m.forward_initial(ids, 0) for m in ranks])
        assert (getattr(red, "rs_calls", 0) > 0) == sp
        step = run_ranks([lambda m=m: m.forward_step(got[0][1], S)[0].copy() for m in ranks])
        for r, m in enumerate(ranks):
            out[f"{name}/rank{r}"] = sha(got[r][0], np.uint32(got[r][1]), step[r])
            out[f"{name}/rank{r}/profile"] = profile_of(m)
            m.close()


def compute() -> dict:
    out = {}
    text_cases(out)
    unfused_case(out)
    vl_case(out)
    asr_case(out)
    cp_cases(out)
    tp_cases(out)
    return out


if __name__ == "__main__":
    res = compute()
    print(json.dumps(res, indent=1))
    if len(sys.argv) > 1:
        os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
        with open(sys.argv[1], "w") as f:
            json.dump(res, f, indent=1, sort_keys=True)
