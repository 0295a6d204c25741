"""-m gpu: batched Qwen3-VL generation with images and videos (aha_hip_generate_batch_mm / HipInferenceModel.generate_batch_mm) on the
tiny Qwen3-VL model (real head dims 72 / 128, ViT + DeepStack):

  * exact greedy sequences on a decisive checkpoint against generate_generic on each request alone and the oracle's free-running greedy
    sequence, with one prefill pass per request and with one pass for all;
  * every step's logits of every image request against the oracle, teacher-forced on the batch's tokens (decode positions carry the
    request's own rope_delta);
  * isolation, text requests bit-identical to generate_batch / generate_batch_sampled, sampled rows replayed with the sampler
    specification, the tower's single attention launch (tests/tools/vit_seg_attn_worker.py), errors and the model state afterwards.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from aha_amd._lib import AhaHipError
from aha_amd.configs import tiny_qwen3, tiny_qwen3vl
from aha_amd.sampling import SamplingParams
from aha_amd.weights import qwen3_text_weights, qwen3vl_weights
from oracle import qwen3 as oq
from oracle import qwen3vl as ov
from oracle import rand_stdrng as ornd
from oracle import sampling as osamp
from oracle.numerics import Numerics

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import decisive  # noqa: E402

pytestmark = pytest.mark.gpu
NM = Numerics("bf16", matmul_f64=True)
MAX_NEW = 8


def bits(x):
    return np.asarray(x, dtype=np.float32).view(np.uint32)


def rel_err(got, ref):
    ref = np.asarray(ref, dtype=np.float32).reshape(-1)
    return float(np.abs(got - ref).max()) / float(ref.std()), float(np.sqrt(((got - ref) ** 2).mean())) / float(ref.std())


def make_request(cfg, seed, img_sizes=(), vid_shapes=(), n_text=5):
    """(ids, MultiModalData or None, the oracle's mm tuple or None): images, then videos in the processor's layout, then text."""
    from aha_amd.model import MultiModalData
    from aha_amd.vision_host import image_prompt_ids, video_prompt_ids
    g = np.random.default_rng(seed)
    ids = [int(x) for x in g.integers(0, 1900, size=3)]
    if not img_sizes and not vid_shapes:
        return ids + [int(x) for x in g.integers(0, 1900, size=n_text)], None, None
    pv = grid = pvv = vgrid = None
    if img_sizes:
        pv, grid = ov.process_images(NM, [g.integers(0, 256, size=(h, w, 3), dtype=np.uint8) for (h, w) in img_sizes])
        ids = image_prompt_ids(cfg, grid, ids, [int(x) for x in g.integers(0, 1900, size=2)])
    if vid_shapes:
        pvv, vgrid = ov.process_videos(NM, [g.integers(0, 256, size=(t, h, w, 3), dtype=np.uint8) for (t, h, w) in vid_shapes])
        stamps = [[int(x) for x in g.integers(0, 1900, size=3)] for _ in range(int(vgrid[:, 0].sum()))]
        ids += video_prompt_ids(cfg, vgrid, stamps)
    ids += [int(x) for x in g.integers(0, 1900, size=n_text)]
    data = MultiModalData(pv.to(torch.bfloat16) if pv is not None else None, grid,
                          pixel_values_video=pvv.to(torch.bfloat16) if pvv is not None else None, video_grid_thw=vgrid)
    omm = (pv, grid) if pvv is None else (pv, grid, pvv, vgrid)
    return ids, data, omm


def batch(cfg):
    """Text only; one image; two images of different sizes; an image plus a video of two temporal patches; prompts on both sides of
    40 tokens."""
    return [make_request(cfg, 1, n_text=12),
            make_request(cfg, 2, [(64, 96)], n_text=9),
            make_request(cfg, 3, [(96, 160), (64, 64)], n_text=50),
            make_request(cfg, 4, [(64, 64)], [(4, 64, 64)], n_text=4),
            make_request(cfg, 5, n_text=60),
            make_request(cfg, 6, [(64, 64)], n_text=2)]


@pytest.fixture(scope="module")
def decisive_vl(gpu):
    from aha_amd.model import HipInferenceModel
    cfg = tiny_qwen3vl()
    w = qwen3vl_weights(cfg, seed=0)
    decisive.make_untied_decisive(w, "model.language_model.embed_tokens.weight", "lm_head.weight", scale=32.0, seed=7, n_text=2000)
    m = HipInferenceModel(cfg, w)
    yield cfg, w, m
    m.close()


@pytest.fixture(scope="module")
def vl(gpu):
    from aha_amd.model import HipInferenceModel
    cfg = tiny_qwen3vl()
    w = qwen3vl_weights(cfg, seed=0)
    m = HipInferenceModel(cfg, w)
    yield cfg, w, m
    m.close()


def test_generate_batch_mm_exact_greedy(decisive_vl):
    from aha_amd.model import generate_generic
    cfg, w, m = decisive_vl
    reqs = batch(cfg)
    o = ov.OracleQwen3VL(cfg, w, NM)
    want = []
    for ids, data, omm in reqs:
        o.clear_cache()
        toks, lgs = oq.greedy_generate(o, ids, MAX_NEW, mm=omm, return_logits=True)
        assert min(decisive.margin_std(lg) for lg in lgs) >= 0.5
        single = generate_generic(m, ids, MAX_NEW, data)[0]
        assert single == toks
        want.append(toks)
    prompts, datas = [r[0] for r in reqs], [r[1] for r in reqs]
    for budget in (1, 0):
        got = m.generate_batch_mm(prompts, datas, MAX_NEW, max_tokens_per_pass=budget)
        assert m.cache_len() == 0
        assert got == want, budget


def test_generate_batch_mm_logits_follow_the_oracle(vl):
    cfg, w, m = vl
    reqs = batch(cfg)
    toks, step = m.generate_batch_mm([r[0] for r in reqs], [r[1] for r in reqs], MAX_NEW, want_step_logits=True)
    o = ov.OracleQwen3VL(cfg, w, NM)
    for j, (ids, data, omm) in enumerate(reqs):
        if data is None:
            continue
        assert len(toks[j]) == MAX_NEW
        o.clear_cache()
        ref = o.forward_initial(ids, 0, omm).reshape(-1).numpy()
        off = len(ids)
        for s in range(MAX_NEW):
            if s:
                ref = o.forward_step([toks[j][s - 1]], off).reshape(-1).numpy()
                off += 1
            e_max, e_rms = rel_err(step[j, s], ref)
            assert e_max < 0.05 and e_rms < 0.02, f"request {j} step {s}: max {e_max:.4f} rms {e_rms:.4f} (in std units)"
        assert o.rope_delta < 0, j


def test_generate_batch_mm_isolation(vl):
    cfg, w, m = vl
    reqs = batch(cfg)
    a = reqs[3]
    alone, la = m.generate_batch_mm([a[0]], [a[1]], MAX_NEW, max_tokens_per_pass=1, want_step_logits=True)
    others = [a] + [reqs[1], reqs[0], reqs[2]]
    got, lg = m.generate_batch_mm([r[0] for r in others], [r[1] for r in others], MAX_NEW, max_tokens_per_pass=1, want_step_logits=True)
    assert got[0] == alone[0]
    assert np.array_equal(bits(lg[0]), bits(la[0]))
    assert m.cache_len() == 0


def test_generate_batch_mm_text_requests_equal_the_text_entries(vl):
    cfg, w, m = vl
    g = np.random.default_rng(61)
    prompts = [[int(x) for x in g.integers(0, 1900, size=n)] for n in (1, 9, 40, 64, 65, 130, 3)]
    want, wl = m.generate_batch(prompts, MAX_NEW, want_logits=True)
    for data in (None, [None] * len(prompts)):
        got, step = m.generate_batch_mm(prompts, data, MAX_NEW, want_step_logits=True)
        assert got == want
        for j in range(len(prompts)):
            assert np.array_equal(bits(step[j, len(got[j]) - 1]), bits(wl[j])), j
    params = [SamplingParams(), SamplingParams(0.6, 0.95, 20, repeat_penalty=1.1, seed=3), SamplingParams(1.0, top_p=0.9, seed=4)]
    params = [params[j % 3] for j in range(len(prompts))]
    ws, wsl = m.generate_batch_sampled(prompts, params, MAX_NEW, want_step_logits=True)
    gs, gsl = m.generate_batch_mm(prompts, None, MAX_NEW, params=params, want_step_logits=True)
    assert gs == ws
    assert np.array_equal(bits(gsl), bits(wsl))


def replay(params, toks, step_logits):
    """generate_generic's sampler on the reported step logits, in the oracle restatement; one RNG stream per sequence."""
    V = step_logits.shape[-1]
    s = osamp.get_logit_processor(params.temperature, params.top_p, params.top_k)
    rng = ornd.StdRng.seed_from_u64(params.seed)
    pen_v = 1.0 if params.repeat_penalty is None else params.repeat_penalty
    out = []
    for t in range(len(toks)):
        pen = osamp.use_repeat_penalty(pen_v, params.repeat_last_n, step_logits[t], out)
        if s.kind == "ArgMax":
            tok = int(np.argmax(pen))
        else:
            wts = osamp.final_weights(pen, s)
            if s.kind in ("TopK", "TopKThenTopP") and s.k < V:
                prs = osamp.softmax_last_dim(pen * np.float32(1.0 / s.temperature))
                keep = osamp.topk_order(prs, pen)[: s.k]
                tok = int(keep[ornd.sample_multinomial(rng, wts[keep])])
            else:
                tok = ornd.sample_multinomial(rng, wts)
        out.append(tok)
    return out


def test_generate_batch_mm_sampled_replay(vl):
    cfg, w, m = vl
    reqs = [r for r in batch(cfg) if r[1] is not None]
    mixed = [SamplingParams(), SamplingParams(0.6, 0.95, 20, repeat_penalty=1.1, seed=5), SamplingParams(1.0, top_p=0.9, seed=6)]
    params = [mixed[j % 3] for j in range(len(reqs))]
    prompts, datas = [r[0] for r in reqs], [r[1] for r in reqs]
    toks, step = m.generate_batch_mm(prompts, datas, 12, params=params, want_step_logits=True)
    greedy = m.generate_batch_mm(prompts, datas, 12)
    for j, p in enumerate(params):
        assert len(toks[j]) == 12
        assert replay(p, toks[j], step[j]) == toks[j], f"request {j} ({p}) differs from the sampler specification"
        if p.temperature is None:
            assert toks[j] == greedy[j], j
    assert m.cache_len() == 0


def test_vit_single_launch_is_bit_identical(gpu):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = {}
    for flag in ("0", "1"):
        r = subprocess.run([sys.executable, os.path.join(root, "tests", "tools", "vit_seg_attn_worker.py")],
                           env=dict(os.environ, AHA_VIT_SEG_ATTN=flag), capture_output=True, text=True, timeout=900)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
        dig = [ln.split()[1] for ln in r.stdout.splitlines() if ln.startswith("VIT_SEG_DIGEST")]
        cnt = [json.loads(ln.split(None, 1)[1]) for ln in r.stdout.splitlines() if ln.startswith("VIT_SEG_LAUNCHES")]
        assert dig and cnt, r.stdout[-2000:]
        out[flag] = (dig[0], cnt[0])
    assert out["0"][0] == out["1"][0], "the single ViT attention launch changed the tower's bits"
    c0, c1 = out["0"][1], out["1"][1]
    assert c0["forward_initial"] == c0["depth"] * c0["segments"], c0
    assert c0["batch"] == c0["depth"] * c0["batch_segments"], c0
    assert c1["forward_initial"] == c1["depth"] * (1 + 1), c1   # the small segments in one launch + the one 64-row-form segment
    assert c1["batch"] == c1["depth"] * (1 + 1), c1


def test_generate_batch_mm_errors_and_state(vl, gpu):
    from aha_amd.model import HipInferenceModel, MultiModalData
    cfg, w, m = vl
    reqs = batch(cfg)
    ids, data, _ = reqs[1]
    m.clear_cache()
    before, tok = m.forward_initial(ids, 0, data)
    before2, _ = m.forward_step(tok, len(ids))
    m.clear_cache()
    bad = list(reqs[2][0])
    bad.remove(cfg.image_token_id)
    prompts, datas = [r[0] for r in reqs], [r[1] for r in reqs]
    with pytest.raises(AhaHipError, match="sequence 2") as e:
        m.generate_batch_mm(prompts[:2] + [bad] + prompts[3:], datas, 4)
    assert e.value.code == -4   # AHA_ERR_SHAPE
    assert m.cache_len() == 0
    emb = m.vision_encode(data)
    with pytest.raises(AhaHipError, match="image_embeds") as e:
        m.generate_batch_mm([ids], [MultiModalData(image_grid_thw=data.image_grid_thw, image_embeds=emb)], 4)
    assert e.value.code == -6   # AHA_ERR_UNSUPPORTED
    assert m.cache_len() == 0
    m.generate_batch_mm(prompts, datas, 4)
    assert m.cache_len() == 0
    after, tok2 = m.forward_initial(ids, 0, data)
    after2, _ = m.forward_step(tok2, len(ids))
    m.clear_cache()
    assert np.array_equal(bits(before), bits(after)) and np.array_equal(bits(before2), bits(after2))
    tcfg = tiny_qwen3(layers=1, hidden=256, heads=2, kv_heads=1, inter=512, vocab=2048)
    t = HipInferenceModel(tcfg, qwen3_text_weights(tcfg, seed=1))
    try:
        with pytest.raises(AhaHipError, match="vision tower") as e:
            t.generate_batch_mm([[1, 2, 3], ids], [None, data], 4)
        assert e.value.code == -6
        assert t.cache_len() == 0
    finally:
        t.close()
