"""-m gpu: batched Qwen3-ASR generation with audio clips (aha_hip_generate_batch_mm / HipInferenceModel.generate_batch_mm,
sampling.generate_asr_batch) on the tiny Qwen3-ASR model (real head dims: 64 in the audio encoder, 128 in the thinker):

  * exact greedy sequences on a decisive checkpoint against the oracle's free-running greedy sequence, serial forward_initial +
    forward_step of each request, and the batch with one prefill pass per request and with one pass for all;
  * every step's logits of every audio request against the oracle, teacher-forced on the batch's tokens;
  * isolation across clips, the single-clip path unchanged bit for bit (digests recorded before the batched tower,
    tests/golden/asr_single_clip_digests.json), the batched log-mel against the one-clip op, launch counts of one tower pass,
    errors and the model state afterwards, sampled rows replayed with the sampler specification.
"""
import hashlib
import json
import os
import sys

import numpy as np
import pytest
import torch

from aha_amd._lib import AhaHipError
from aha_amd.configs import tiny_qwen3, tiny_qwen3_asr
from aha_amd.sampling import SamplingParams
from aha_amd.weights import qwen3_asr_weights, qwen3_text_weights
from oracle import qwen3 as oq
from oracle import qwen3_asr as oa
from oracle import rand_stdrng as ornd
from oracle import sampling as osamp
from oracle.numerics import Numerics

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import decisive  # noqa: E402

pytestmark = pytest.mark.gpu
NM = Numerics("bf16", matmul_f64=True)
MAX_NEW = 8
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "asr_single_clip_digests.json")


def synth_audio(n, seed):
    """BASELINE.md section 4 cfg 4: N(0, 0.1^2) clipped to [-1, 1], 16 kHz."""
    return np.clip(np.random.default_rng(seed).normal(0, 0.1, n), -1, 1).astype(np.float32)


def make_ids(cfg, n_audio_tok, seed, n_pre=5, n_post=7):
    g = np.random.default_rng(seed)
    pre = [int(x) for x in g.integers(0, 1900, size=n_pre)]
    post = [int(x) for x in g.integers(0, 1900, size=n_post)]
    return pre + [cfg.audio_start_token_id] + [cfg.audio_token_id] * n_audio_tok + [cfg.audio_end_token_id] + post


def rel_err(got, ref):
    ref = np.asarray(ref, dtype=np.float32).reshape(-1)
    return float(np.abs(got - ref).max()) / float(ref.std()), float(np.sqrt(((got - ref) ** 2).mean())) / float(ref.std())


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a, dtype=np.float32).tobytes()).hexdigest()


def audio_request(cfg, n_samples, seed, as_features=False, n_post=7):
    """(ids, MultiModalData, the oracle's features): a clip of n_samples seeded samples, given as samples or as host features."""
    from aha_amd.model import MultiModalData
    wave = synth_audio(n_samples, seed)
    feats = oa.log_mel(wave)
    ids = make_ids(cfg, oa.get_feat_extract_output_lengths(feats.shape[1]), seed, n_post=n_post)
    data = MultiModalData(audio_features=feats) if as_features else MultiModalData(audio_samples=wave)
    return ids, data, torch.from_numpy(feats)


def batch(cfg, all_features=False):
    """Clips of 0.6 s (one partial window), 2.5 s and 7.3 s (partial last windows) as samples, 4.0 s (whole windows) as features, a
    text-only request; prompts on both sides of 40 tokens."""
    g = np.random.default_rng(99)
    return [audio_request(cfg, 9600, 11, all_features, n_post=3),
            audio_request(cfg, 40000, 12, all_features),
            audio_request(cfg, 64000, 13, True, n_post=30),
            ([int(x) for x in g.integers(0, 1900, size=12)], None, None),
            audio_request(cfg, 116800, 14, all_features)]


@pytest.fixture(scope="module")
def decisive_asr(gpu):
    from aha_amd.model import HipInferenceModel
    cfg = tiny_qwen3_asr()
    w = qwen3_asr_weights(cfg, seed=0)
    decisive.make_tied_decisive(w, "thinker.model.embed_tokens.weight", "thinker.model.norm.weight", scale=32.0, seed=7, n_text=2000)
    m = HipInferenceModel(cfg, w)
    yield cfg, w, m
    m.close()


@pytest.fixture(scope="module")
def asr(gpu):
    from aha_amd.model import HipInferenceModel
    cfg = tiny_qwen3_asr()
    w = qwen3_asr_weights(cfg, seed=0)
    m = HipInferenceModel(cfg, w)
    yield cfg, w, m
    m.close()


def serial_greedy(m, ids, data, n):
    m.clear_cache()
    _, tok = m.forward_initial(ids, 0, data, want_logits=False)
    toks, off = [tok], len(ids)
    for _ in range(n - 1):
        _, tok = m.forward_step(tok, off, want_logits=False)
        toks.append(tok)
        off += 1
    m.clear_cache()
    return toks


def test_generate_batch_asr_exact_greedy(decisive_asr):
    from aha_amd import sampling as hs
    cfg, w, m = decisive_asr
    reqs = batch(cfg)
    assert min(len(r[0]) for r in reqs) < 40 < max(len(r[0]) for r in reqs)
    o = oa.OracleQwen3ASR(cfg, w, NM)
    want = []
    for ids, data, feats in reqs:
        o.clear_cache()
        toks, lgs = oq.greedy_generate(o, ids, MAX_NEW, mm=feats, return_logits=True)
        assert min(decisive.margin_std(lg) for lg in lgs) >= 0.5
        assert serial_greedy(m, ids, data, MAX_NEW) == toks
        want.append(toks)
    prompts, datas = [r[0] for r in reqs], [r[1] for r in reqs]
    for budget in (1, 0):
        got = m.generate_batch_mm(prompts, datas, MAX_NEW, max_tokens_per_pass=budget)
        assert m.cache_len() == 0
        assert got == want, budget
    # the ASR loop over the same requests (one chunk each; the tiny model has no eos ids): generate_asr_batch = generate_asr
    audio = [[(ids, data)] for ids, data, _ in reqs if data is not None]
    assert hs.generate_asr_batch(m, audio, 0.0, max_tokens=MAX_NEW) == [hs.generate_asr(m, r, 0.0, max_tokens=MAX_NEW) for r in audio]


def test_generate_batch_asr_logits_against_oracle(asr):
    """Teacher-forced on the batch's own tokens; the bounds of tests/test_asr_gpu.py (audio given as features, as the oracle takes it)."""
    cfg, w, m = asr
    reqs = batch(cfg, all_features=True)
    prompts, datas = [r[0] for r in reqs], [r[1] for r in reqs]
    toks, step = m.generate_batch_mm(prompts, datas, 5, want_step_logits=True)
    o = oa.OracleQwen3ASR(cfg, w, NM)
    for j, (ids, data, feats) in enumerate(reqs):
        if data is None:
            continue
        o.clear_cache()
        ref = o.forward_initial(ids, 0, feats).reshape(-1).numpy()
        off = len(ids)
        for t in range(len(toks[j])):
            if t > 0:
                ref = o.forward_step([toks[j][t - 1]], off).reshape(-1).numpy()
                off += 1
            l_max, l_rms = rel_err(step[j, t], ref)
            assert l_max < 0.05 and l_rms < 0.02, f"request {j} step {t}: max {l_max:.4f} rms {l_rms:.4f}"
    assert m.cache_len() == 0


def test_generate_batch_asr_isolation(asr):
    """[A, B] and [A, C], B and C of equal length but different content: A's tokens and step logits are bit-identical (same shapes, so
    the same plans) -- nothing of B or C leaks into A through the attention, the conv windows or the compaction."""
    cfg, w, m = asr
    a = audio_request(cfg, 40000, 21)
    b = audio_request(cfg, 56000, 22)
    c = audio_request(cfg, 56000, 23)
    assert b[0] == c[0] or len(b[0]) == len(c[0])
    ta, sa = m.generate_batch_mm([a[0], b[0]], [a[1], b[1]], 6, want_step_logits=True)
    tb, sb = m.generate_batch_mm([a[0], c[0]], [a[1], c[1]], 6, want_step_logits=True)
    assert ta[0] == tb[0]
    assert np.array_equal(sa[0].view(np.uint32), sb[0].view(np.uint32))
    assert not np.array_equal(sa[1], sb[1])


def test_single_clip_path_unchanged(asr):
    """forward_initial's audio embeddings and prefill logits for three clips (samples, features, a partial window), bit for bit those
    of the one-clip tower before the batched one."""
    from aha_amd.model import MultiModalData
    cfg, w, m = asr
    golden = json.load(open(GOLDEN))
    assert set(golden) == {"samples", "features", "partial"}
    for name, rec in golden.items():
        wave = synth_audio(rec["n_samples"], rec["seed"])
        n_tok = oa.get_feat_extract_output_lengths(rec["n_samples"] // 160)
        assert n_tok == rec["n_tok"]
        ids = make_ids(cfg, n_tok, rec["seed"])
        data = MultiModalData(audio_features=oa.log_mel(wave)) if name == "features" else MultiModalData(audio_samples=wave)
        m.clear_cache()
        lg, am = m.forward_initial(ids, 0, data)
        assert sha(m.debug_audio_embeds(n_tok)) == rec["embeds_sha256"], name
        assert sha(lg) == rec["logits_sha256"], name
        assert am == rec["argmax"]
    m.clear_cache()


def test_logmel_batch_bit_identical_per_clip(gpu):
    from aha_amd import ops
    lens = [401, 16000, 47999, 480000]
    clips = [torch.from_numpy(synth_audio(n, 30 + i)).to(gpu) for i, n in enumerate(lens)]
    out = ops.logmel_batch(clips).cpu().numpy()
    assert out.shape == (128, sum(n // 160 for n in lens))
    col = 0
    for c, n in zip(clips, lens):
        one = ops.logmel(c).cpu().numpy()
        assert np.array_equal(out[:, col:col + n // 160].view(np.uint32), one.view(np.uint32)), n
        col += n // 160


def test_one_tower_pass_launch_counts(asr):
    """Four clips in one prefill pass: one log-mel launch pair for all of them and one attention launch per encoder layer."""
    cfg, w, m = asr
    reqs = [audio_request(cfg, n, 40 + i) for i, n in enumerate([9600, 40000, 64000, 116800])]
    m.set_profiling(True)
    try:
        m.generate_batch_mm([r[0] for r in reqs], [r[1] for r in reqs], 1)
        attn = m.get_profile("attn_audio")["launches"]
        mel = m.get_profile("logmel")["launches"]
    finally:
        m.set_profiling(False)
    assert attn == cfg.audio.encoder_layers
    assert mel == 1
    assert m.cache_len() == 0


def test_generate_batch_asr_errors_and_state(asr, gpu):
    from aha_amd.model import HipInferenceModel, MultiModalData
    cfg, w, m = asr
    a = audio_request(cfg, 40000, 51)
    text = [int(x) for x in np.random.default_rng(5).integers(0, 1900, size=9)]
    m.clear_cache()
    lg0, t0 = m.forward_initial(a[0], 0, a[1])
    st0, _ = m.forward_step(t0, len(a[0]))
    m.clear_cache()

    def expect(datas, prompts, code, words):
        with pytest.raises(AhaHipError) as e:
            m.generate_batch_mm(prompts, datas, 4)
        assert e.value.code == code, str(e.value)
        for wd in words:
            assert wd in str(e.value), str(e.value)
        assert m.cache_len() == 0

    wrong = list(a[0])
    wrong.insert(7, cfg.audio_token_id)
    expect([a[1], a[1]], [a[0], wrong], -4, ["sequence 1", "n_audio_tokens num"])
    expect([None, MultiModalData(audio_samples=synth_audio(400, 1))], [text, a[0]], -1, ["sequence 1", "400 samples"])
    expect([a[1], None, MultiModalData()], [a[0], text, a[0]], -1, ["sequence 2", "without features or samples"])
    pv = torch.zeros(16, 3 * 2 * 16 * 16, dtype=torch.bfloat16)
    expect([MultiModalData(pv, np.asarray([[1, 4, 4]], dtype=np.uint32))], [text], -6, ["sequence 0", "vision tower"])
    # a successful batch, then the single-request path gives the same bits as before
    assert len(m.generate_batch_mm([a[0], text], [a[1], None], 3)[1]) == 3
    assert m.cache_len() == 0
    lg1, t1 = m.forward_initial(a[0], 0, a[1])
    st1, _ = m.forward_step(t1, len(a[0]))
    m.clear_cache()
    assert t1 == t0 and np.array_equal(lg1.view(np.uint32), lg0.view(np.uint32)) and np.array_equal(st1.view(np.uint32), st0.view(np.uint32))
    # audio on a model without an audio tower
    tcfg = tiny_qwen3(vocab=2048)
    tm = HipInferenceModel(tcfg, qwen3_text_weights(tcfg, seed=0))
    try:
        with pytest.raises(AhaHipError) as e:
            tm.generate_batch_mm([text, text], [None, a[1]], 2)
        assert e.value.code == -6 and "sequence 1" in str(e.value) and "audio tower" in str(e.value)
        assert tm.cache_len() == 0
    finally:
        tm.close()


def replay(params, toks, step_logits):
    """generate_generic's sampler on the reported step logits, in the oracle restatement; one RNG stream per sequence."""
    s = osamp.get_logit_processor(params.temperature, params.top_p, params.top_k)
    rng = ornd.StdRng.seed_from_u64(params.seed)
    pen_v = 1.0 if params.repeat_penalty is None else params.repeat_penalty
    out = []
    for t in range(len(toks)):
        pen = osamp.use_repeat_penalty(pen_v, params.repeat_last_n, step_logits[t], out)
        tok = int(np.argmax(pen)) if s.kind == "ArgMax" else ornd.sample_multinomial(rng, osamp.final_weights(pen, s))
        out.append(tok)
    return out


def test_generate_batch_asr_sampled_replay(asr):
    """Single-chunk sampled requests (the ASR loop's sampler: top_k None, penalty 1) replayed with the sampler specification."""
    cfg, w, m = asr
    reqs = [r for r in batch(cfg) if r[1] is not None]
    mixed = [SamplingParams(1.0, seed=34562), SamplingParams(0.7, top_p=0.9, seed=5), SamplingParams()]
    params = [mixed[j % 3] for j in range(len(reqs))]
    toks, step = m.generate_batch_mm([r[0] for r in reqs], [r[1] for r in reqs], 10, params=params, want_step_logits=True)
    for j, p in enumerate(params):
        assert len(toks[j]) == 10
        assert replay(p, toks[j], step[j]) == toks[j], f"request {j} ({p}) differs from the sampler specification"
    assert m.cache_len() == 0
