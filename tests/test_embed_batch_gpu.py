"""-m gpu: packed variable-length embedding (aha_hip_embed_batch / HipInferenceModel.embed_batch).  Every row must be the embedding of
its own text: against the oracle restatement of Qwen3Embedding::embed_one (oracle/qwen3.py; reference qwen3_embedding/mod.rs:50-64),
against the library's single-text path, bit for bit independent of what the other texts of the batch hold, and independent of batch
order and pass split.  Two shapes: 4 q / 2 kv heads (grid block order of the segmented attention) and 16 / 8 heads (the XCD-aware order,
kv heads a multiple of 8) on a scrambled page pool."""
import numpy as np
import pytest

from aha_amd.configs import tiny_qwen3
from aha_amd.weights import qwen3_text_weights
from oracle import qwen3 as oq
from oracle.numerics import Numerics

pytestmark = pytest.mark.gpu

# page (64-token) and q-block (64 rows) edges, and one text of several pages
LENS = [1, 2, 15, 16, 17, 63, 64, 65, 127, 128, 129, 300]


def _make(cfg, scramble):
    from aha_amd.model import HipInferenceModel
    w = qwen3_text_weights(cfg, seed=0)
    m = HipInferenceModel(cfg, w)
    if scramble:
        m.debug_scramble_pages(True)
    return m, oq.OracleQwen3(cfg, w, Numerics("bf16", matmul_f64=True))


@pytest.fixture(scope="module", params=["narrow", "wide"])
def pair(gpu, request):
    if request.param == "narrow":
        cfg = tiny_qwen3(layers=3, hidden=512, heads=4, kv_heads=2, inter=1024, vocab=4096)
    else:
        cfg = tiny_qwen3(layers=2, hidden=1024, heads=16, kv_heads=8, inter=3072, vocab=4096)
    m, o = _make(cfg, scramble=request.param == "wide")
    yield cfg, m, o
    m.close()


def seqs_for(cfg, lens, seed):
    g = np.random.default_rng(seed)
    return [[int(x) for x in g.integers(0, cfg.vocab_size, size=n)] for n in lens]


def cos_rows(a, b):
    return (a * b).sum(-1) / (np.linalg.norm(a, axis=-1) * np.linalg.norm(b, axis=-1))


def test_embed_batch_matches_oracle(pair):
    """The bounds of test_embedding_gpu.py::test_embed_matches_oracle per row of one mixed-length batch: unit norm to 1e-5, cosine to
    the oracle >= 0.9995, per element <= 0.04 of the row's rms -- or, where the single-text path itself lies further from the oracle
    (embed_one on these texts reaches 0.047 rms on the narrow shape and 0.062 on the wide one), no further than embed_one + 0.01 rms."""
    cfg, m, o = pair
    seqs = seqs_for(cfg, LENS, 11)
    got = m.embed_batch(seqs)
    assert got.shape == (len(LENS), cfg.hidden_size) and got.dtype == np.float32
    for j, ids in enumerate(seqs):
        ref = oq.embed_one(o, ids).numpy()
        assert abs(float(np.linalg.norm(got[j])) - 1.0) < 1e-5, j
        rms = float(np.sqrt((ref ** 2).mean()))
        bound = max(0.04 * rms, float(np.abs(m.embed_one(ids) - ref).max()) + 0.01 * rms)
        assert float(np.abs(got[j] - ref).max()) <= bound, (j, len(ids))
        assert float(got[j] @ ref) >= 0.9995, (j, len(ids))
    assert m.cache_len() == 0


def test_embed_batch_rows_are_isolated(pair):
    """A sequence's row does not depend on the tokens of the other sequences (lengths fixed): bit-identical.  A mask or page window
    that let one sequence see another's keys would move it."""
    cfg, m, o = pair
    seqs = seqs_for(cfg, LENS, 12)
    other = seqs_for(cfg, LENS, 13)
    base = m.embed_batch(seqs)
    # every other sequence replaced: the untouched ones keep their bits
    alt = m.embed_batch([other[j] if j % 2 else s for j, s in enumerate(seqs)])
    for j in range(0, len(LENS), 2):
        np.testing.assert_array_equal(alt[j], base[j], err_msg=f"row {j} (len {LENS[j]})")
    # all but one replaced
    for t in (1, 7, len(LENS) - 1):
        alt = m.embed_batch([s if j == t else other[j] for j, s in enumerate(seqs)])
        np.testing.assert_array_equal(alt[t], base[t], err_msg=f"row {t} (len {LENS[t]})")


def test_embed_batch_agrees_with_embed_one(pair):
    """Every row against the single-text path: cosine >= 0.9999.  One sequence of 2 .. 999 tokens runs the same kernels as embed_one
    (only the final normalisation moved to the device): |delta| <= 1e-6 per element."""
    cfg, m, o = pair
    seqs = seqs_for(cfg, LENS, 14)
    got = m.embed_batch(seqs)
    one = np.stack([m.embed_one(s) for s in seqs])
    assert float(cos_rows(got, one).min()) >= 0.9999
    for s in seqs:
        if 2 <= len(s) < 1000:
            d = float(np.abs(m.embed_batch([s])[0] - m.embed_one(s)).max())
            assert d <= 1e-6, (len(s), d)


def test_embed_batch_order_and_passes(pair):
    cfg, m, o = pair
    seqs = seqs_for(cfg, LENS, 15)
    base = m.embed_batch(seqs)
    perm = np.random.default_rng(0).permutation(len(seqs))
    got = m.embed_batch([seqs[i] for i in perm])
    assert float(cos_rows(got, base[perm]).min()) >= 0.9999
    # 256 tokens per pass (927 in all): at least four passes, the last sequence (300) longer than the budget
    m.set_profiling(True)
    try:
        split = m.embed_batch(seqs, max_tokens_per_pass=256)
        launches = m.get_profile("attn_prefill")["launches"]
    finally:
        m.set_profiling(False)
    assert launches % cfg.num_hidden_layers == 0 and launches // cfg.num_hidden_layers >= 4, launches
    assert float(cos_rows(split, base).min()) >= 0.9999
    assert m.cache_len() == 0


def test_embed_batch_leaves_generation_state_alone(pair):
    """cache empty afterwards; a prompt's prefill + 4 decode steps give the same logits bits before and after an embed_batch call."""
    cfg, m, o = pair
    prompt = seqs_for(cfg, [90], 16)[0]

    def run():
        m.clear_cache()
        lg, tok = m.forward_initial(prompt, 0)
        out = [lg.copy()]
        for i in range(4):
            lg, tok = m.forward_step(tok, len(prompt) + i)
            out.append(lg.copy())
        m.clear_cache()
        return np.stack(out)

    before = run()
    m.embed_batch(seqs_for(cfg, LENS, 17))
    assert m.cache_len() == 0
    np.testing.assert_array_equal(run(), before)


def test_embed_batch_errors_and_cost(pair):
    from aha_amd._lib import AhaHipError
    cfg, m, o = pair
    seqs = seqs_for(cfg, [40, 7, 130], 18)
    good = m.embed_batch(seqs)
    with pytest.raises(AhaHipError, match="empty"):
        m.embed_batch([])
    with pytest.raises(AhaHipError, match="empty"):
        m.embed_batch([seqs[0], []])
    with pytest.raises(AhaHipError, match=r"out of range in sequence 1 at position 3"):
        m.embed_batch([seqs[0], [1, 2, 3, cfg.vocab_size]])
    assert m.cache_len() == 0
    np.testing.assert_array_equal(m.embed_batch(seqs), good)   # still usable, same bits
    # one pass: exactly one attention launch per layer
    m.set_profiling(True)
    try:
        m.embed_batch(seqs)
        assert m.get_profile("attn_prefill")["launches"] == cfg.num_hidden_layers
    finally:
        m.set_profiling(False)


def test_embed_batch_across_prefill_scratch_growth(pair):
    """A longer forward_initial between two calls regrows the prefill scratch; the batch's own tables and output buffer are not part
    of it and must survive (the second call here also grows them)."""
    cfg, m, o = pair
    small, big = seqs_for(cfg, [5, 9], 19), seqs_for(cfg, LENS, 20)
    ref = m.embed_batch(big)
    m.embed_batch(small)
    m.clear_cache()
    m.forward_initial(seqs_for(cfg, [1500], 21)[0], 0)
    m.clear_cache()
    np.testing.assert_array_equal(m.embed_batch(big), ref)
    assert m.cache_len() == 0
