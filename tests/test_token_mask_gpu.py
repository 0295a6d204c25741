"""-m gpu: per-step allowed-token masks (guided decoding) on the device -- aha_hip_sample_rows_masked, aha_hip_generate_batch_masked,
aha_hip_engine_submit_masked / aha_hip_engine_set_mask.

The definition (include/aha_hip.h), restated in numpy wherever a reference is needed: z = the step's f32 logits after the repeat penalty
and the addends (steps 1-3 of the logit_bias definition); z_i = -inf for every id whose bit i & 31 of word i >> 5 is clear (bits at
positions >= V are ignored); the request's sampler runs on z; RNG consumption is unchanged; logprobs stay those of the raw logits.

  1. the op against numpy: z built in f32, masked, then oracle.sampling.topk_candidates; idx and the bits of vals and max equal, sumexp
     within 2e-5 relative of the f64 sum (the bound tests/test_logit_adjust_gpu.py states for its op test: the same __expf sum); entries past
     the number of allowed ids are -inf; an all-ones mask and no mask are bit-identical to ops.sample_rows_adjusted; the logits only read;
  2. generation: every token equals the oracle replay (penalty, addends, mask, sampler with the same seed) on the reported step logits;
     guided choice through generate_batch_masked and through the engine; a callback that returns 0 / all-ones masks against
     generate_batch_adjusted bit for bit; logprobs; isolation from the batch;
  3. the engine: sticky / replaced / cleared masks, the first token, slot reuse, mixed requests;  4. errors.

The models are the three tiny shapes of tests/test_logprobs_gpu.py::Models (V = 4096 / 2048) with two stop ids each, so that a constraint
can end a sequence.
"""
import numpy as np
import pytest
import torch

from aha_amd._lib import AhaHipError
from aha_amd.configs import tiny_qwen3, tiny_qwen3vl
from aha_amd.guided import ChoiceConstraint, mask_words, pack_mask, unpack_mask
from aha_amd.sampling import SamplingParams
from aha_amd.weights import qwen3_text_weights, qwen3vl_weights
from oracle import rand_stdrng as ornd
from oracle import sampling as osamp

from test_generate_sampled_gpu import LENS, MIXED, QWEN3_DEFAULT
from test_logit_adjust_cpu import addends
from test_logit_adjust_gpu import PAIRS, make_adjust_list, with_adjust
from test_logprobs_gpu import bits, check_sequences, make_rows, profiled, prompts_for

pytestmark = pytest.mark.gpu
NINF = float("-inf")
MAX_NEW = 16
STOPS = [5, 77]


def allowed_of(words, V):
    ids = np.arange(V)
    return ((np.asarray(words, dtype=np.uint32)[ids >> 5] >> (ids & 31).astype(np.uint32)) & np.uint32(1)).astype(bool)


def garbage_past(words, V):
    w = np.array(words, dtype=np.uint32)
    if V % 32:
        w[-1] |= np.uint32((0xffffffff << (V % 32)) & 0xffffffff)
    return w


# ---- 1. the op ------------------------------------------------------------------------------------------------------------------------
PATTERNS = ("ones", "first", "last", "last_word", "wave_cleared", "one_wave_left", "alternating", "half", "sparse", "none")


def make_pattern(name, V, g):
    """The allowed ids (bool, V) of one pattern, or None for a row without a mask."""
    a = np.zeros(V, dtype=bool)
    if name == "none":
        return None
    if name == "ones":
        a[:] = True
    elif name == "first":
        a[0] = True
    elif name == "last":
        a[V - 1] = True
    elif name == "last_word":                                         # inside the last (for V % 32 != 0: partial) word, not at its ends if it has room
        lo = (V - 1) // 32 * 32
        a[lo + (V - 1 - lo) // 2] = True
    elif name == "wave_cleared":                                      # one whole stage-1 wave's 512 ids cleared (V <= 512: the first half)
        a[:] = True
        a[512:1024] = False
        if V <= 512:
            a[:] = True
            a[:max(V // 2, 1) if V > 1 else 0] = False
    elif name == "one_wave_left":                                     # all but the last wave cleared (V <= 512: all but the second half)
        a[(V - 1) // 512 * 512 if V > 512 else V // 2:] = True
    elif name == "alternating":
        a[(1 if V > 1 else 0)::2] = True
    elif name == "half":
        a = g.random(V) < 0.5
    elif name == "sparse":
        a = g.random(V) < 1e-3
    if not a.any():
        a[int(g.integers(0, V))] = True
    return a


def masked_reference(x, k, temp, pen, ctx, ids, vals, allowed):
    y = osamp.apply_repeat_penalty(x, pen, ctx) if pen != 1.0 else x.copy()
    z = np.asarray(y, dtype=np.float32).copy()
    if len(ids):
        i = np.asarray(ids, dtype=np.int64)
        z[i] = z[i] + np.asarray(vals, dtype=np.float32)           # one f32 add per listed id
    if allowed is not None:
        z[~allowed] = -np.inf
    wv, wi, wm, wse = osamp.topk_candidates(z, k, temp)
    return z, wv, wi, np.float32(wm), wse


@pytest.mark.parametrize("V", [1, 31, 32, 33, 511, 512, 513, 1536, 4096, 151936])
def test_sample_rows_masked_against_numpy(gpu, V):
    from aha_amd import ops
    R_ALL, PAD, W = 40, 5, mask_words(V)
    host = make_rows(R_ALL, V, 700 + V % 89).numpy().copy()
    g = np.random.default_rng(2000 + V)
    rows, mask_tab = [], np.zeros((R_ALL, W), dtype=np.uint32)
    for r in range(R_ALL):
        name = PATTERNS[r % len(PATTERNS)]
        allowed = make_pattern(name, V, g)
        k = min(V, int(g.choice([1, 2, 20, 63, 64])) if r % 3 else int(g.integers(1, 65)))
        temp = float(g.choice([0.0, 0.6, 1.3, 7.0]))
        form = (0, 1, 2, 4, 7)[(r // len(PATTERNS) + r) % 5]          # masks combined with a penalty context and addends (finite ones)
        pen = 1.3 if form == 7 else float(g.choice([1.0, 1.2, 0.9]))
        ctx = [int(c) for c in g.integers(0, min(V, 64), size=int(g.integers(1 if form == 7 else 0, 30)))]
        if r % 5 == 0:
            ctx += [V + 3]
        if allowed is not None and not np.isfinite(host[r][allowed]).any():   # (a -inf logit under the only allowed id: unspecified, so
            host[r, int(np.flatnonzero(allowed)[0])] = 0.25                   #  the test's own row gets a finite one there)
        y = osamp.apply_repeat_penalty(host[r], pen, ctx) if pen != 1.0 else host[r]
        ids, vals = make_adjust_list(form, y, V, k, ctx, g)
        if allowed is not None:
            w = pack_mask(np.flatnonzero(allowed).tolist(), V)
            mask_tab[r] = garbage_past(w, V) if r % 2 else w          # garbage in the bits past V on every other row
            assert np.array_equal(allowed_of(mask_tab[r], V), allowed)
        z, wv, wi, wm, wse = masked_reference(host[r], k, temp, pen, ctx, ids, vals, allowed)
        assert np.isfinite(z).any(), (V, r, name)
        rows.append(dict(name=name, k=k, temp=temp, pen=pen, ctx=ctx, adj=(ids, vals), allowed=allowed, want=(wv, wi, wm, wse)))
    if V == 1536:
        assert any(not r["allowed"][512:1024].any() and r["allowed"][:512].all() for r in rows if r["name"] == "wave_cleared")
    dev = torch.full((R_ALL, V + PAD), 3.0e38, dtype=torch.float32)   # a row pitch above V; a read past V would pick the padding up
    dev[:, :V] = torch.from_numpy(host)
    dev = dev.cuda()
    before = dev.clone()
    masks = torch.from_numpy(mask_tab.view(np.int32)).cuda()
    worst = 0.0
    for R in (1, 7, 40):
        sel = list(range(R)) if R != 7 else [6, 13, 3, 5, 29, 38, 0]   # masked and unmasked rows mixed, masks not in row order
        lg = dev[sel][:, :V] if R != 40 else dev[:, :V]
        assert lg.stride(0) == V + PAD
        args = ([rows[i]["k"] for i in sel], [rows[i]["temp"] for i in sel], [rows[i]["pen"] for i in sel], [rows[i]["ctx"] for i in sel],
                [rows[i]["adj"] for i in sel])
        mask_rows = [-1 if rows[i]["allowed"] is None else i for i in sel]
        vals, idx, ms = ops.sample_rows_masked(lg, *args, masks, mask_rows)
        pv, pi, pm = ops.sample_rows_adjusted(lg, *args)
        torch.cuda.synchronize()
        vals, idx, ms = vals.cpu().numpy(), idx.cpu().numpy().view(np.uint32), ms.cpu().numpy()
        pv, pi, pm = pv.cpu().numpy(), pi.cpu().numpy().view(np.uint32), pm.cpu().numpy()
        for s, i in enumerate(sel):
            row = rows[i]
            k, (wv, wi, wm, wse) = row["k"], row["want"]
            what = (V, R, i, row["name"])
            assert np.array_equal(idx[s, :k], wi), (what, idx[s, :k], wi)
            assert np.array_equal(bits(vals[s, :k]), bits(wv)), what
            assert bits(ms[s, 0]) == bits(wm), (what, ms[s, 0], wm)
            assert np.isfinite(ms[s, 1]), (what, ms[s])
            rel = abs(float(ms[s, 1]) - wse) / wse
            worst = max(worst, rel)
            assert rel <= 2e-5, (what, ms[s, 1], wse)
            if row["allowed"] is not None:                            # entries past the number of allowed ids are -inf, and every
                n_allowed = int(row["allowed"].sum())                 # finite entry is an allowed id
                assert np.isneginf(vals[s, n_allowed:k]).all(), what
                assert row["allowed"][idx[s, :k][np.isfinite(vals[s, :k])].astype(np.int64)].all(), what
            if row["name"] in ("ones", "none"):                       # what sample_rows_adjusted gives, bit for bit
                assert np.array_equal(bits(vals[s, :k]), bits(pv[s, :k])) and np.array_equal(idx[s, :k], pi[s, :k]), what
                assert np.array_equal(bits(ms[s]), bits(pm[s])), what
    assert torch.equal(dev.view(torch.int32), before.view(torch.int32)), "sample_rows_masked wrote its input logits"
    assert np.array_equal(masks.cpu().numpy().view(np.uint32), mask_tab), "sample_rows_masked wrote its masks"
    print(f"\nsample_rows_masked V={V}: max relative sumexp error {worst:.3e} (bound 2e-5)")


def test_sample_rows_masked_argument_errors(gpu):
    from aha_amd import ops
    lg = torch.zeros(2, 600, device="cuda")
    masks = torch.full((1, mask_words(600)), -1, dtype=torch.int32, device="cuda")
    with pytest.raises(AssertionError):
        ops.sample_rows_masked(lg, [1, 1], [0.0, 0.0], [1.0, 1.0], [[], []], None, masks, [0, 1])      # a mask that does not exist
    with pytest.raises(AssertionError):
        ops.sample_rows_masked(lg, [1, 1], [0.0, 0.0], [1.0, 1.0], [[], []], None, masks[:, :-1].contiguous(), [0, -1])
    with pytest.raises(AhaHipError, match="sample_rows_adjusted: row"):                                # the addends keep their checks
        ops.sample_rows_masked(lg, [1, 1], [0.0, 0.0], [1.0, 1.0], [[], []], [([600], [1.0]), ([], [])], masks, [0, -1])
    vals, idx, ms = ops.sample_rows_masked(lg, [1, 1], [0.0, 0.0], [1.0, 1.0], [[], []], None, masks, [0, -1])
    assert idx.cpu().numpy()[:, 0].tolist() == [0, 0]


# ---- 2. generation --------------------------------------------------------------------------------------------------------------------
class StopModels:
    """tests/test_logprobs_gpu.py::Models' three shapes, each with the stop ids STOPS, built when first asked for."""

    def __init__(self):
        self.built = {}

    def get(self, name):
        from aha_amd.model import HipInferenceModel
        if name not in self.built:
            if name == "narrow":
                cfg = tiny_qwen3(layers=3, hidden=512, heads=4, kv_heads=2, inter=1024, vocab=4096)
                cfg.eos_token_ids = list(STOPS)
                m = HipInferenceModel(cfg, qwen3_text_weights(cfg, seed=0))
            elif name == "wide":
                cfg = tiny_qwen3(layers=2, hidden=1024, heads=16, kv_heads=8, inter=3072, vocab=4096)
                cfg.eos_token_ids = list(STOPS)
                m = HipInferenceModel(cfg, qwen3_text_weights(cfg, seed=0))
                m.debug_scramble_pages(True)
            else:
                cfg = tiny_qwen3vl()
                cfg.text.eos_token_ids = list(STOPS)
                m = HipInferenceModel(cfg, qwen3vl_weights(cfg, seed=0))
            assert m.stop_token_ids() == STOPS
            self.built[name] = m
        return name, self.built[name].text_cfg, self.built[name]


@pytest.fixture(scope="module")
def models(gpu):
    ms = StopModels()
    yield ms
    for m in ms.built.values():
        m.close()


ALL_MODELS = pytest.mark.parametrize("which", ["narrow", "wide", "vl"])


def step_allowed(seq, step, V):
    """The seeded pseudo-random mask of (seq, step): about 40 % allowed, the stop ids included on one step in three and excluded on the
    others; ids 17 and 1000 (the +100 / +9 biases of tests/test_logit_adjust_gpu.py's adjusts) follow the coin like every other id."""
    a = np.random.default_rng(100003 * seq + step).random(V) < 0.4
    a[STOPS] = (seq + step) % 3 == 0
    return a


class RandomConstraint:
    """The constraint protocol over step_allowed; `seq_of` maps the call's sequence index to the mask stream (the isolation test runs
    sequence j alone as sequence 0).  Counts the calls and the bytes handed over."""

    def __init__(self, V, seq_of=lambda s: s):
        self.V, self.seq_of, self.calls = V, seq_of, []

    def __call__(self, seq, generated):
        self.calls.append((seq, len(generated)))
        return garbage_past(pack_mask(np.flatnonzero(step_allowed(self.seq_of(seq), len(generated), self.V)).tolist(), self.V), self.V)


def masked_params():
    return [with_adjust(p, PAIRS[j]) for j, p in enumerate(MIXED)]


def replay(params, toks, step_logits, V, allowed_at):
    """tests/test_logit_adjust_gpu.py's replay with step 3b between the addends and the sampler; allowed_at(t) -> bool (V,) or None."""
    s = osamp.get_logit_processor(params.temperature, params.top_p, params.top_k)
    rng = ornd.StdRng.seed_from_u64(params.seed)
    pen_v = 1.0 if params.repeat_penalty is None else params.repeat_penalty
    bias = list((params.logit_bias or {}).items())
    out = []
    for t in range(len(toks)):
        z = np.asarray(osamp.use_repeat_penalty(pen_v, params.repeat_last_n, step_logits[t], out), dtype=np.float32).copy()
        if params.adjust_active:
            ids, a = addends(params.presence_penalty, params.frequency_penalty, bias, out, V)
            z[ids] = z[ids] + a
        allowed = allowed_at(t)
        if allowed is not None:
            z[~allowed] = -np.inf
        if s.kind == "ArgMax":
            tok = int(np.argmax(z))
        else:
            w = osamp.final_weights(z, s)
            if s.kind in ("TopK", "TopKThenTopP") and s.k < V:
                prs = osamp.softmax_last_dim(z * np.float32(1.0 / s.temperature))
                keep = osamp.topk_order(prs, z)[: s.k]
                tok = int(keep[ornd.sample_multinomial(rng, w[keep])])
            else:
                tok = ornd.sample_multinomial(rng, w)
        out.append(tok)
    return out


RUNS = {}


def masked_run(models, which):
    """One masked call per model, with adjusts and logprobs, shared by the replay and the logprob tests."""
    if which not in RUNS:
        name, cfg, m = models.get(which)
        prompts = prompts_for(len(MIXED), 51, cfg.vocab_size, LENS)
        tops = [(None, 0, 1, 5, 20)[(j + 2) % 5] for j in range(len(prompts))]
        params = masked_params()
        con = RandomConstraint(cfg.vocab_size)
        toks, lps, step = m.generate_batch_masked(prompts, MAX_NEW, con, params, tops, want_step_logits=True)
        assert m.cache_len() == 0
        RUNS[which] = (prompts, params, tops, toks, lps, step, con)
    return RUNS[which]


@ALL_MODELS
def test_generate_batch_masked_exact_replay(models, which):
    name, cfg, m = models.get(which)
    V = cfg.vocab_size
    prompts, params, tops, toks, lps, step, con = masked_run(models, which)
    plain, _ = m.generate_batch_adjusted(prompts, MAX_NEW, params)
    ended = 0
    for j, p in enumerate(params):
        # the callback was asked once per live sequence per step, the first token included, and never after the sequence ended
        assert [n for s, n in con.calls if s == j] == list(range(len(toks[j]))), j
        assert replay(p, toks[j], step[j], V, lambda t: step_allowed(j, t, V)) == toks[j], f"sequence {j} ({p}) differs from the oracle replay"
        for t, tok in enumerate(toks[j]):
            assert step_allowed(j, t, V)[tok], (j, t, tok)
        assert len(toks[j]) == MAX_NEW or (toks[j][-1] in STOPS and len(toks[j]) > 1), (j, toks[j])
        assert not set(toks[j][1:-1]) & set(STOPS), (j, toks[j])
        ended += len(toks[j]) < MAX_NEW
    print(f"\n{name}: {ended} of {len(params)} sequences ended on a stop id; differ from the unmasked call: {[a != b for a, b in zip(toks, plain)]}")
    assert sum(a != b for a, b in zip(toks, plain)) >= len(params) - 1    # a 40 % mask moves (nearly) every sequence


def choice_setup(cfg):
    V = cfg.vocab_size
    choices = [[900, 901, 902], [900, 901], [900, 950, 951, 952, 953, 954], [1200], [1300, 901, 17, 23]]   # 1-6 tokens, shared prefixes
    return choices, ChoiceConstraint(choices, STOPS, V)


def is_choice_then_stop(toks, choices):
    return len(toks) >= 2 and toks[-1] in STOPS and toks[:-1] in choices


CHOICE_PARAMS = [None, SamplingParams(**QWEN3_DEFAULT, seed=2), SamplingParams(1.2, seed=6), SamplingParams(0.0, repeat_penalty=1.3, repeat_last_n=5),
                 SamplingParams(1.0, top_p=0.9, seed=4), SamplingParams(0.9, top_k=20, seed=1, logit_bias={1300: 4.0, 900: NINF})]


@ALL_MODELS
def test_choice_constraint_through_generate_batch_masked(models, which):
    name, cfg, m = models.get(which)
    choices, con = choice_setup(cfg)
    prompts = prompts_for(12, 81, cfg.vocab_size, LENS)
    for params in (None, [CHOICE_PARAMS[1 + j % 5] for j in range(12)]):   # greedy, then sampled
        toks, _ = m.generate_batch_masked(prompts, 10, con, params)
        for j, t in enumerate(toks):
            assert is_choice_then_stop(t, choices), (name, j, t)
        assert m.cache_len() == 0
        print(f"\n{name}: choices taken: {sorted(set(tuple(t[:-1]) for t in toks))}")
    assert toks[4][0] != 900 and toks[9][0] != 900                    # the -inf bias holds under the mask


def test_choice_constraint_through_the_engine(models):
    from aha_amd.model import HipEngine
    name, cfg, m = models.get("narrow")
    choices, con = choice_setup(cfg)
    prompts = prompts_for(6, 82, cfg.vocab_size, [70, 9, 33, 64, 5, 20])
    eng = HipEngine(m, max_running=4, kv_pages=64)
    try:
        rid = {}
        for step in range(60):
            if step < len(prompts):                                   # greedy and sampled requests, one submitted per step
                rid[eng.submit(prompts[step], 10, CHOICE_PARAMS[step], mask=con(0, []))] = step
            for ev in eng.step():
                assert not ev.cancelled
                if not ev.finished:
                    eng.set_mask(ev.req_id, con(0, eng.tokens(ev.req_id)))
            st = eng.stats()
            if step >= len(prompts) and st["running"] == 0 and st["waiting"] == 0:
                break
        assert st["free_pages"] == st["total_pages"], st
        got = {i: eng.tokens(r) for r, i in rid.items()}
    finally:
        eng.close()
    for i, p in enumerate(prompts):
        assert is_choice_then_stop(got[i], choices), (i, got[i])
        # the batch entry driven by the same constraint gives the same tokens
        want, _ = m.generate_batch_masked([p], 10, con, None if CHOICE_PARAMS[i] is None else [CHOICE_PARAMS[i]])
        assert got[i] == want[0], (i, got[i], want[0])
    print(f"\nengine: choices taken: {sorted(set(tuple(t[:-1]) for t in got.values()))}")
    assert m.cache_len() == 0


@ALL_MODELS
def test_return_zero_and_all_ones_masks_change_nothing(models, which):
    name, cfg, m = models.get(which)
    V = cfg.vocab_size
    prompts = prompts_for(len(MIXED), 51, V, LENS)
    tops = [(None, 0, 1, 5, 20)[j % 5] for j in range(len(prompts))]
    params = masked_params()
    (want, wlp, wstep), base = profiled(m, lambda: m.generate_batch_adjusted(prompts, 12, params, tops, want_step_logits=True))
    ones = np.full(mask_words(V), 0xffffffff, dtype=np.uint32)
    seen = []

    def none_cb(seq, gen):
        seen.append((seq, len(gen)))
        return None

    for con in (none_cb, lambda seq, gen: ones):
        (toks, lps, step), prof = profiled(m, lambda: m.generate_batch_masked(prompts, 12, con, params, tops, want_step_logits=True))
        assert toks == want and np.array_equal(bits(step), bits(wstep))
        for j in range(len(prompts)):
            if tops[j] is None:
                assert lps[j] is None and wlp[j] is None
                continue
            for a, b in zip(lps[j], wlp[j]):
                assert bits(a[0]) == bits(b[0]) and [i for i, _ in a[1]] == [i for i, _ in b[1]]
                assert np.array_equal(bits([v for _, v in a[1]]), bits([v for _, v in b[1]]))
        if con is none_cb:
            assert prof == base, (prof, base)                         # the launches of the five profile classes are unchanged too
            assert sorted(seen) == sorted((j, t) for j in range(len(prompts)) for t in range(len(want[j])))
    # greedy (params None) with a callback that returns 0: generate_batch's tokens, and no candidate step at all
    (gt, glp), gprof = profiled(m, lambda: m.generate_batch_masked(prompts[:5], 6, none_cb))
    assert gt == m.generate_batch(prompts[:5], 6) and glp is None and all(v == 0 for v in gprof.values()), gprof
    # a NULL callback is generate_batch_adjusted
    assert m.generate_batch_masked(prompts, 12, None, params)[0] == want


@ALL_MODELS
def test_logprobs_under_a_mask_follow_the_raw_logits(models, which):
    prompts, params, tops, toks, lps, step, con = masked_run(models, which)
    check_sequences(toks, lps, step, tops, which)
    # tokens the mask forced are unlikely under the model's own distribution: some reported logprob is far below the top one's
    low = [lp[0] for j in range(len(toks)) if tops[j] for lp in lps[j]]
    assert min(low) < -4.0, min(low)


@ALL_MODELS
def test_masked_sequences_do_not_depend_on_the_batch(models, which):
    """One prefill pass per prompt (max_tokens_per_pass=1), the rule of test_adjusted_sequences_do_not_depend_on_the_batch."""
    name, cfg, m = models.get(which)
    V = cfg.vocab_size
    prompts = prompts_for(len(MIXED), 53, V, LENS)
    params = masked_params()
    base, _, bl = m.generate_batch_masked(prompts, 12, RandomConstraint(V), params, max_tokens_per_pass=1, want_step_logits=True)
    for j in range(len(prompts)):
        alone, _, al = m.generate_batch_masked([prompts[j]], 12, RandomConstraint(V, lambda s, j=j: j), [params[j]], max_tokens_per_pass=1,
                                               want_step_logits=True)
        assert alone[0] == base[j], j
        assert np.array_equal(bits(al[0]), bits(bl[j])), j


# ---- 3. the engine --------------------------------------------------------------------------------------------------------------------
def drive(m, reqs, script=None, cancel=None, max_running=4, steps_max=200):
    """reqs[i] = (ids, max_new, params, mask) submitted before step i; script(eng, i, n_tokens) -> called after every token of request i;
    cancel = (request, step).  Returns per request its tokens and the logits that chose them."""
    from aha_amd.model import HipEngine
    eng = HipEngine(m, max_running=max_running, kv_pages=64)
    try:
        rid, toks, logits, cancelled = {}, {}, {}, set()
        for step in range(steps_max):
            if step < len(reqs):
                ids, max_new, params, mask = reqs[step]
                r = eng.submit(ids, max_new, params, mask=mask)
                rid[r] = step
                toks[step], logits[step] = [], []
            if cancel and step == cancel[1]:
                eng.cancel([r for r, i in rid.items() if i == cancel[0]][0])
            evs, lg = eng.step(want_logits=True)
            for n, ev in enumerate(evs):
                i = rid[ev.req_id]
                if ev.cancelled:
                    cancelled.add(i)
                    continue
                toks[i].append(ev.token)
                logits[i].append(lg[n].copy())
                if script and not ev.finished:
                    script(eng, ev.req_id, i, len(toks[i]))
            st = eng.stats()
            if step >= len(reqs) and st["running"] == 0 and st["waiting"] == 0:
                break
        assert st["free_pages"] == st["total_pages"], st
        return toks, logits, cancelled, eng, rid
    finally:
        eng.close()


def test_engine_sticky_replaced_cleared_and_initial_mask(models):
    name, cfg, m = models.get("narrow")
    V = cfg.vocab_size
    ps = prompts_for(2, 91, V, [33, 70])
    base = m.generate_batch([ps[0], ps[1]], 14)
    g = np.random.default_rng(7)

    def mask_without(tokens):                                         # about 40 % allowed, none of `tokens`, no stop id
        a = g.random(V) < 0.4
        a[list(tokens)] = False
        a[STOPS] = False
        return a

    A, B, M0 = mask_without(base[0]), mask_without(base[0]), mask_without(base[1])
    words = lambda a: pack_mask(np.flatnonzero(a).tolist(), V)

    def script(eng, req_id, i, n):
        if i != 0:
            return
        if n == 2:
            eng.set_mask(req_id, words(A))                            # acts from token 2, and stays
        elif n == 6:
            eng.set_mask(req_id, words(B))                            # replaced: from token 6
        elif n == 9:
            eng.set_mask(req_id, None)                                # cleared: from token 9

    # request 1 carries an initial mask that governs its first token (and every later one: it is never replaced)
    toks, logits, cancelled, _, _ = drive(m, [(ps[0], 14, None, None), (ps[1], 14, None, words(M0))], script)
    assert not cancelled and len(toks[0]) == 14 and len(toks[1]) == 14
    regime = lambda t: None if t < 2 or t >= 9 else A if t < 6 else B
    for t, tok in enumerate(toks[0]):
        a = regime(t)
        want = int(np.argmax(logits[0][t] if a is None else np.where(a, logits[0][t], -np.inf)))
        assert tok == want, (t, tok, want)
    assert toks[0][:2] == base[0][:2] and all(tok not in base[0] for tok in toks[0][2:9])
    for t, tok in enumerate(toks[1]):
        assert tok == int(np.argmax(np.where(M0, logits[1][t], -np.inf))), (t, tok)
    assert toks[1][0] != base[1][0]
    assert m.cache_len() == 0


def test_engine_slot_reuse_after_a_masked_request(models):
    name, cfg, m = models.get("narrow")
    V = cfg.vocab_size
    ps = prompts_for(2, 92, V, [33, 20])
    only = pack_mask([3000, 3001, 3002], V)
    want = m.generate_batch([ps[1]], 12)[0]
    sampled = SamplingParams(**QWEN3_DEFAULT, seed=3)
    want_s = m.generate_batch_sampled([ps[1]], [sampled], 12)[0]
    # one slot: request 1 takes request 0's after it ended by length ...
    toks, _, cancelled, _, _ = drive(m, [(ps[0], 5, None, only), (ps[1], 12, None, None)], max_running=1)
    assert not cancelled and set(toks[0]) <= {3000, 3001, 3002} and toks[1] == want, (toks, want)
    # ... and after it was cancelled, greedy and sampled
    for p, w in ((None, want), (sampled, want_s)):
        toks, _, cancelled, _, _ = drive(m, [(ps[0], 40, sampled, only), (ps[1], 12, p, None)], cancel=(0, 6), max_running=1)
        assert cancelled == {0} and 0 < len(toks[0]) < 40 and set(toks[0]) <= {3000, 3001, 3002}
        assert toks[1] == w, (toks[1], w)
    assert m.cache_len() == 0


def test_engine_masked_adjusted_and_plain_requests_share_steps(models):
    name, cfg, m = models.get("narrow")
    V = cfg.vocab_size
    ps = prompts_for(5, 93, V, [70, 9, 33, 64, 5])
    g = np.random.default_rng(11)
    masks = [pack_mask(np.flatnonzero(g.random(V) < 0.3).tolist(), V) for _ in range(2)]
    sampled = SamplingParams(**QWEN3_DEFAULT, repeat_penalty=1.3, repeat_last_n=6, seed=3)
    reqs = [(ps[0], 14, None, masks[0]),                                                         # masked, greedy
            (ps[1], 9, None, None),                                                              # plain
            (ps[2], 16, with_adjust(sampled, PAIRS[3]), masks[1]),                               # masked, sampled, adjusted
            (ps[3], 8, with_adjust(SamplingParams(), PAIRS[0]), None),                           # adjusted only
            (ps[4], 12, SamplingParams(1.2, seed=6), masks[0])]                                  # masked, Sampling::All: the full vector
    toks, _, cancelled, _, _ = drive(m, reqs)
    assert not cancelled
    for i, (ids, max_new, params, mask) in enumerate(reqs):
        con = None if mask is None else (lambda s, gen, mask=mask: mask)
        want, _ = m.generate_batch_masked([ids], max_new, con, None if params is None else [params])
        assert toks[i] == want[0], (i, toks[i], want[0])
        if mask is not None:
            assert allowed_of(mask, V)[toks[i]].all(), i
    assert m.cache_len() == 0


# ---- 4. errors ------------------------------------------------------------------------------------------------------------------------
def test_mask_argument_errors(models):
    from aha_amd.model import HipEngine
    name, cfg, m = models.get("narrow")
    V = cfg.vocab_size
    W = mask_words(V)
    prompts = prompts_for(3, 58, V, [5, 9, 3])
    usual = m.generate_batch(prompts, 4)
    ok = pack_mask(range(100, 200), V)

    # a negative callback return: AHA_ERR_STATE naming the sequence and the step; the cache is left cleared
    def fails(seq, gen):
        return -3 if seq == 1 and len(gen) == 2 else ok
    with pytest.raises(AhaHipError, match=r"callback returned -3 for sequence 1 at step 2") as ei:
        m.generate_batch_masked(prompts, 6, fails)
    assert ei.value.code == -7 and m.cache_len() == 0
    assert m.generate_batch(prompts, 4) == usual
    # an empty callback mask (its only bits past nothing): AHA_ERR_INVALID, the same way -- on the first token too
    for at in (0, 3):
        with pytest.raises(AhaHipError, match=rf"mask of sequence 2 at step {at} allows no id") as ei:
            m.generate_batch_masked(prompts, 6, lambda seq, gen: np.zeros(W, np.uint32) if seq == 2 and len(gen) == at else ok)
        assert ei.value.code == -1 and m.cache_len() == 0
    assert m.generate_batch(prompts, 4) == usual
    # what a Python constraint can get wrong on its own: a wrong number of words, an exception -- raised again as they are
    with pytest.raises(ValueError, match="words for prompt 0"):
        m.generate_batch_masked(prompts, 6, lambda seq, gen: np.ones(W + 1, np.uint32))
    with pytest.raises(KeyError):
        m.generate_batch_masked(prompts, 6, lambda seq, gen: {}[seq])
    assert m.cache_len() == 0 and m.generate_batch(prompts, 4) == usual
    # a ChoiceConstraint whose prefix left the trie (the first step is unmasked here, so the model's own token leaves it)
    con = ChoiceConstraint([[900, 901]], STOPS, V)
    with pytest.raises(ValueError, match="not a prefix of any choice"):
        m.generate_batch_masked(prompts, 6, lambda seq, gen: None if not gen else con(seq, gen))
    assert m.cache_len() == 0
    eng = HipEngine(m, max_running=2, kv_pages=8)
    try:
        for bad, msg in ((np.ones(W - 1, np.uint32), "the mask has 127 words"), (np.ones(W + 1, np.uint32), "the mask has 129 words"),
                         (np.zeros(W, np.uint32), "the mask allows no id")):
            with pytest.raises(AhaHipError, match="engine_submit_masked: " + msg) as ei:
                eng.submit(prompts[0], 4, mask=bad)
            assert ei.value.code == -1 and eng.stats()["waiting"] == 0
        r = eng.submit(prompts[0], 3, mask=ok)
        for bad, msg in ((np.ones(W - 1, np.uint32), "the mask has 127 words"), (np.zeros(W, np.uint32), "the mask allows no id")):
            with pytest.raises(AhaHipError, match="engine_set_mask: " + msg) as ei:
                eng.set_mask(r, bad)
            assert ei.value.code == -1
        with pytest.raises(AhaHipError, match="engine_set_mask: no waiting or running request 999"):
            eng.set_mask(999, ok)
        eng.set_mask(r, None)                                         # a waiting request: cleared, then set again
        eng.set_mask(r, ok)
        got = []
        while not eng.finished(r):
            got += [ev.token for ev in eng.step()]
        assert len(got) == 3 and all(100 <= t < 200 for t in got)
        with pytest.raises(AhaHipError, match=f"engine_set_mask: no waiting or running request {r}") as ei:   # an ended id
            eng.set_mask(r, ok)
        assert ei.value.code == -1
    finally:
        eng.close()
    assert m.cache_len() == 0 and m.generate_batch(prompts, 4) == usual
