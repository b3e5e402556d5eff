"""GPU tests of suppressed tokens ("Suppressed tokens"). Everything is compared bit for bit; nothing here needs a tolerance.

  * wh_op_suppress_logits against numpy, x[:, ids] = -inf, every other float untouched, NaN guard bands around the buffer;
  * placement: wh_decode's logits with a set held are the unfiltered ones with -inf at the set, its probabilities the vocabulary softmax of those;
  * wh_lang_detect does not see the set;
  * the greedy device-side loop, tempered sampling, per-row sampling, beam search;
  * the library: Context / BatchRunner.set_suppress_tokens, the non-speech set, whisper-main -sns, the refusals.
The CPU twin: tests/test_suppress_cpu.py."""
import ctypes as C
import os
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from whisper_amd import binding, ggml_format as gf  # noqa: E402

pytestmark = pytest.mark.gpu

TOKEN_DT = np.dtype([("id", "<i4"), ("tid", "<i4"), ("p", "<f4"), ("pt", "<f4"), ("ptsum", "<f4")])
FIELDS = ("id", "tid", "p", "pt", "ptsum")


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def ptr(t):
    return C.c_void_p(t.data_ptr())


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---------------------------------------------------------------------------------------------------------------------
# 1. the op
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V", [51865, 51866])
def test_suppress_logits_op_against_numpy(V):
    """Rows 1, 5, 64; 1, 2, 88 and 4096 ids, ids 0 and eot - 1 among them; rows that already hold -inf and NaN; NaN guard bands of 4096 floats before and
    behind the buffer must keep their bits, like every float outside the set. A count of 0 writes nothing."""
    L = binding.lib()
    eot = gf.special_tokens(SimpleNamespace(n_vocab=V))["eot"]
    rng = np.random.default_rng(V)
    G = 4096
    for rows in (1, 5, 64):
        x = (3.0 * rng.standard_normal((rows, V))).astype(np.float32)
        x[rows - 1, rng.integers(0, V, 500)] = -np.inf
        x[0, rng.integers(0, V, 50)] = np.nan
        x[0, 0] = np.nan
        x[rows - 1, eot - 1] = -np.inf
        for count in (1, 2, 88, 4096):
            ids = np.unique(np.concatenate([[0, eot - 1][:count], rng.choice(np.arange(1, eot - 1), max(0, count - 2), replace=False)])).astype(np.int32)
            assert len(ids) == count and ids[0] == 0 and (count == 1 or ids[-1] == eot - 1)
            flat = np.full(G + rows * V + G, np.nan, np.float32)
            flat.view(np.uint32)[:G] = 0x7FC00123                                # NaNs with a payload: a rewritten guard would lose it
            flat.view(np.uint32)[-G:] = 0x7FC00321
            flat[G:G + rows * V] = x.ravel()
            buf, ids_dev = dev(flat), dev(ids)
            body = C.c_void_p(buf.data_ptr() + 4 * G)
            binding.check(L.wh_op_suppress_logits(None, body, rows, V, ptr(ids_dev), 0))          # count 0: nothing is written
            torch.cuda.synchronize()
            assert np.array_equal(buf.cpu().numpy().view(np.uint32), flat.view(np.uint32))
            binding.check(L.wh_op_suppress_logits(None, body, rows, V, ptr(ids_dev), count))
            torch.cuda.synchronize()
            want = flat.copy()
            w = want[G:G + rows * V].reshape(rows, V)
            w[:, ids] = -np.inf
            assert np.array_equal(buf.cpu().numpy().view(np.uint32), want.view(np.uint32)), (rows, count)
    x = dev(np.zeros(8, np.float32))
    i = dev(np.zeros(2, np.int32))
    assert L.wh_op_suppress_logits(None, None, 1, 8, ptr(i), 1) != 0 and L.wh_op_suppress_logits(None, ptr(x), 0, 8, ptr(i), 1) != 0
    assert L.wh_op_suppress_logits(None, ptr(x), 1, 8, None, 1) != 0 and L.wh_op_suppress_logits(None, ptr(x), 1, 8, ptr(i), -1) != 0
    assert L.wh_op_suppress_logits(None, ptr(x), 1, 8, None, 0) == 0


# ---------------------------------------------------------------------------------------------------------------------
# context level
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def conditioned():
    hp = gf.hparams_for("test-d128-ml")
    ggml = gf.conditioned_model(gf.conditioned_layout(hp), 4, kind="test-d128-ml", seed=10)
    model = binding.HipModel.from_ggml(ggml)
    yield SimpleNamespace(hp=hp, ggml=ggml, model=model, sp=gf.special_tokens(hp))
    model.close()


def _mels(batch):
    rng = np.random.default_rng(17)
    return torch.from_numpy(rng.uniform(-1, 1, (batch, 80, 3000)).astype(np.float32)).cuda()


def _window(ctx, prompt, n_steps):
    ctx.decode_window_start(prompt, n_steps)
    data = ctx.decode_window_fetch_data(0, 1 + n_steps)
    ctx.decode_window_finish()
    return data


def _prompts(sp, batch):
    return np.array([[sp["prev"], 1000 + b, sp["sot"], sp["sot"] + 1, sp["transcribe"]] for b in range(batch)], np.int32)


def _prompts4(sp, batch):
    """The prompt length the conditioned model was built for: its first sample is a timestamp with p ~ 0.7 (behind the five-token prompt above every
    timestamp of the forced first sample has probability 0 and the pick is a tie: nothing to measure a margin on)."""
    return np.array([[sp["prev"], 1000 + b, sp["sot"], sp["sot"] + 1] for b in range(batch)], np.int32)


def _soft_max(logits):
    L = binding.lib()
    rows, V = logits.shape
    x = dev(logits)
    out = torch.full((rows, V), float("nan"), dtype=torch.float32, device="cuda")
    binding.check(L.wh_op_vocab_soft_max(None, ptr(x), ptr(out), rows, V))
    torch.cuda.synchronize()
    return out.cpu().numpy()


@pytest.mark.parametrize("batch,hyp", [(1, 1), (5, 1), (1, 5)])
def test_placement_behind_the_vocabulary_product(conditioned, batch, hyp):
    """One context, the same tokens, the set off, on and off again, a multi-token call (the prompt) and a single-token call (both decode paths of a batch of 1,
    the batched path at 5 rows, a hypothesis group of 5): logits_on = where( mask, -inf, logits_off ), probs_on = wh_op_vocab_soft_max( logits_on ), and the
    first run's bits come back when the set is turned off."""
    c, sp, V = conditioned, conditioned.sp, conditioned.hp.n_vocab
    seqs = batch * hyp
    ctx = binding.HipContext(c.model, batch, hypotheses=hyp)
    ctx.encode(_mels(batch))
    prompt = _prompts(sp, seqs)
    calls = [(prompt, 0), (np.full((seqs, 1), sp["beg"], np.int32), prompt.shape[1])]
    off = [ctx.decode(t, n) for t, n in calls]
    # the set: every seventh text token, ids 0 and eot - 1, and every row's own best text token -- what the softmax loses must matter
    ids = set(range(3, sp["eot"], 7)) | {0, sp["eot"] - 1}
    for lg, _ in off:
        ids |= {int(i) for i in np.argmax(lg[:, :sp["eot"]], axis=1)}
    ids = np.array(sorted(ids), np.int32)
    mask = np.zeros(V, bool)
    mask[ids] = True
    shuffled = np.concatenate([ids[::-1], ids[:5]])                              # unsorted, with duplicates: the context stores the sorted unique set
    ctx.set_suppress(shuffled)
    on = [ctx.decode(t, n) for t, n in calls]
    ctx.set_suppress(None)
    again = [ctx.decode(t, n) for t, n in calls]
    ctx.set_suppress([])
    for (l0, p0), (l1, p1), (l2, p2) in zip(off, on, again):
        assert np.isfinite(l0).all() and not np.array_equal(bits(p0), bits(p1))
        assert np.array_equal(bits(l1), bits(np.where(mask[None, :], np.float32(-np.inf), l0)))
        assert np.array_equal(bits(p1), bits(_soft_max(l1))) and (p1[:, ids] == 0).all() and abs(float(p1[0].sum()) - 1.0) < 1e-3
        assert np.array_equal(bits(l2), bits(l0)) and np.array_equal(bits(p2), bits(p0))
    ctx.close()


def test_detection_is_untouched(conditioned):
    """wh_lang_detect gives the same bits with and without a set -- a set that holds no language token cannot show it, so the set here is every text token
    below eot but one, which moves every probability of a filtered row -- and the decode that follows is filtered again."""
    c, sp, V = conditioned, conditioned.sp, conditioned.hp.n_vocab
    for batch, hyp in ((2, 1), (5, 1), (1, 5)):
        ctx = binding.HipContext(c.model, batch, hypotheses=hyp)
        ctx.encode(_mels(batch))
        p0, best0 = ctx.lang_detect()
        tokens = np.full((batch * hyp, 1), sp["sot"], np.int32)
        l_off, pr_off = ctx.decode(tokens, 0)
        ids = np.arange(1, sp["eot"], dtype=np.int32)
        ctx.set_suppress(ids)
        p1, best1 = ctx.lang_detect()
        assert np.array_equal(bits(p1), bits(p0)) and np.array_equal(best1, best0) and p0.shape == (batch, 99)
        l_on, pr_on = ctx.decode(tokens, 0)
        assert np.isneginf(l_on[:, ids]).all() and np.array_equal(bits(l_on[:, sp["eot"]:]), bits(l_off[:, sp["eot"]:]))
        lang = slice(sp["sot"] + 1, sp["sot"] + 100)
        assert not np.array_equal(bits(pr_on[::hyp, lang]), bits(p0))            # a filtered detection would have looked like this
        assert np.array_equal(bits(pr_off[::hyp, lang]), bits(p0))
        p2, best2 = ctx.lang_detect()
        assert np.array_equal(bits(p2), bits(p0)) and np.array_equal(best2, best0)
        ctx.close()


def _sample_best(probs, sp, force, initial):
    L = binding.lib()
    rows, V = probs.shape
    out = torch.zeros(rows * 5, dtype=torch.int32, device="cuda")
    pd = dev(probs)
    binding.check(L.wh_op_sample_best(None, ptr(pd), rows, V, sp["beg"], sp["sot"], sp["solm"], sp["not_"], int(force), int(initial), ptr(out)))
    torch.cuda.synchronize()
    return np.frombuffer(out.cpu().numpy().tobytes(), TOKEN_DT)


def _margins(row, sp, force, initial):
    """sampleBest's comparisons on an unfiltered row, each as a difference: timestamp mass against the best text token (when nothing is forced), and the pick
    against the runner-up among the tokens it was chosen from."""
    V, beg = len(row), sp["beg"]
    ts_end = min(beg + 101, V) if initial else V
    sum_ts = float(row[beg:ts_end].astype(np.float64).sum())
    tx = float(row[:beg].max())
    only_ts = force or sum_ts > tx
    cand = row.astype(np.float64).copy()
    cand[ts_end:] = -1
    if only_ts:
        cand[:beg] = -1
    for s in (sp["sot"], sp["solm"], sp["not_"]):
        cand[s] = -1
    top = np.sort(cand)[-2:]
    out = [top[1] - top[0]]
    if not force:
        out.append(abs(sum_ts - tx))
    return min(out), float(top[1])


@pytest.mark.parametrize("batch", [2, 5])
def test_greedy_loop(conditioned, batch):
    """wh_decode_window_start on the audio-conditioned model, graph replay and eager steps alike. S = the text tokens the unfiltered window emits: with S held
    none of them appears. Up to the first step k at which the unfiltered run picks a token of S, a row's ids are the unfiltered run's -- the unfiltered
    margins of sampleBest's comparisons at those steps are asserted to exceed 1e-3 of the pick's probability, so renormalising the row cannot flip one. At
    step k the pick is wh_op_sample_best's on the unfiltered row with S zeroed (5 rows: the fused sampler leaves the normalised row in "probs"; the spread
    sampler of 2 rows leaves e unnormalised, there the first two properties are checked). k must exist, or the test shows nothing."""
    c, sp, V = conditioned, conditioned.sp, conditioned.hp.n_vocab
    n_steps = 16
    prompt = _prompts4(sp, batch)
    ctx = binding.HipContext(c.model, batch)
    ctx.encode(_mels(batch))
    off = _window(ctx, prompt, n_steps)
    S = np.unique(off["id"][off["id"] < sp["eot"]]).astype(np.int32)
    in_s = np.isin(off["id"], S)
    assert len(S) >= 1 and in_s.any(axis=0).all()                                # every row emits text: k exists for each
    k = in_s.argmax(axis=0)                                                      # per row: the first step with a token of S
    assert (k >= 1).all()                                                        # ... and there are steps before it to compare
    ctx.set_suppress(S)
    runs = []
    for flags in (0, binding.WH_FLAG_NO_GRAPH, 0):
        ctx.set_flags(flags)
        runs.append(_window(ctx, prompt, n_steps))
    ctx.set_flags(0)
    on = runs[0]
    for f in FIELDS:
        assert np.array_equal(runs[1][f].view(np.uint32), on[f].view(np.uint32)), f
        assert np.array_equal(runs[2][f].view(np.uint32), on[f].view(np.uint32)), f
    assert not np.isin(on["id"], S).any() and not np.array_equal(on["id"], off["id"])
    for b in range(batch):
        assert np.array_equal(on["id"][:k[b], b], off["id"][:k[b], b]), b
    print("batch %d: |S| = %d, first step with a token of S per row: %s" % (batch, len(S), k.tolist()))
    if batch > 4:
        ctx.set_suppress(None)
        for j in range(int(k.max()) + 1):
            _window(ctx, prompt, j)                                              # exactly j + 1 samples: "probs" is the row of sample j
            rows = ctx.debug_read("probs", rows=batch)
            first = j == 0
            below = [b for b in range(batch) if j < k[b]]
            for b in below:
                margin, p = _margins(rows[b], sp, first, first)
                print("  row %d step %d: margin %.3e of p %.3e" % (b, j, margin, p))
                assert margin > 1e-3 * p, (b, j, margin, p)
            at = [b for b in range(batch) if j == k[b]]
            if at:
                zeroed = rows.copy()
                zeroed[:, S] = 0
                want = _sample_best(zeroed, sp, first, first)
                for b in at:
                    assert on["id"][j, b] == want["id"][b] and off["id"][j, b] in S, (b, j)
        again = _window(ctx, prompt, n_steps)
        for f in FIELDS:
            assert np.array_equal(again[f].view(np.uint32), off[f].view(np.uint32)), f
    ctx.close()


# The random-weight test-d128 model at the default weight scale has a row so flat that sampleBest's sum rule (the timestamps' mass, 1501 of 51864 columns,
# against the best single text token) makes EVERY draw a timestamp: no text token is ever drawn and a set of text tokens could show nothing. A weight scale
# of 0.3 spreads the logits (standard deviation ~ 3.4) far enough for the best text token to beat the timestamps' mass while thousands of tokens keep mass.
SAMPLING_W_STD = 0.3
SAMPLING_SEED, SAMPLING_NONCE = 2, 11                                           # measured with the set off: 22 of 201 drawn tokens in S, 190 text tokens
ROWS_SEED = 0xC0FFEE


@pytest.fixture(scope="module")
def random_weights():
    hp = gf.hparams_for("test-d128")
    model = binding.HipModel.from_ggml(gf.synth_model("test-d128", seed=31, w_std=SAMPLING_W_STD))
    yield SimpleNamespace(hp=hp, model=model, sp=gf.special_tokens(hp))
    model.close()


def test_sampling(random_weights):
    """wh_context_set_sampling( 1.0 ) on the random-weight model, S = every 12th id below eot, one window of 200 steps: with the set off at least 5 drawn
    tokens lie in S (asserted here: otherwise the test shows nothing), with it on none does, graph replay and eager steps alike."""
    c, sp = random_weights, random_weights.sp
    S = np.arange(0, sp["eot"], 12, dtype=np.int32)
    prompt = np.array([[sp["sot"]]], np.int32)
    n_steps = 200
    ctx = binding.HipContext(c.model, 1)
    ctx.encode(_mels(1))
    ctx.set_sampling(1.0, SAMPLING_SEED, SAMPLING_NONCE)
    off = _window(ctx, prompt, n_steps)
    n_in = int(np.isin(off["id"], S).sum())
    print("set off: %d of %d drawn tokens in S, %d text tokens, %d distinct ids" % (n_in, off["id"].size, int((off["id"] < sp["eot"]).sum()), len(np.unique(off["id"]))))
    assert n_in >= 5
    ctx.set_suppress(S)
    for flags in (0, binding.WH_FLAG_NO_GRAPH):
        ctx.set_flags(flags)
        on = _window(ctx, prompt, n_steps)
        assert not np.isin(on["id"], S).any() and (on["id"] < sp["eot"]).sum() >= 5
    ctx.set_flags(0)
    ctx.set_suppress(None)
    again = _window(ctx, prompt, n_steps)
    assert np.array_equal(again["id"], off["id"]) and np.array_equal(bits(again["p"]), bits(off["p"]))
    ctx.close()


def test_sampling_rows(random_weights):
    """The same through wh_context_set_sampling_rows with a mixed batch of 5: rows 0, 2 and 4 sampled at temperature 1, rows 1 and 3 greedy."""
    c, sp = random_weights, random_weights.sp
    S = np.arange(0, sp["eot"], 12, dtype=np.int32)
    batch, n_steps = 5, 200
    prompt = np.array([[sp["sot"]]] * batch, np.int32)
    temps = [1.0, 0.0, 1.0, 0.0, 1.0]
    ctx = binding.HipContext(c.model, batch)
    ctx.encode(_mels(batch))
    ctx.set_sampling_rows(temps, [ROWS_SEED + b for b in range(batch)], [SAMPLING_NONCE] * batch)
    off = _window(ctx, prompt, n_steps)
    sampled = [b for b in range(batch) if temps[b] > 0]
    n_in = [int(np.isin(off["id"][:, b], S).sum()) for b in range(batch)]
    print("set off: drawn tokens in S per row", n_in)
    assert sum(n_in[b] for b in sampled) >= 5
    ctx.set_suppress(S)
    on = _window(ctx, prompt, n_steps)
    assert not np.isin(on["id"], S).any()
    ctx.set_sampling_rows(None)
    greedy_on = _window(ctx, prompt, n_steps)                                    # all rows greedy, the set still held
    assert not np.isin(greedy_on["id"], S).any()
    ctx.close()


def test_refusals(conditioned):
    c, sp = conditioned, conditioned.sp
    ctx = binding.HipContext(c.model, 1)
    for bad in ([sp["eot"]], [-1], [5, sp["beg"]], [conditioned.hp.n_vocab]):
        with pytest.raises(binding.WhisperHipError):
            ctx.set_suppress(bad)
    ctx.set_suppress([5, sp["eot"] - 1, 0])
    with pytest.raises(binding.WhisperHipError):
        ctx.set_flags(binding.WH_FLAG_PARITY_EXACT, 2)                           # the exact mode over a held set
    ctx.set_flags(0)
    ctx.set_suppress(None)
    ctx.set_flags(binding.WH_FLAG_PARITY_EXACT, 2)
    with pytest.raises(binding.WhisperHipError):
        ctx.set_suppress([5])                                                    # a non-empty set under the exact mode
    ctx.set_suppress([])                                                         # an empty one is the state it is in
    ctx.set_flags(0)
    ctx.set_suppress([5])
    ctx.close()


# ---------------------------------------------------------------------------------------------------------------------
# the library
# ---------------------------------------------------------------------------------------------------------------------
def _pcm(seconds, tone, seed):
    t = np.arange(int(seconds * 16000)) / 16000.0
    rng = np.random.default_rng(seed)
    return (0.25 * np.sin(2 * np.pi * tone * t) * (1 + 0.6 * np.sin(2 * np.pi * 2.5 * t)) + 0.05 * rng.standard_normal(len(t))).astype(np.float32)


def _strip(segs):
    return [(s["t0"], s["t1"], s["text"], [(t["id"], t["p"], t["pt"], t["ptsum"]) for t in s["tokens"]]) for s in segs]


def _ids(segs):
    return [t["id"] for s in segs for t in s["tokens"]]


RECORDINGS = ((40, 330, 7), (65, 440, 8), (45, 250, 9), (35, 520, 10), (50, 390, 11), (38, 300, 12))      # seconds, tone, seed


@pytest.fixture(scope="module")
def library(conditioned, tmp_path_factory):
    from whisper_amd import api
    path = str(tmp_path_factory.mktemp("sup") / "cond.bin")
    gf.write_model(path, conditioned.ggml)
    model = api.Model(path)
    pcms = [_pcm(*r) for r in RECORDINGS]
    kw = dict(language="en", prompt=[1000], n_max_text_ctx=0, flags=api.NO_CONTEXT)
    ctx = model.create_context()
    off = []
    for pcm in pcms:
        assert ctx.run_full(pcm, **kw) == 0
        off.append(ctx.results())
    eot = model.special_tokens()["eot"]
    S = sorted({i for segs in off for i in _ids(segs) if i < eot})
    assert len(S) >= 4
    yield SimpleNamespace(api=api, path=path, model=model, pcms=pcms, kw=kw, ctx=ctx, off=off, S=S, eot=eot)
    ctx.close()
    model.close()


def test_library_context(library):
    """Context.set_suppress_tokens( S ), S = the text tokens of the unfiltered transcripts: run_full and run_streamed emit none of them and differ from the
    unfiltered transcripts; None and [] give back results identical in every field to a context on which the call was never made."""
    lb = library
    fresh = lb.model.create_context()
    lb.ctx.set_suppress_tokens(lb.S)
    on = []
    for pcm, off in zip(lb.pcms[:3], lb.off):
        assert lb.ctx.run_full(pcm, **lb.kw) == 0
        got = lb.ctx.results()
        on.append(_strip(got))
        assert not set(_ids(got)) & set(lb.S) and _strip(got) != _strip(off) and len(got) >= 1
        hr, _ = lb.ctx.run_streamed(pcm, **lb.kw)
        streamed = lb.ctx.results()
        assert hr == 0 and not set(_ids(streamed)) & set(lb.S) and len(streamed) >= 1
        hr, _ = fresh.run_streamed(pcm, **lb.kw)
        assert hr == 0 and _strip(streamed) != _strip(fresh.results())
    for clear in (None, []):
        lb.ctx.set_suppress_tokens(lb.S)
        lb.ctx.set_suppress_tokens(clear)
        for pcm, off in zip(lb.pcms[:2], lb.off):
            assert lb.ctx.run_full(pcm, **lb.kw) == 0 and _strip(lb.ctx.results()) == _strip(off)
            assert fresh.run_full(pcm, **lb.kw) == 0 and _strip(fresh.results()) == _strip(off)
    fresh.close()
    # refusals through the library: an id at eot, a negative one
    for bad in ([lb.eot], [3, -1]):
        with pytest.raises(lb.api.WhisperError):
            lb.ctx.set_suppress_tokens(bad)
    # a suppressed id in the prompt is legal: prompt tokens are fed, not sampled
    lb.ctx.set_suppress_tokens([1000] + lb.S)
    assert lb.ctx.run_full(lb.pcms[0], **lb.kw) == 0 and _strip(lb.ctx.results()) == on[0]
    # the exact mode cannot be turned on over a held set, nor a set given under the exact mode
    with pytest.raises(lb.api.WhisperError):
        lb.ctx.set_device_flags(binding.WH_FLAG_PARITY_EXACT, 2)
    lb.ctx.set_suppress_tokens(None)
    lb.ctx.set_device_flags(binding.WH_FLAG_PARITY_EXACT, 2)
    with pytest.raises(lb.api.WhisperError):
        lb.ctx.set_suppress_tokens(lb.S)
    lb.ctx.set_device_flags(0, 1)


def test_library_language_auto_detects_as_before(library):
    lb = library
    kw = dict(lb.kw, language="auto")
    assert lb.ctx.run_full(lb.pcms[0], **kw) == 0
    before, seen = lb.ctx.detected_language, _strip(lb.ctx.results())
    lb.ctx.set_suppress_tokens(list(range(1, lb.eot)))
    try:
        assert lb.ctx.run_full(lb.pcms[0], **kw) == 0
        assert lb.ctx.detected_language == before and before is not None and _strip(lb.ctx.results()) != seen
    finally:
        lb.ctx.set_suppress_tokens(None)


def test_library_fallback_through_all_six_temperatures(library):
    """logprob_thold = +1 forces every window through six attempts, the last at temperature 1.0: window_stats shows them, and no token of S is in the result."""
    lb = library
    lb.ctx.set_fallback(temperature_inc=0.2, logprob_thold=1.0, entropy_thold=-1.0, no_speech_thold=2.0, seed=5)
    try:
        assert lb.ctx.run_full(lb.pcms[0], **lb.kw) == 0
        plain = _strip(lb.ctx.results())
        lb.ctx.set_suppress_tokens(lb.S)
        assert lb.ctx.run_full(lb.pcms[0], **lb.kw) == 0
        got, stats = lb.ctx.results(), lb.ctx.window_stats()
        assert len(stats) >= 1 and all(w["attempts"] == 6 for w in stats)
        assert not set(_ids(got)) & set(lb.S) and _strip(got) != plain
    finally:
        lb.ctx.set_suppress_tokens(None)
        lb.ctx.set_fallback(None)


def test_library_beam(library):
    """run_full( beam_width = 5 ) with the set: no id of S in any segment; width 1 with the set equals the greedy run with the same set, token for token."""
    lb = library
    key = lambda segs: [(s["t0"], s["t1"], [t["id"] for t in s["tokens"]]) for s in segs]
    assert lb.ctx.run_full(lb.pcms[0], beam_width=5, **lb.kw) == 0
    plain5 = key(lb.ctx.results())
    lb.ctx.set_suppress_tokens(lb.S)                                             # the hypothesis-group contexts exist already: they are told
    try:
        assert lb.ctx.run_full(lb.pcms[0], **lb.kw) == 0
        greedy = key(lb.ctx.results())
        assert lb.ctx.run_full(lb.pcms[0], beam_width=1, **lb.kw) == 0            # a context created AFTER the call: it is told as well
        assert key(lb.ctx.results()) == greedy
        for pcm in lb.pcms[:2]:
            assert lb.ctx.run_full(pcm, beam_width=5, **lb.kw) == 0
            got = lb.ctx.results()
            assert not set(_ids(got)) & set(lb.S) and len(got) >= 1
        assert lb.ctx.run_full(lb.pcms[0], beam_width=5, **lb.kw) == 0 and key(lb.ctx.results()) != plain5
    finally:
        lb.ctx.set_suppress_tokens(None)
    assert lb.ctx.run_full(lb.pcms[0], beam_width=5, **lb.kw) == 0 and key(lb.ctx.results()) == plain5


def test_library_batch_runner(library):
    """BatchRunner.set_suppress_tokens( S ) with 5 slots and 6 streams: every stream's result equals Context.run_full of that stream with the same set -- ids,
    times and probabilities, the runner's standing contract -- also while neighbours retry under the batch fallback; None and [] give the results of a runner
    on which the call was never made."""
    lb = library
    kw = dict(lb.kw, flags=lb.api.NO_CONTEXT | lb.api.SINGLE_SEGMENT)
    runner = lb.model.create_batch_runner(max_slots=5, groups=1)
    hr, never, per = runner.run(lb.pcms, **kw)
    assert hr == 0 and all(p == 0 for p in per)
    never = [_strip(s) for s in never]
    lb.ctx.set_suppress_tokens(lb.S)
    single = []
    for pcm in lb.pcms:
        assert lb.ctx.run_full(pcm, **kw) == 0
        single.append(lb.ctx.results())
    lb.ctx.set_suppress_tokens(None)
    runner.set_suppress_tokens(lb.S)
    hr, got, per = runner.run(lb.pcms, **kw)
    assert hr == 0 and all(p == 0 for p in per)
    for i, (g, s) in enumerate(zip(got, single)):
        assert not set(_ids(g)) & set(lb.S) and _strip(g) != never[i], i
        assert [(x["t0"], x["t1"], x["text"], [t["id"] for t in x["tokens"]]) for x in g] == [(x["t0"], x["t1"], x["text"], [t["id"] for t in x["tokens"]]) for x in s], i
        pg = np.array([t["p"] for x in g for t in x["tokens"]])
        ps = np.array([t["p"] for x in s for t in x["tokens"]])
        assert np.abs(pg - ps).max() < 2e-2, i                                   # batch-versus-single probabilities: what tests/test_batch_api.py grants
    # neighbours retry under the batch fallback (a threshold midway between the streams' worst windows): the others keep the transcripts above
    runner.set_fallback(logprob_thold=-1e30, entropy_thold=-1.0, no_speech_thold=2.0)
    hr, _, _ = runner.run(lb.pcms, **kw)
    lowest = sorted((min(x["avg_logprob"] for x in w), i) for i, w in enumerate(runner.window_stats))
    mid = len(lowest) // 2
    thold = 0.5 * (lowest[mid - 1][0] + lowest[mid][0])
    runner.set_fallback(temperature_inc=0.5, logprob_thold=thold, entropy_thold=-1.0, no_speech_thold=2.0, seed=9)
    hr, retried, _ = runner.run(lb.pcms, **kw)
    stats = runner.window_stats
    runner.set_fallback(None)
    assert hr == 0 and any(x["attempts"] > 1 for w in stats for x in w)
    for i, g in enumerate(retried):
        assert not set(_ids(g)) & set(lb.S), i
        if all(x["attempts"] == 1 for x in stats[i]):
            assert _strip(g) == _strip(got[i]), i
    for clear in (None, []):
        runner.set_suppress_tokens(lb.S)
        runner.set_suppress_tokens(clear)
        hr, back, _ = runner.run(lb.pcms, **kw)
        assert hr == 0 and [_strip(s) for s in back] == never
    with pytest.raises(lb.api.WhisperError):
        runner.set_suppress_tokens([lb.eot])
    runner.close()


def test_non_speech_set_and_whisper_main(tmp_path, conditioned):
    """Model.non_speech_tokens() on a model file with a planted vocabulary equals the CPU test's expectation, "non_speech" resolves to it, the flat C entry
    answers E_BOUNDS for too small a buffer, and whisper-main -sns / --suppress-nst writes the transcript of the library run with that set (and without the
    option the unfiltered one, which differs); -h does not mention the option."""
    import wave
    import test_suppress_cpu as T
    from whisper_amd import api, build
    hp, words, eot, hits = T.planted_vocabulary("test-d128-ml")
    q = np.clip(np.round(_pcm(40, 330, 7) * 32768.0), -32768, 32767).astype("<i2")
    pcm = q.astype(np.float32) / 32768.0                                         # what the tool reads from the 16-bit file
    # which text tokens does this model emit? Plant non-speech strings exactly there, so that the set changes the transcript
    path0 = str(tmp_path / "plain.bin")
    gf.write_model(path0, conditioned.ggml)
    m0 = api.Model(path0)
    c0 = m0.create_context()
    assert c0.run_full(pcm) == 0
    emitted = sorted({i for i in _ids(c0.results()) if 256 <= i < eot and not 300 <= i <= 312 and i not in hits})
    c0.close()
    m0.close()
    assert len(emitted) >= 2
    for i, w in zip(emitted[::2], (" ♪", " [", "((", " (", " ♪♪", " \"")):
        words[i] = w.encode()
    g = conditioned.ggml
    path = str(tmp_path / "planted.bin")
    gf.write_model(path, gf.GgmlModel(g.hparams, g.filters, words, g.tensors))
    want = T.expected(words, eot)
    m = api.Model(path)
    assert m.non_speech_tokens() == want and set(emitted[::2][:6]) <= set(want)
    n = C.c_uint32(0)
    small = (C.c_int32 * 4)()
    assert api.lib().whisperc_non_speech_tokens(m.h, small, 4, C.byref(n)) & 0xFFFFFFFF == 0x8000000B and n.value == len(want)
    assert api.lib().whisperc_non_speech_tokens(m.h, None, 0, C.byref(n)) == 0 and n.value == len(want)
    ctx = m.create_context()
    assert ctx.run_full(pcm) == 0
    plain = [s["text"] for s in ctx.results()]
    ctx.set_suppress_tokens("non_speech")
    assert ctx.run_full(pcm) == 0
    got = ctx.results()
    texts = [s["text"] for s in got]
    assert not set(_ids(got)) & set(want) and texts != plain and len(texts) >= 1
    ctx.set_suppress_tokens(want)
    assert ctx.run_full(pcm) == 0 and [s["text"] for s in ctx.results()] == texts
    ctx.close()
    m.close()

    wav = str(tmp_path / "rec.wav")
    with wave.open(wav, "wb") as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(16000)
        w.writeframes(q.tobytes())

    def tool(*extra):
        r = subprocess.run([build.CLI_BIN, "-m", path, "-f", wav, "-l", "en", "-nc"] + list(extra), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
        assert r.returncode == 0, r.stderr.decode(errors="replace")[-2000:]
        return [ln.split(b"]  ", 1)[1] for ln in r.stdout.splitlines() if b"]  " in ln]

    with_sns, with_long, without = tool("-sns"), tool("--suppress-nst"), tool()
    assert with_sns == texts and with_long == texts and without == plain
    usage = subprocess.run([build.CLI_BIN, "-h"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=60)
    assert "-sns" not in usage.stdout + usage.stderr and "suppress" not in usage.stdout + usage.stderr
