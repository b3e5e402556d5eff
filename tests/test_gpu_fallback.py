"""GPU tests of the decoding fallback, against the float64 restatement of tests/fallback_ref.py:

  * wh_op_vocab_soft_max_scaled: the bits of wh_op_vocab_soft_max on host-scaled logits, both kernels;
  * wh_op_philox_u: the restatement's numbers exactly;
  * wh_op_sample_draw: the restatement's token on rows built for every branch (tests/test_fallback_cpu.py shows on the CPU that none of these draws lies
    within 1e-10 W of a prefix boundary, so none is left out), tid / pt / ptsum with wh_op_sample_best's bits, and the counts on a 4-token row;
  * wh_context_set_sampling: the device-side loop with and without the captured graph equals a host-stepped replay through the op entry points, below and
    above the row count at which the decode path changes; back at temperature 0 the greedy tokens return; wh_decode_window_no_speech; the refusals;
  * the library: Context.set_fallback / window_stats through runFull.
"""
import ctypes as C
import math
from types import SimpleNamespace

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import fallback_ref as F  # noqa: E402
from whisper_amd import binding, ggml_format as gf  # noqa: E402

pytestmark = pytest.mark.gpu

TOKEN_DT = np.dtype([("id", "<i4"), ("tid", "<i4"), ("p", "<f4"), ("pt", "<f4"), ("ptsum", "<f4")])
E_NOTIMPL = 0x80004001


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def ptr(t):
    return C.c_void_p(t.data_ptr())


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---------------------------------------------------------------------------------------------------------------------
# op level
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cols", [1000, 51865, 51866, 52225])
def test_scaled_soft_max_equals_the_soft_max_of_host_scaled_logits(cols):
    """Bit for bit, rows 1 and 3, invT 5, 1 and 1 / 0.6, rows with -inf entries; 52225 columns take the three-pass kernel, and so does every width with
    beam_regs 0."""
    L = binding.lib()
    rng = np.random.default_rng(cols)
    for rows in (1, 3):
        x = (3.0 * rng.standard_normal((rows, cols))).astype(np.float32)
        x[rows - 1, rng.integers(0, cols, cols // 9)] = -np.inf
        x[0, cols - 1] = 9.0
        xd = dev(x)
        for inv_t in (np.float32(5.0), np.float32(1.0), np.float32(1.0) / np.float32(0.6)):
            scaled = dev(x * inv_t)                                              # float32 * float32: each product rounded once
            for regs in (1, 0):
                binding.set_option("beam_regs", regs)
                try:
                    want = torch.full((rows, cols), float("nan"), dtype=torch.float32, device="cuda")
                    got = torch.full((rows, cols), float("nan"), dtype=torch.float32, device="cuda")
                    binding.check(L.wh_op_vocab_soft_max(None, ptr(scaled), ptr(want), rows, cols))
                    binding.check(L.wh_op_vocab_soft_max_scaled(None, ptr(xd), float(inv_t), ptr(got), rows, cols))
                    torch.cuda.synchronize()
                finally:
                    binding.set_option("beam_regs", binding.OPTION_DEFAULTS["beam_regs"])
                g, w = got.cpu().numpy(), want.cpu().numpy()
                assert np.isfinite(g).all() and (g[np.isneginf(x)] == 0).all() and abs(float(g.sum(1)[0]) - 1.0) < 1e-3
                assert np.array_equal(bits(g), bits(w)), (rows, cols, float(inv_t), regs)
        assert np.array_equal(bits(xd.cpu().numpy()), bits(x)), "the input was written"
    p = dev(np.zeros(8, np.float32))
    assert L.wh_op_vocab_soft_max_scaled(None, None, 1.0, ptr(p), 1, 8) != 0 and L.wh_op_vocab_soft_max_scaled(None, ptr(p), 1.0, ptr(p), 0, 8) != 0


def test_philox_u_equals_the_restatement():
    L = binding.lib()
    rng = np.random.default_rng(3)
    for rows, seed, nonce in ((1, 0, 0), (1000, 0x0123456789ABCDEF, 0xFFFFFFFF), (257, 2 ** 64 - 1, 7)):
        pos = rng.integers(0, 2 ** 31 - 1, rows).astype(np.int32)
        pos[0] = 0
        out = torch.full((rows,), -1.0, dtype=torch.float64, device="cuda")
        pos_dev = dev(pos)
        binding.check(L.wh_op_philox_u(None, seed, nonce, rows, ptr(pos_dev), ptr(out)))
        torch.cuda.synchronize()
        want = F.uniforms(seed, nonce, pos)
        assert np.array_equal(out.cpu().numpy(), want) and (want >= 0).all() and (want < 1).all()
    assert L.wh_op_philox_u(None, 1, 1, 0, ptr(out), ptr(out)) != 0 and L.wh_op_philox_u(None, 1, 1, 4, None, ptr(out)) != 0


def _tokens(fn, probs_dev, rows, V, sp, force, initial, extra=()):
    out = torch.zeros(rows * 5, dtype=torch.int32, device="cuda")
    binding.check(fn(None, ptr(probs_dev), rows, V, sp["beg"], sp["sot"], sp["solm"], sp["not_"], int(force), int(initial), *extra, ptr(out)))
    torch.cuda.synchronize()
    return np.frombuffer(out.cpu().numpy().tobytes(), TOKEN_DT)


@pytest.mark.parametrize("V", [51865, 51866])
def test_sample_draw_against_the_restatement(V):
    """Every kind of row alone (1 row), then 5 and 64 rows, the four flag combinations: the restatement's token, p = probs[ id ], and tid / pt / ptsum with
    wh_op_sample_best's bits; where nothing is allowed (W == 0) wh_op_sample_best's own token. A draw may be left out only within 1e-10 W of a prefix
    boundary (an FP64 sum of 52 k non-negative terms moves by less than 5.8e-12 relative with its order), at most 1 % of them; these seeds leave out none."""
    L = binding.lib()
    sp = gf.special_tokens(SimpleNamespace(n_vocab=V))
    n = left_out = drawn = 0
    for kinds, probs, positions in F.draw_batches(V, sp):
        rows = len(kinds)
        pd, posd = dev(probs), dev(positions)
        u = F.uniforms(F.DRAW_SEED, F.DRAW_NONCE, positions)
        for force in (0, 1):
            for initial in (0, 1):
                got = _tokens(L.wh_op_sample_draw, pd, rows, V, sp, force, initial, (F.DRAW_SEED, F.DRAW_NONCE, ptr(posd)))
                best = _tokens(L.wh_op_sample_best, pd, rows, V, sp, force, initial)
                for k in ("tid", "pt", "ptsum"):
                    assert np.array_equal(got[k].view(np.uint32), best[k].view(np.uint32)), (k, kinds, force, initial)
                for r in range(rows):
                    where = (V, kinds[r], rows, r, force, initial)
                    tok, margin = F.draw(probs[r], sp["beg"], sp["sot"], sp["solm"], sp["not_"], force, initial, u[r])
                    n += 1
                    if tok is None:
                        assert got["id"][r] == best["id"][r] and bits(got["p"][r]) == bits(best["p"][r]), where
                        continue
                    drawn += 1
                    if margin < 1e-10:
                        left_out += 1
                        continue
                    assert got["id"][r] == tok, where + (int(got["id"][r]), tok, margin)
                    assert bits(got["p"][r]) == bits(probs[r][tok]), where
    print("V %d: %d draws, %d with an allowed token, %d left out" % (V, n, drawn, left_out))
    assert left_out <= 0.01 * drawn and left_out == 0 and drawn > 100
    # bad arguments
    p = dev(np.zeros(16, np.float32))
    pos = dev(np.zeros(2, np.int32))
    out = dev(np.zeros(10, np.int32))
    assert L.wh_op_sample_draw(None, ptr(p), 1, 16, 8, 1, 2, 3, 0, 0, 1, 1, None, ptr(out)) != 0                      # no positions
    assert L.wh_op_sample_draw(None, ptr(p), 1, 8, 8, 1, 2, 3, 0, 0, 1, 1, ptr(pos), ptr(out)) != 0                  # no timestamp token
    assert L.wh_op_sample_draw(None, ptr(p), 1, 65537, 8, 1, 2, 3, 0, 0, 1, 1, ptr(pos), ptr(out)) != 0              # more than 65536 columns


def test_sample_draw_counts_on_a_four_token_row():
    """4096 rows of (0.5, 0.25, 0.125, 0.125), one position each: the device's tokens are the restatement's, row by row, hence its counts."""
    L = binding.lib()
    row = np.zeros(8, np.float32)
    row[:4] = (0.5, 0.25, 0.125, 0.125)
    rows = 4096
    sp = dict(beg=7, sot=4, solm=5, not_=6)
    positions = np.arange(rows, dtype=np.int32)
    probs_dev, pos_dev = dev(np.tile(row, (rows, 1))), dev(positions)
    got = _tokens(L.wh_op_sample_draw, probs_dev, rows, 8, sp, 0, 0, (1234, 7, ptr(pos_dev)))
    want = np.array([F.draw(row, 7, 4, 5, 6, 0, 0, F.uniform(1234, 7, int(pos), r))[0] for r, pos in enumerate(positions)])
    assert np.array_equal(got["id"], want)
    counts = np.bincount(got["id"], minlength=4)
    print("counts", counts)
    assert np.array_equal(counts, np.bincount(want, minlength=4)) and counts.sum() == rows and len(counts) == 4


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


@pytest.fixture(scope="module")
def random_weights():
    hp = gf.hparams_for("test-d128-ml")
    model = binding.HipModel.from_ggml(gf.synth_model("test-d128-ml", seed=31))
    yield SimpleNamespace(hp=hp, model=model, sp=gf.special_tokens(hp))
    model.close()


@pytest.mark.parametrize("weights", ["random", "conditioned"])
@pytest.mark.parametrize("batch", [2, 5])
def test_sampling_context_equals_a_host_stepped_replay(conditioned, random_weights, batch, weights):
    """After wh_encode of `batch` windows: 12 steps at T = 0.8 through wh_decode_window_start, with and without WH_FLAG_NO_GRAPH, equal
    wh_decode -> wh_op_vocab_soft_max_scaled -> wh_op_sample_draw with the same seed, nonce and position (the position of the token just fed). 2 rows take the
    single-stream decode path and the host mailbox, 5 rows (one above SMALL_MAX_ROWS) the batched path and the event fetch. Nothing is encoded again between
    the attempts: the window's caches stay valid. Back at temperature 0 the greedy tokens are those from before. Two models: random weights (a broad
    distribution, every sample a timestamp by the sum rule) and an audio-conditioned one (text between timestamps)."""
    L = binding.lib()
    c = random_weights if weights == "random" else conditioned
    sp, V = c.sp, c.hp.n_vocab
    n_steps, T, seed, nonce = 12, 0.8, 0xDEADBEEFCAFE, 24 * 8 + 3
    prompt = np.array([[sp["prev"], 1000 + b, sp["sot"], sp["sot"] + 1, sp["transcribe"]] for b in range(batch)], np.int32)
    n_prompt = prompt.shape[1]
    ctx = binding.HipContext(c.model, batch)
    ctx.encode(_mels(batch))
    greedy = _window(ctx, prompt, n_steps)

    ctx.set_sampling(T, seed, nonce)
    runs = []
    for flags in (0, binding.WH_FLAG_NO_GRAPH, 0):
        ctx.set_flags(flags)
        runs.append(_window(ctx, prompt, n_steps))
    ctx.set_flags(0)
    for k in ("id", "tid", "p", "pt", "ptsum"):
        assert np.array_equal(runs[0][k], runs[1][k]) and np.array_equal(runs[0][k], runs[2][k]), k
    print("%s, %d rows: %d of %d tokens differ from the greedy ones" % (weights, batch, int((runs[0]["id"] != greedy["id"]).sum()), greedy["id"].size))
    if weights == "random":
        assert not np.array_equal(runs[0]["id"], greedy["id"])                   # the temperature reached the loop
        assert len({tuple(runs[0]["id"][:, b]) for b in range(batch)}) > 1       # rows draw their own numbers

    # host-stepped replay through the op entry points
    inv_t = float(np.float32(1.0) / np.float32(T))
    probs = torch.empty((batch, V), dtype=torch.float32, device="cuda")
    want_id, want_p = [], []
    tokens, n_past = prompt, 0
    for s in range(1 + n_steps):
        logits, _ = ctx.decode(tokens, n_past, want_probs=False)
        logits_dev = dev(logits)
        binding.check(L.wh_op_vocab_soft_max_scaled(None, ptr(logits_dev), inv_t, ptr(probs), batch, V))
        pos = dev(np.full(batch, n_prompt - 1 + s, np.int32))
        first = int(s == 0)
        tok = _tokens(L.wh_op_sample_draw, probs, batch, V, sp, first, first, (seed, nonce, ptr(pos)))
        want_id.append(tok["id"].copy())
        want_p.append(tok["p"].copy())
        n_past += tokens.shape[1]
        tokens = tok["id"].astype(np.int32)[:, None]
    assert np.array_equal(runs[0]["id"], np.stack(want_id))
    assert np.array_equal(bits(runs[0]["p"]), bits(np.stack(want_p)))

    # another nonce: other draws from the same graph; temperature 0: the greedy tokens from before
    ctx.set_sampling(T, seed, nonce + 1)
    other = _window(ctx, prompt, n_steps)
    assert weights != "random" or not np.array_equal(other["id"], runs[0]["id"])
    ctx.set_sampling(0.0)
    again = _window(ctx, prompt, n_steps)
    for k in ("id", "tid", "p", "pt", "ptsum"):
        assert np.array_equal(again[k], greedy[k]), k
    ctx.close()


def test_no_speech_probability_and_refusals(conditioned):
    c, sp, V = conditioned, conditioned.sp, conditioned.hp.n_vocab
    L = binding.lib()
    for batch in (2, 5):
        prompt = np.array([[sp["sot"], sp["sot"] + 1 + b, sp["transcribe"]] for b in range(batch)], np.int32)
        ctx = binding.HipContext(c.model, batch)
        ctx.encode(_mels(batch))
        ctx.decode_window_start(prompt, 2)
        with pytest.raises(binding.WhisperHipError):
            ctx.window_no_speech(batch)                                          # not turned on
        ctx.decode_window_finish()
        ctx.set_no_speech(True)
        ctx.decode_window_start(prompt, 6)
        got = ctx.window_no_speech(batch)
        ctx.decode_window_finish()
        logits, probs = ctx.decode(prompt, 0)
        assert np.array_equal(bits(got), bits(probs[:, sp["solm"]])), (got, probs[:, sp["solm"]])
        assert (got > 0).all() and len(set(got.tolist())) == batch
        # at a temperature the step's own (tempered) row is what is read
        ctx.set_sampling(0.5, 1, 2)
        ctx.decode_window_start(prompt, 1)
        hot = ctx.window_no_speech(batch)
        ctx.decode_window_finish()
        want = torch.empty((batch, V), dtype=torch.float32, device="cuda")
        logits_dev = dev(logits)
        binding.check(L.wh_op_vocab_soft_max_scaled(None, ptr(logits_dev), 2.0, ptr(want), batch, V))
        torch.cuda.synchronize()
        assert np.array_equal(bits(hot), bits(want.cpu().numpy()[:, sp["solm"]]))
        ctx.set_sampling(0.0)
        ctx.set_no_speech(False)
        ctx.decode_window_start(prompt, 1)
        with pytest.raises(binding.WhisperHipError):
            ctx.window_no_speech(batch)
        ctx.decode_window_finish()
        ctx.close()

    # the spread sampler (TUNE_SAMPLE_SPREAD, not the default) leaves unnormalised exponentials in the row: the gather normalises with the sampler's own sum
    L.wh_debug_set_tuning(binding.TUNE_DEFAULT | binding.TUNE_SAMPLE_SPREAD)
    try:
        prompt = np.array([[sp["sot"], sp["sot"] + 1 + b, sp["transcribe"]] for b in range(2)], np.int32)
        ctx = binding.HipContext(c.model, 2)
        ctx.encode(_mels(2))
        ctx.set_no_speech(True)
        ctx.decode_window_start(prompt, 3)
        got = ctx.window_no_speech(2)
        ctx.decode_window_finish()
        _, probs = ctx.decode(prompt, 0)
        assert np.array_equal(bits(got), bits(probs[:, sp["solm"]])), (got, probs[:, sp["solm"]])
        ctx.close()
    finally:
        L.wh_debug_set_tuning(binding.TUNE_DEFAULT)

    ctx = binding.HipContext(c.model, 1)
    for bad in (-0.5, float("nan"), 4.5, float("inf")):
        with pytest.raises(binding.WhisperHipError):
            ctx.set_sampling(bad)
    ctx.set_sampling(4.0)
    ctx.set_sampling(0.0)
    ctx.set_flags(binding.WH_FLAG_PARITY_EXACT)
    with pytest.raises(binding.WhisperHipError):
        ctx.set_sampling(0.5)
    ctx.set_flags(0)
    ctx.close()
    hyp = binding.HipContext(c.model, 1, hypotheses=2)
    with pytest.raises(binding.WhisperHipError):
        hyp.set_sampling(0.5)
    hyp.close()


# ---------------------------------------------------------------------------------------------------------------------
# library
# ---------------------------------------------------------------------------------------------------------------------
def _pcm():
    t = np.arange(40 * 16000) / 16000.0
    rng = np.random.default_rng(7)
    return (0.25 * np.sin(2 * np.pi * 330 * t) * (1 + 0.6 * np.sin(2 * np.pi * 2.5 * t)) + 0.05 * rng.standard_normal(len(t))).astype(np.float32)


def _strip(segs):
    return [(s["t0"], s["t1"], s["text"], [(t["id"], t["p"], t["pt"], t["ptsum"]) for t in s["tokens"]]) for s in segs]


def test_library_fallback(conditioned, tmp_path):
    from whisper_amd import api
    path = str(tmp_path / "cond.bin")
    gf.write_model(path, conditioned.ggml)
    model = api.Model(path)
    ctx = model.create_context()
    pcm = _pcm()
    kw = dict(language="en", prompt=[1000], n_max_text_ctx=0, flags=api.NO_CONTEXT | api.SINGLE_SEGMENT)
    inf = float("inf")

    assert ctx.run_full(pcm, **kw) == 0
    plain = _strip(ctx.results())
    assert len(plain) >= 2 and ctx.window_stats() == []

    # gates that nothing can fail: the plain run, one attempt per window
    ctx.set_fallback(logprob_thold=-inf, entropy_thold=-inf)
    assert ctx.run_full(pcm, **kw) == 0
    stats = ctx.window_stats()
    assert _strip(ctx.results()) == plain
    assert len(stats) >= len(plain) and all(w["attempts"] == 1 and w["temperature"] == 0 and not w["skipped"] for w in stats)
    assert all(0 <= w["no_speech"] < 1 for w in stats)                          # (a peaked row can round it to 0)

    # gates that everything fails, and no silence: six attempts per window, the last at temperature 1.0; a function of the seed
    def hot(seed):
        ctx.set_fallback(logprob_thold=inf, no_speech_thold=2.0, seed=seed)
        assert ctx.run_full(pcm, **kw) == 0
        return ctx.results(), ctx.window_stats()
    res_a, stats_a = hot(5)
    res_b, stats_b = hot(5)
    res_c, _ = hot(6)
    assert _strip(res_a) == _strip(res_b) and stats_a == stats_b and _strip(res_a) != _strip(res_c)
    assert len(stats_a) >= 2 and all(w["attempts"] == 6 and w["temperature"] == 1.0 and not w["skipped"] for w in stats_a)
    # SingleSegment: a window's segment holds exactly the tokens that were scored; every segment must be some window's, in order
    windows = iter(stats_a)
    for seg in res_a:
        avg, ent = F.score([(t["id"], t["p"]) for t in seg["tokens"]], len(seg["tokens"]))
        assert any(math.isclose(w["avg_logprob"], avg, rel_tol=1e-12) and math.isclose(w["entropy"], ent, rel_tol=1e-12, abs_tol=1e-15) for w in windows), (avg, ent, stats_a)
    assert len(res_a) >= 1

    # everything is silence: no segments, every window skipped after its first attempt
    ctx.set_fallback(logprob_thold=inf, no_speech_thold=-1.0)
    assert ctx.run_full(pcm, **kw) == 0
    stats = ctx.window_stats()
    assert ctx.results() == [] and len(stats) >= 2 and all(w["skipped"] and w["attempts"] == 1 for w in stats)
    assert [w["seek"] for w in stats] == sorted({w["seek"] for w in stats})      # the stream moved on window by window

    # beam search is refused while the feature is on; the streamed run takes it
    with pytest.raises(api.WhisperError) as e:
        ctx.run_full(pcm, beam_width=2, **kw)
    assert e.value.hr & 0xFFFFFFFF == E_NOTIMPL
    ctx.set_fallback(logprob_thold=-inf, entropy_thold=-inf)
    hr, _ = ctx.run_streamed(pcm, **kw)
    streamed, n_stats = _strip(ctx.results()), len(ctx.window_stats())
    ctx.set_fallback(None)
    hr2, _ = ctx.run_streamed(pcm, **kw)
    assert hr == hr2 == 0 and _strip(ctx.results()) == streamed and n_stats >= 2 and ctx.window_stats() == []

    # off again: the plain transcript, beam search runs
    assert ctx.run_full(pcm, **kw) == 0
    assert _strip(ctx.results()) == plain and ctx.window_stats() == []
    assert ctx.run_full(pcm, beam_width=2, **kw) == 0
    with pytest.raises(api.WhisperError):
        ctx.set_fallback(temperature_inc=0.001)
    with pytest.raises(api.WhisperError):
        ctx.set_fallback(logprob_thold=float("nan"))
    ctx.close()
    model.close()
