"""GPU tests of top-k and nucleus sampling ("Top-k and nucleus sampling"): wh_op_nucleus_logits against the float64 restatement
(tests/nucleus_ref.py), the device-side loop with wh_context_set_nucleus on, and the refusals."""
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import nucleus_ref as R  # noqa: E402
import test_gpu_timestamp_rules as T  # noqa: E402  (its helpers: windows, prompts, device buffers)
from whisper_amd import binding  # noqa: E402

pytestmark = pytest.mark.gpu

dev, ptr, same_records = T.dev, T.ptr, T.same_records
G = 1024                                                                         # NaN guard band, floats, before and behind the rows
KINDS = ("ladder", "negative", "denormal", "ties", "plateau", "few_finite", "dominant")
LADDER = [.3, .2, .15, .1, .08, .06, .04, .03, .02]
TEMPS = (1.0, 0.2, 0.0)                                                          # row r samples at TEMPS[ r % 3 ]; 0 = a greedy row


def _row(kind, V, temp, rng):
    """One row whose probabilities at its own temperature are designed: x = temp * ln( mass ) + c at random columns, so that the cumulative mass stands clear of
    0.1 and 0.9 (the restatement asserts it) whatever top_k leaves, over a tail that carries next to nothing."""
    pos, c = rng.permutation(V), 25.0 * temp
    x = (c - temp * (30.0 + 3.0 * np.abs(rng.standard_normal(V)))).astype(np.float32)
    mass = np.array(LADDER) * rng.uniform(0.99, 1.01, len(LADDER))
    if kind == "negative":                                                       # every logit below zero
        c = -30.0
        x = (x - 60.0).astype(np.float32)
    elif kind == "denormal":                                                     # the tail: denormals of both signs with repeats, and both zeros -- top_k = 1024 cuts inside it
        x = (rng.integers(-300, 300, V) * 1e-42).astype(np.float32)
        x[pos[-7:]] = -0.0
    elif kind == "ties":                                                         # ranks 0-2 equal; 100 equal values across rank 50 and across rank 1024
        mass = np.concatenate([[.2, .2, .2, .1, .08, .06, .04, .03], 1e-5 * 0.99 ** np.arange(min(1192, V // 2))])
        mass[20:120] = mass[20]
        mass[1000:1100] = mass[1000:1001]
    elif kind == "plateau":                                                      # 96 equal values that top_p cuts into, behind one head
        mass = np.concatenate([[.27], np.full(96, (1 - .27 - 1e-4) / 96)])
    elif kind == "few_finite":                                                   # 30 entries, fewer than top_k = 50; -inf as the other filters leave it, and NaN
        mass = np.concatenate([mass, 1e-4 * 0.9 ** np.arange(21)])
        x[:] = -np.inf
        x[pos[-2:]] = np.nan
    elif kind == "dominant":                                                     # top_p keeps exactly one
        x = (3.0 * rng.standard_normal(V)).astype(np.float32)
        mass = np.array([1.0])
        c = float(x.max()) + 60.0 * temp
    x[pos[:len(mass)]] = (temp * np.log(mass) + c).astype(np.float32)
    return x


def _rows(kind, rows, V, rng):
    temps = np.array([TEMPS[r % 3] for r in range(rows)], np.float32)
    return np.stack([_row(kind, V, float(t) or 1.0, rng) for t in temps]), np.where(temps > 0, np.float32(1) / np.maximum(temps, np.float32(1e-9)), 0).astype(np.float32)


@pytest.mark.parametrize("rows", [1, 5, 67])
@pytest.mark.parametrize("V", [1000, 51865, 51866])
def test_op_against_the_float64_restatement(V, rows):
    """Every kind of row at top_k 0, 1, 2, 50, 1024 x top_p 0.1, 0.9, 1.0, rows a stride of V + 3 apart (odd rows start misaligned) with NaN between them and NaN
    guard bands around them; rows at T = 1.0, 0.2 and greedy rows in turn. Exactly the restatement's entries are -inf and every other float of the buffer -- the
    kept values, the greedy rows, NaNs, the gaps and the guards -- keeps its bits. The same launch twice gives the same bits."""
    rng = np.random.default_rng(V * 128 + rows)
    stride = V + 3
    for kind in KINDS:
        x, inv_t = _rows(kind, rows, V, rng)
        ranked = [R.order(x[r]) for r in range(rows)]
        flat = np.full(G + rows * stride + G, np.nan, np.float32)
        flat.view(np.uint32)[:] = 0x7FC00123                                     # NaNs with a payload: a rewritten float would lose it
        for r in range(rows):
            flat[G + r * stride:G + r * stride + V] = x[r]
        clean, inv_t_dev = dev(flat), dev(inv_t)
        for k in (0, 1, 2, 50, 1024):
            for p in (0.1, 0.9, 1.0):
                want = flat.copy()
                for r in range(rows):
                    if inv_t[r] > 0:
                        want[G + r * stride:G + r * stride + V][R.discarded(x[r], k, p, inv_t[r], ranked[r])] = -np.inf
                got = []
                for _ in range(2):
                    buf = clean.clone()
                    binding.op_nucleus_logits(C.c_void_p(buf.data_ptr() + 4 * G), rows, stride, V, k, p, ptr(inv_t_dev))
                    torch.cuda.synchronize()
                    got.append(buf.cpu().numpy().view(np.uint32))
                bad = np.flatnonzero(got[0] != want.view(np.uint32))
                assert bad.size == 0, (kind, k, p, bad[:8] - G, bad.size)
                assert np.array_equal(got[0], got[1]), (kind, k, p)


@pytest.fixture(scope="module")
def net():
    c = T._conditioned(10)
    yield c
    c.model.close()


def _context(net, batch):
    ctx = binding.HipContext(net.model, batch)
    ctx.encode(T._mels(batch))
    return ctx, T._prompts4(net.sp, batch)


def _kept_at_every_loop_step(ctx, prompt, ids, k, rows):
    """ids [1 + n_steps][batch] of a window: for the given rows, the id of every loop step is among the k entries the restatement keeps of wh_decode's logits of
    the same prefix -- wh_decode is unfiltered, whatever mode the context is in. (Sample 0 is the prompt step's: a forced timestamp, never narrowed.)"""
    tokens, n_past = prompt, 0
    for s in range(len(ids)):
        logits, _ = ctx.decode(tokens, n_past, want_probs=False)
        for b in rows if s else ():
            assert not R.discarded(logits[b], k, 1.0, 1.0)[ids[s][b]], (s, b, ids[s][b])
        n_past += tokens.shape[1]
        tokens = ids[s].astype(np.int32)[:, None]


@pytest.mark.parametrize("k", [1, 5])
@pytest.mark.parametrize("batch", [1, 5])
def test_a_sampled_window_draws_from_the_restatement_s_k(net, batch, k):
    """T = 1.0: with top_k = 1 one entry is left, so every loop step's draw IS the largest logit of its prefix -- a wrong threshold fails at once -- and with
    top_k = 5 it is one of five; by replayed graph and by eager steps the same records. At top_k = 1 the filter must matter (the window differs from the unfiltered one);
    cleared, the sampled window has the bits it had before the filter was ever set; and a greedy context never launches it: same captures, same bits."""
    ctx, prompt = _context(net, batch)
    n_steps = 12
    greedy = T._window(ctx, prompt, n_steps)
    captures = ctx.step_captures()
    ctx.set_nucleus(top_k=k)
    assert same_records(T._window(ctx, prompt, n_steps), greedy) and ctx.step_captures() == captures
    ctx.set_nucleus()
    ctx.set_sampling(1.0, 77, 3)
    plain = T._window(ctx, prompt, n_steps)
    ctx.set_nucleus(top_k=k)
    on = T._window(ctx, prompt, n_steps)
    assert (k > 1 or not np.array_equal(on["id"], plain["id"])) and np.array_equal(on["id"][0], plain["id"][0])
    ctx.set_flags(binding.WH_FLAG_NO_GRAPH)
    assert same_records(T._window(ctx, prompt, n_steps, chunk=4), on)
    ctx.set_flags(0)
    ctx.set_nucleus(0, 1.0)
    assert same_records(T._window(ctx, prompt, n_steps), plain)
    _kept_at_every_loop_step(ctx, prompt, on["id"], k, range(batch))
    ctx.close()


def test_per_row_mode_filters_the_retried_row_alone(net):
    """wh_context_set_sampling_rows with row 1 at T = 1.0 among greedy neighbours: with top_k = 1 every loop step of row 1 draws the largest logit of its prefix,
    and rows 0 and 2 keep every bit of their records."""
    ctx, prompt = _context(net, 3)
    n_steps = 10
    ctx.set_sampling_rows([0.0, 1.0, 0.0], [0, 99, 0], [0, 5, 0])
    plain = T._window(ctx, prompt, n_steps)
    ctx.set_nucleus(top_k=1)
    on = T._window(ctx, prompt, n_steps)
    assert not np.array_equal(on["id"][:, 1], plain["id"][:, 1])
    for b in (0, 2):
        assert same_records({f: v[:, b] for f, v in on.items()}, {f: v[:, b] for f, v in plain.items()})
    _kept_at_every_loop_step(ctx, prompt, on["id"], 1, [1])
    ctx.close()


@pytest.mark.parametrize("temperature", [0.2, 1.0])
def test_a_tempered_window_equals_the_emulation_at_its_own_temperature(net, temperature):
    """wh_context_set_sampling at T with top_k = 50 and top_p = 0.9: token for token and bit for bit in p what a host-in-the-loop emulation gives -- wh_decode's
    logits, the restatement at 1 / T on every loop step, the op entries' softmax and draw. The nucleus at T = 0.2 is not the one at 1.0: a factor read from the
    wrong place, or a stale top_p, changes the kept set and with it the renormalised p of every sample."""
    ctx, prompt = _context(net, 2)
    sp, V, L, n_steps, seed, nonce = net.sp, net.hp.n_vocab, binding.lib(), 10, 4242, 7
    ctx.set_sampling(temperature, seed, nonce)
    ctx.set_nucleus(50, 0.9)
    got = T._window(ctx, prompt, n_steps)
    inv_t = float(np.float32(1.0) / np.float32(temperature))
    probs = torch.empty((2, V), dtype=torch.float32, device="cuda")
    tokens, n_past, narrowed = prompt, 0, 0
    for s in range(1 + n_steps):
        logits, _ = ctx.decode(tokens, n_past, want_probs=False)
        for b in range(2 if s else 0):
            gone = R.discarded(logits[b], 50, 0.9, inv_t, margin=0.0)
            narrowed += int((~gone & (logits[b] > -np.inf)).sum() < 50)
            logits[b][gone] = -np.inf
        binding.check(L.wh_op_vocab_soft_max_scaled(None, ptr(dev(logits)), inv_t, ptr(probs), 2, V))
        pos = dev(np.full(2, prompt.shape[1] - 1 + s, np.int32))
        tok = T._tokens(L.wh_op_sample_draw, probs, 2, V, sp, int(s == 0), int(s == 0), (seed, nonce, ptr(pos)))
        assert np.array_equal(tok["id"], got["id"][s]) and np.array_equal(tok["p"].view(np.uint32), got["p"][s].view(np.uint32)), (s, tok, got["id"][s])
        n_past += tokens.shape[1]
        tokens = tok["id"].astype(np.int32)[:, None]
    assert narrowed > 0                                                          # top_p cut below top_k somewhere: both halves took part
    ctx.close()


library = T.library                                                              # the conditioned model as a file, six recordings, a context


def test_library_context_and_batch_runner(library):
    """Context.set_sampling_filter under a fallback that forces every window through all six attempts: top_k = 1 reaches the transcripts; cleared, transcripts and
    window_stats are those of a fresh context. BatchRunner.set_sampling_filter( 50, 0.9 ) with some streams retrying among greedy neighbours: every stream equals
    Context.run_full of that stream with the same filter and fallback -- the per-row records' factor against the context's own."""
    lb, key = library, T._key
    forced = dict(temperature_inc=0.2, logprob_thold=1.0, entropy_thold=-1.0, no_speech_thold=2.0, seed=5)
    fresh = lb.model.create_context()
    fresh.set_fallback(**forced)
    assert fresh.run_full(lb.pcms[0], **lb.kw) == 0
    want, want_stats = key(fresh.results()), fresh.window_stats()
    fresh.close()
    try:
        lb.ctx.set_fallback(**forced)
        lb.ctx.set_sampling_filter(top_k=1)
        assert lb.ctx.run_full(lb.pcms[0], **lb.kw) == 0 and key(lb.ctx.results()) != want
        assert all(w["attempts"] == 6 for w in lb.ctx.window_stats())
        lb.ctx.set_sampling_filter()
        assert lb.ctx.run_full(lb.pcms[0], **lb.kw) == 0 and key(lb.ctx.results()) == want and lb.ctx.window_stats() == want_stats
        kw = dict(lb.kw, flags=lb.api.NO_CONTEXT | lb.api.SINGLE_SEGMENT)
        runner = lb.model.create_batch_runner(max_slots=5, groups=1)
        runner.set_fallback(logprob_thold=-1e30, entropy_thold=-1.0, no_speech_thold=2.0)
        assert runner.run(lb.pcms, **kw)[0] == 0
        lowest = sorted(min(x["avg_logprob"] for x in w) for w in runner.window_stats)
        fb = dict(temperature_inc=0.5, logprob_thold=0.5 * (lowest[2] + lowest[3]), entropy_thold=-1.0, no_speech_thold=2.0)
        runner.set_fallback(seed=9, **fb)
        hr, plain, _ = runner.run(lb.pcms, **kw)
        runner.set_sampling_filter(50, 0.9)
        hr2, got, per = runner.run(lb.pcms, **kw)
        stats = runner.window_stats
        assert hr == 0 and hr2 == 0 and all(p == 0 for p in per) and [key(g) for g in got] != [key(g) for g in plain]
        assert any(x["attempts"] > 1 for w in stats for x in w) and any(all(x["attempts"] == 1 for x in w) for w in stats)
        lb.ctx.set_sampling_filter(50, 0.9)
        for i, (pcm, g) in enumerate(zip(lb.pcms, got)):
            lb.ctx.set_fallback(seed=9 + i, **fb)
            assert lb.ctx.run_full(pcm, **kw) == 0 and key(g) == key(lb.ctx.results()), i
        for obj in (lb.ctx, runner):
            for bad in ((1025, 1.0), (-1, 1.0), (0, 0.0), (0, 1.5), (0, float("nan"))):
                with pytest.raises(lb.api.WhisperError) as e:
                    obj.set_sampling_filter(*bad)
                assert e.value.hr == 0x80070057
        runner.close()
    finally:
        lb.ctx.set_fallback(None)
        lb.ctx.set_sampling_filter()


def test_whisper_main_takes_the_options(library, tmp_path):
    """whisper-main --top-k / --top-p: legal without --fallback and then without effect (the plain transcript); with --fallback forcing every attempt, top_k = 1
    changes it; a top_k beyond 1024 ends the tool with an error."""
    import subprocess
    import wave
    from whisper_amd import build
    wav = str(tmp_path / "rec.wav")
    with wave.open(wav, "wb") as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(16000)
        w.writeframes(np.clip(np.round(library.pcms[0] * 32768.0), -32768, 32767).astype("<i2").tobytes())

    def tool(*extra):
        return subprocess.run([build.CLI_BIN, "-m", library.path, "-f", wav, "-l", "en", "-nc"] + list(extra), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)

    plain, forced = tool(), tool("--fallback", "-lpt", "1", "-nth", "2")
    assert plain.returncode == 0 and forced.returncode == 0 and plain.stdout
    assert tool("--top-k", "1", "--top-p", "0.5").stdout == plain.stdout
    narrowed = tool("--fallback", "-lpt", "1", "-nth", "2", "--top-k", "1")
    assert narrowed.returncode == 0 and narrowed.stdout and narrowed.stdout != forced.stdout
    assert tool("--top-k", "2000").returncode != 0


@pytest.mark.parametrize("what,message", [
    ((-1, 1.0), "top_k outside"), ((1025, 1.0), "top_k outside"), ((0, 0.0), "top_p outside"), ((0, 1.5), "top_p outside"), ((0, float("nan")), "top_p outside"),
    ("hyp", "hypothesis-group"), ("flag_then_setting", "WH_FLAG_PARITY_EXACT"), ("setting_then_flag", "wh_context_set_nucleus is on")])
def test_refusals(net, what, message):
    ctx = binding.HipContext(net.model, 1, hypotheses=2 if what == "hyp" else 1)
    try:
        with pytest.raises(binding.WhisperHipError, match=message):
            if what == "flag_then_setting":
                ctx.set_flags(binding.WH_FLAG_PARITY_EXACT, 2)
            if what == "setting_then_flag":
                ctx.set_nucleus(50, 0.9)
                ctx.set_flags(binding.WH_FLAG_PARITY_EXACT, 2)
            ctx.set_nucleus(*(what if isinstance(what, tuple) else (50, 0.9)))
    finally:
        ctx.close()
