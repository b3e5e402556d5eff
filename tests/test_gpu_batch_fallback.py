"""GPU tests of the decoding fallback in the lock-step batch runner ("The batch runner"):

  * wh_op_sample_rows: a greedy row is wh_op_vocab_soft_max + wh_op_sample_best, a sampled row wh_op_vocab_soft_max_scaled( 1 / T ) + wh_op_sample_draw run on
    that row alone with the row's seed, nonce and position -- every field and every probability, bit for bit, both softmax kernels, both flag settings;
  * wh_context_set_sampling_rows: in a ragged batch of 6 the greedy rows keep the records of an all-greedy run, the sampled rows equal a host-stepped replay;
    rounds that enter and leave the mode (both captured graphs alive side by side) leave the greedy records as they were; the refusals;
  * the library: BatchRunner.set_fallback / window_stats, whisperc_batch_set_fallback / whisperc_tr_window_stats, whisper-mgpu -fallback.
"""
import ctypes as C
import json
import os
import re
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from whisper_amd import binding, ggml_format as gf  # noqa: E402

pytestmark = pytest.mark.gpu

TOKEN_DT = np.dtype([("id", "<i4"), ("tid", "<i4"), ("p", "<f4"), ("pt", "<f4"), ("ptsum", "<f4")])
FIELDS = ("id", "tid", "p", "pt", "ptsum")
E_NOTIMPL = 0x80004001


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def ptr(t):
    return C.c_void_p(t.data_ptr())


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same_records(a, b):
    """Every TokenData field, floats by their bits"""
    return all(np.array_equal(np.ascontiguousarray(a[k]).view(np.uint32), np.ascontiguousarray(b[k]).view(np.uint32)) for k in FIELDS)


def _tokens(fn, probs_dev, rows, V, sp, force, initial, extra=()):
    out = torch.zeros(rows * 5, dtype=torch.int32, device="cuda")
    binding.check(fn(None, ptr(probs_dev), rows, V, sp["beg"], sp["sot"], sp["solm"], sp["not_"], int(force), int(initial), *extra, ptr(out)))
    torch.cuda.synchronize()
    return np.frombuffer(out.cpu().numpy().tobytes(), TOKEN_DT)


def _sample_rows(logits_dev, rows, V, sp, force, initial, temps, seeds, nonces, pos_dev):
    """wh_op_sample_rows on rows [0, rows) of logits_dev: (records, probabilities [rows][V])"""
    L = binding.lib()
    params = (binding.SampleRowC * rows)(*[binding.SampleRowC(float(t), int(n), int(s)) for t, s, n in zip(temps, seeds, nonces)])
    probs = torch.full((rows, V), float("nan"), dtype=torch.float32, device="cuda")
    out = torch.zeros(rows * 5, dtype=torch.int32, device="cuda")
    binding.check(L.wh_op_sample_rows(None, ptr(logits_dev), rows, V, sp["beg"], sp["sot"], sp["solm"], sp["not_"], int(force), int(initial),
                                      C.cast(params, C.c_void_p), ptr(pos_dev), ptr(probs), ptr(out)))
    torch.cuda.synchronize()
    return np.frombuffer(out.cpu().numpy().tobytes(), TOKEN_DT), probs.cpu().numpy()


def _specials(V):
    if V >= 51864:
        return gf.special_tokens(SimpleNamespace(n_vocab=V))
    return dict(beg=V - 300, sot=V - 420, solm=V - 303, not_=V - 302)           # a small vocabulary: 300 timestamps, the specials below them


# ---------------------------------------------------------------------------------------------------------------------
# op level
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V", [1000, 51865, 51866, 52225])
def test_sample_rows_op_bit_for_bit(V):
    """Rows = 5 with temperatures [0, 0.4, 0, 1.0, 0.2] and rows = 1 (greedy, then sampled); forceTimestamp / isInitial 0 and 1; the logits between NaN guard
    rows. 52225 columns take the three-pass softmax. Both sides run the same arithmetic in the same order: exact, nothing left out."""
    L = binding.lib()
    sp = _specials(V)
    rng = np.random.default_rng(V)
    cases = [([0.0, 0.4, 0.0, 1.0, 0.2], [11, 2 ** 63 + 5, 0, 0xDEADBEEFCAFE, 7], [3, 24 * 8 + 1, 0, 0xFFFFFFFF, 9], [4, 17, 0, 223, 5]),
             ([0.0], [1], [2], [3]), ([0.7], [0x0123456789ABCDEF], [40 * 8 + 2], [31])]
    n_sampled = n_moved = 0
    for temps, seeds, nonces, positions in cases:
        rows = len(temps)
        x = np.full((rows + 2, V), np.nan, np.float32)                          # guard rows before and behind
        x[1:-1] = (2.5 * rng.standard_normal((rows, V))).astype(np.float32)
        x[1:-1, sp["beg"]:] += 1.0                                                # timestamps carry mass: pt / ptsum are not trivial
        x[1, rng.integers(0, V, V // 11)] = -np.inf
        x[rows, sp["sot"]] = 30.0                                                 # the last row's best token is a special: sampleBest's rounds skip it
        xd = dev(x)
        logits = xd[1:-1]
        pos_dev = dev(np.asarray(positions, np.int32))
        for flag in (0, 1):
            got, got_p = _sample_rows(logits, rows, V, sp, flag, flag, temps, seeds, nonces, pos_dev)
            for r, (T, seed, nonce, pos) in enumerate(zip(temps, seeds, nonces, positions)):
                want_p = torch.full((1, V), float("nan"), dtype=torch.float32, device="cuda")
                if T == 0:
                    binding.check(L.wh_op_vocab_soft_max(None, ptr(logits[r]), ptr(want_p), 1, V))
                    want = _tokens(L.wh_op_sample_best, want_p, 1, V, sp, flag, flag)
                else:
                    inv_t = float(np.float32(1.0) / np.float32(T))
                    binding.check(L.wh_op_vocab_soft_max_scaled(None, ptr(logits[r]), inv_t, ptr(want_p), 1, V))
                    one_pos = dev(np.asarray([pos], np.int32))
                    want = _tokens(L.wh_op_sample_draw, want_p, 1, V, sp, flag, flag, (seed, nonce, ptr(one_pos)))
                    best = _tokens(L.wh_op_sample_best, want_p, 1, V, sp, flag, flag)
                    n_sampled += 1
                    n_moved += int(want["id"][0] != best["id"][0])
                where = (V, rows, r, T, flag)
                assert np.array_equal(bits(got_p[r]), bits(want_p.cpu().numpy()[0])), where
                assert same_records(got[r:r + 1], want), where + (got[r], want[0])
        assert np.array_equal(x.view(np.uint32), xd.cpu().numpy().view(np.uint32)), "the logits were written"
    print("V %d: %d sampled rows, %d drew another token than the best one" % (V, n_sampled, n_moved))
    assert n_moved > 0                                                           # the draws are draws
    # bad arguments
    pos = dev(np.zeros(1, np.int32))
    p = dev(np.zeros(16, np.float32))
    out = dev(np.zeros(5, np.int32))
    one = (binding.SampleRowC * 1)(binding.SampleRowC(0.5, 0, 0))
    hot = (binding.SampleRowC * 1)(binding.SampleRowC(4.5, 0, 0))
    args = (8, 1, 2, 3, 0, 0)
    assert L.wh_op_sample_rows(None, ptr(p), 1, 16, *args, None, ptr(pos), ptr(p), ptr(out)) != 0
    assert L.wh_op_sample_rows(None, ptr(p), 1, 16, *args, C.cast(hot, C.c_void_p), ptr(pos), ptr(p), ptr(out)) != 0
    assert L.wh_op_sample_rows(None, ptr(p), 1, 16, *args, C.cast(one, C.c_void_p), None, ptr(p), ptr(out)) != 0
    assert L.wh_op_sample_rows(None, ptr(p), 1, 65537, *args, C.cast(one, C.c_void_p), ptr(pos), ptr(p), ptr(out)) != 0


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


def _ragged_window(ctx, prompts, n_steps, chunk=0):
    """prompt step + n_steps steps, in one enqueue or in chunks: dict of [1 + n_steps][batch] arrays"""
    if chunk:
        ctx.decode_window_start_ragged(prompts, 0)
        for _ in range(n_steps // chunk):
            ctx.decode_window_continue(chunk)
    else:
        ctx.decode_window_start_ragged(prompts, n_steps)
    data = ctx.decode_window_fetch_data(0, 1 + n_steps)
    ctx.decode_window_finish()
    return data


def test_context_rows_in_a_ragged_batch(conditioned):
    """6 rows (above SMALL_MAX_ROWS), ragged prompts, a prompt step plus 12 steps, in one enqueue and in chunks of 4. Rows 1 and 4 sample (0.8 and 0.5, keys and
    nonces of their own); they carry the longest prompts, so a replay through wh_decode -- same tokens, same padding, uniform positions -- feeds them the
    device's own logits: wh_op_sample_rows on those must give their records. The other rows keep the records of the all-greedy run. Then all 0 -> mixed ->
    all 0 once more: the greedy rounds replay the greedy graph that lived through the per-row rounds."""
    c, sp, V = conditioned, conditioned.sp, conditioned.hp.n_vocab
    batch, n_steps = 6, 12
    n_max = 6
    lens = [3, n_max, 4, 5, n_max, 3]
    prompts = []
    for b, ln in enumerate(lens):
        head = [sp["prev"]] + [1000 + 7 * b + i for i in range(ln - 4)] if ln > 3 else []
        prompts.append((head + [sp["sot"], sp["sot"] + 1 + b, sp["transcribe"]])[-ln:])
    assert [len(p) for p in prompts] == lens
    temps = np.array([0, 0.8, 0, 0, 0.5, 0], np.float32)
    seeds = np.array([1, 0xDEADBEEFCAFE, 2, 3, 2 ** 63 + 11, 4], np.uint64)
    nonces = np.array([0, 24 * 8 + 3, 0, 0, 7, 0], np.uint32)
    sampled = [1, 4]
    others = [0, 2, 3, 5]

    ctx = binding.HipContext(c.model, batch)
    ctx.encode(_mels(batch))
    greedy = _ragged_window(ctx, prompts, n_steps)

    ctx.set_sampling_rows(np.zeros(batch, np.float32), seeds, nonces)            # every row greedy: the mode stays off
    assert same_records(_ragged_window(ctx, prompts, n_steps), greedy)

    ctx.set_sampling_rows(temps, seeds, nonces)
    runs = [_ragged_window(ctx, prompts, n_steps), _ragged_window(ctx, prompts, n_steps, chunk=4)]
    ctx.set_flags(binding.WH_FLAG_NO_GRAPH)
    runs.append(_ragged_window(ctx, prompts, n_steps))
    ctx.set_flags(0)
    for r in runs[1:]:
        assert same_records(r, runs[0])
    mixed = runs[0]
    for k in FIELDS:
        assert np.array_equal(mixed[k][:, others].view(np.uint32), greedy[k][:, others].view(np.uint32)), k
    print("sampled rows: %d of %d tokens differ from the greedy ones" % (int((mixed["id"][:, sampled] != greedy["id"][:, sampled]).sum()), 2 * (1 + n_steps)))

    # all 0 -> mixed -> all 0: both captured graphs stay alive, nothing changes
    ctx.set_sampling_rows(None)
    assert same_records(_ragged_window(ctx, prompts, n_steps, chunk=4), greedy)
    ctx.set_sampling_rows(temps, seeds, nonces)
    assert same_records(_ragged_window(ctx, prompts, n_steps, chunk=4), mixed)
    ctx.set_sampling_rows(np.zeros(batch, np.float32), seeds, nonces)
    assert same_records(_ragged_window(ctx, prompts, n_steps), greedy)

    # host-stepped replay of the sampled rows (full-length prompts: right-padded neighbours do not reach them, and their position is the uniform one)
    padded = np.zeros((batch, n_max), np.int32)
    for b, p in enumerate(prompts):
        padded[b, :len(p)] = p
    tokens, n_past = padded, 0
    for s in range(1 + n_steps):
        logits, _ = ctx.decode(tokens, n_past, want_probs=False)
        pos = dev(np.full(batch, n_max - 1 + s, np.int32))
        first = int(s == 0)
        tok, _ = _sample_rows(dev(logits), batch, V, sp, first, first, temps, seeds, nonces, pos)
        for r in sampled:
            got = {k: mixed[k][s, r:r + 1] for k in FIELDS}
            assert same_records(got, tok[r:r + 1]), (s, r, {k: got[k] for k in FIELDS}, tok[r])
        n_past += tokens.shape[1]
        tokens = mixed["id"][s].astype(np.int32)[:, None].copy()
    ctx.close()


def test_sampling_rows_refusals(conditioned):
    c, sp = conditioned, conditioned.sp
    t, s, n = np.array([0.5, 0], np.float32), np.zeros(2, np.uint64), np.zeros(2, np.uint32)
    ctx = binding.HipContext(c.model, 2)
    for bad in (-0.5, float("nan"), 4.5, float("inf")):
        with pytest.raises(binding.WhisperHipError):
            ctx.set_sampling_rows(np.array([0, bad], np.float32), s, n)
    with pytest.raises(binding.WhisperHipError):
        ctx.set_sampling_rows(np.zeros(3, np.float32), np.zeros(3, np.uint64), np.zeros(3, np.uint32))      # more rows than sequences
    ctx.set_sampling_rows(np.array([4.0, 0], np.float32), s, n)
    with pytest.raises(binding.WhisperHipError):
        ctx.set_sampling(0.5)                                                    # the two modes exclude each other
    ctx.set_sampling_rows(None)                                                  # rows == 0 turns the mode off
    ctx.set_sampling(0.5)
    with pytest.raises(binding.WhisperHipError):
        ctx.set_sampling_rows(t, s, n)
    ctx.set_sampling(0.0)
    ctx.set_flags(binding.WH_FLAG_PARITY_EXACT)
    with pytest.raises(binding.WhisperHipError):
        ctx.set_sampling_rows(t, s, n)
    ctx.set_flags(0)
    # off: the greedy sampler of two rows again
    prompt = np.array([[sp["sot"], sp["sot"] + 1 + b, sp["transcribe"]] for b in range(2)], np.int32)
    ctx.encode(_mels(2))
    ctx.decode_window_start(prompt, 3)
    before = ctx.decode_window_fetch_data(0, 4)
    ctx.decode_window_finish()
    ctx.set_sampling_rows(t, s, n)
    ctx.set_sampling_rows(None)
    ctx.decode_window_start(prompt, 3)
    after = ctx.decode_window_fetch_data(0, 4)
    ctx.decode_window_finish()
    assert same_records(before, after)
    ctx.close()
    hyp = binding.HipContext(c.model, 1, hypotheses=2)
    with pytest.raises(binding.WhisperHipError):
        hyp.set_sampling_rows(t, s, n)
    hyp.close()


def test_no_speech_in_a_per_row_round(conditioned):
    """Behind wh_decode_window_start_ragged in a per-row round the gather reads probabilities: a greedy row's value is the prompt step's own P( <|nospeech|> )."""
    c, sp = conditioned, conditioned.sp
    batch = 5
    prompt = np.array([[sp["sot"], sp["sot"] + 1 + b, sp["transcribe"]] for b in range(batch)], np.int32)
    ctx = binding.HipContext(c.model, batch)
    ctx.encode(_mels(batch))
    ctx.set_no_speech(True)
    ctx.set_sampling_rows(np.array([0, 0.5, 0, 0, 0], np.float32), np.ones(batch, np.uint64), np.ones(batch, np.uint32))
    ctx.decode_window_start_ragged([list(p) for p in prompt], 2)
    got = ctx.window_no_speech(batch)
    ctx.decode_window_finish()
    ctx.set_sampling_rows(None)
    _, probs = ctx.decode(prompt, 0)
    keep = [0, 2, 3, 4]
    assert np.array_equal(bits(got[keep]), bits(probs[keep, sp["solm"]])) and (got > 0).all()
    ctx.close()


# ---------------------------------------------------------------------------------------------------------------------
# library
# ---------------------------------------------------------------------------------------------------------------------
def _pcm(seconds, tone, seed):
    t = np.arange(int(seconds * 16000)) / 16000.0
    rng = np.random.default_rng(seed)
    return (0.25 * np.sin(2 * np.pi * tone * t) * (1 + 0.6 * np.sin(2 * np.pi * 2.5 * t)) + 0.05 * rng.standard_normal(len(t))).astype(np.float32)


def _strip(segs):
    return [(s["t0"], s["t1"], s["text"], [(t["id"], t["p"], t["pt"], t["ptsum"]) for t in s["tokens"]]) for s in segs]


RECORDINGS = ((40, 330, 7), (65, 440, 8), (45, 250, 9), (70, 520, 10), (50, 390, 11), (62, 300, 12))      # seconds, tone, seed: 2 or 3 windows each


@pytest.fixture(scope="module")
def library(conditioned, tmp_path_factory):
    from whisper_amd import api
    path = str(tmp_path_factory.mktemp("bfb") / "cond.bin")
    gf.write_model(path, conditioned.ggml)
    model = api.Model(path)
    pcms = [_pcm(*r) for r in RECORDINGS]
    kw = dict(language="en", prompt=[1000], n_max_text_ctx=0, flags=api.NO_CONTEXT | api.SINGLE_SEGMENT)
    runner = model.create_batch_runner(max_slots=5, groups=1)
    hr, off, per = runner.run(pcms, **kw)
    assert hr == 0 and all(p == 0 for p in per) and runner.window_stats == [[]] * len(pcms)
    yield SimpleNamespace(api=api, path=path, model=model, pcms=pcms, kw=kw, runner=runner, off=[_strip(s) for s in off])
    runner.close()
    model.close()


def test_library_gates_that_cannot_fire(library):
    """(a) ids, times and probabilities of the runner with the feature off, one attempt per window; (e) the greedy attempt's scores of every first window
    against Context.run_full with the same settings: same seeks, same attempts, avgLogprob and noSpeech within the 2e-2 that batch-versus-single
    probabilities are granted (tests/test_batch_api.py)."""
    lb = library
    lb.runner.set_fallback(logprob_thold=-1e30, entropy_thold=-1.0, no_speech_thold=2.0)
    hr, got, per = lb.runner.run(lb.pcms, **lb.kw)
    stats = lb.runner.window_stats
    lb.runner.set_fallback(None)
    assert hr == 0 and [_strip(s) for s in got] == lb.off
    assert all(2 <= len(w) <= 4 for w in stats)
    assert all(x["attempts"] == 1 and x["temperature"] == 0 and not x["skipped"] and 0 <= x["no_speech"] < 1 for w in stats for x in w)
    ctx = lb.model.create_context()
    ctx.set_fallback(logprob_thold=-1e30, entropy_thold=-1.0, no_speech_thold=2.0)
    worst = 0.0
    for pcm, w in zip(lb.pcms, stats):
        assert ctx.run_full(pcm, **lb.kw) == 0
        single = ctx.window_stats()
        assert [(x["seek"], x["attempts"]) for x in single] == [(x["seek"], x["attempts"]) for x in w]
        worst = max(worst, abs(single[0]["avg_logprob"] - w[0]["avg_logprob"]), abs(single[0]["no_speech"] - w[0]["no_speech"]))
    ctx.close()
    print("first windows, batch against one stream: largest difference of avgLogprob / noSpeech %.3e" % worst)
    assert worst < 2e-2


def test_library_every_window_retries(library):
    """(b) logprob_thold = +1, inc 0.5: three attempts per window, the last at temperature 1.0; two runs agree exactly."""
    lb = library
    lb.runner.set_fallback(temperature_inc=0.5, logprob_thold=1.0, entropy_thold=-1.0, no_speech_thold=2.0, seed=5)
    runs = []
    for _ in range(2):
        hr, got, per = lb.runner.run(lb.pcms, **lb.kw)
        assert hr == 0
        runs.append(([_strip(s) for s in got], lb.runner.window_stats))
    lb.runner.set_fallback(None)
    assert runs[0] == runs[1]
    assert all(x["attempts"] == 3 and x["temperature"] == 1.0 and not x["skipped"] for w in runs[0][1] for x in w)
    assert all(2 <= len(w) <= 4 for w in runs[0][1])
    assert runs[0][0] != lb.off                                                  # the temperature reached the streams
    hr, got, _ = lb.runner.run(lb.pcms, **lb.kw)                                 # off again: the transcripts from before
    assert hr == 0 and [_strip(s) for s in got] == lb.off and lb.runner.window_stats == [[]] * len(lb.pcms)


def test_library_neighbours_do_not_see_a_retry(library):
    """(c) logprob_thold midway between two neighbouring greedy avgLogprob values: the streams whose windows all lie above it keep their feature-off
    transcripts bit for bit while their neighbours retry in the same decode steps (the per-row graph); the streams with a window below it retry."""
    lb = library
    lb.runner.set_fallback(logprob_thold=-1e30, entropy_thold=-1.0, no_speech_thold=2.0)
    hr, _, _ = lb.runner.run(lb.pcms, **lb.kw)
    never = lb.runner.window_stats
    lowest = sorted((min(x["avg_logprob"] for x in w), i) for i, w in enumerate(never))      # per stream: its worst window
    assert hr == 0 and len({v for v, _ in lowest}) == len(lowest)
    mid = len(lowest) // 2
    thold = 0.5 * (lowest[mid - 1][0] + lowest[mid][0])
    below, above = [i for v, i in lowest if v < thold], [i for v, i in lowest if v > thold]
    lb.runner.set_fallback(temperature_inc=0.5, logprob_thold=thold, entropy_thold=-1.0, no_speech_thold=2.0, seed=9)
    hr, got, _ = lb.runner.run(lb.pcms, **lb.kw)
    stats = lb.runner.window_stats
    lb.runner.set_fallback(None)
    assert hr == 0 and len(below) == 3 and len(above) == 3
    for i in above:
        assert _strip(got[i]) == lb.off[i], i
        assert all(x["attempts"] == 1 for x in stats[i])
    for i in below:
        assert any(x["attempts"] > 1 for x in stats[i]), (i, stats[i])


def test_library_everything_is_silence(library):
    """(d) no_speech_thold = -1, logprob_thold = +1: every window is skipped after its greedy attempt, no segments, every stream S_FALSE."""
    lb = library
    lb.runner.set_fallback(logprob_thold=1.0, no_speech_thold=-1.0)
    hr, got, per = lb.runner.run(lb.pcms, **lb.kw)
    stats = lb.runner.window_stats
    lb.runner.set_fallback(None)
    assert hr == 0 and all(s == [] for s in got) and per == [1] * len(lb.pcms)
    assert all(x["skipped"] and x["attempts"] == 1 for w in stats for x in w) and all(len(w) >= 2 for w in stats)
    with pytest.raises(lb.api.WhisperError):
        lb.runner.set_fallback(temperature_inc=0.001)
    with pytest.raises(lb.api.WhisperError):
        lb.runner.set_fallback(logprob_thold=float("nan"))


def test_flat_c_and_mgpu_fallback(library, tmp_path):
    """One rank, two chunks of a 45 s recording: whisperc_batch_set_fallback + whisperc_tr_window_stats, then whisper-mgpu -fallback."""
    import wave
    from whisper_amd import build
    lb, api = library, library.api
    L = api.lib()
    pcm = lb.pcms[2]
    chunks = [(0, 480000), (480000, len(pcm) - 480000)]
    n = len(chunks)
    runner = C.c_void_p()
    assert L.whisperc_batch_create(lb.model.h, 5, 1, 0, 0, C.byref(runner)) == 0
    assert L.whisperc_batch_set_fallback(runner, 1, 0.5, 1.0, -1.0, 2.0, 3) == 0
    ptrs, lens, first, cnt = (C.c_void_p * n)(), (C.c_uint32 * n)(), (C.c_int64 * n)(), (C.c_int64 * n)()
    for i, (f, c) in enumerate(chunks):
        ptrs[i], lens[i], first[i], cnt[i] = pcm.ctypes.data, len(pcm), f, c
    res, per = (C.c_void_p * n)(), (C.c_int32 * n)()
    pt = np.asarray([1000], np.int32)
    hr = L.whisperc_batch_run(runner, n, ptrs, lens, first, cnt, b"en", api.NO_CONTEXT | api.SINGLE_SEGMENT, 0, pt.ctypes.data_as(C.c_void_p), 1, 0, res, per)
    assert hr == 0
    for i in range(n):
        cnt_w = C.c_uint32()
        assert res[i] and L.whisperc_tr_window_stats(res[i], None, 0, C.byref(cnt_w)) == 0 and cnt_w.value == 1
        arr = (api.WindowStatsC * 1)()
        assert L.whisperc_tr_window_stats(res[i], arr, 1, C.byref(cnt_w)) == 0
        assert arr[0].attempts == 3 and arr[0].temperature == 1.0 and arr[0].seek == 0 and not arr[0].skipped
        assert L.whisperc_tr_window_stats(res[i], arr, 0, C.byref(cnt_w)) != 0   # too small a buffer
        L.whisperc_release(res[i])
    assert L.whisperc_batch_set_fallback(runner, 0, 0.0, 0.0, 0.0, 0.0, 0) == 0
    L.whisperc_release(runner)

    wav = str(tmp_path / "rec.wav")
    with wave.open(wav, "wb") as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(16000)
        w.writeframes(np.clip(np.round(pcm * 32768.0), -32768, 32767).astype("<i2").tobytes())
    out = str(tmp_path / "t.txt")
    r = subprocess.run([build.MGPU_BIN, "-n", "1", "-m", lb.path, "-f", wav, "-o", out, "-timeout", "60", "-slots", "5", "-fallback", "-tpi", "0.5", "-lpt", "1",
                        "-et", "-1", "-nth", "2"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    print(r.stdout.decode(), r.stderr.decode()[-2000:])
    assert r.returncode == 0
    # (the tool keeps the sliding window inside a chunk: a chunk may take more than one window)
    m = re.search(rb"fallback: (\d+) windows, (\d+) attempts, (\d+) retried, (\d+) skipped", r.stderr)
    windows, attempts, retried, skipped = (int(x) for x in m.groups())
    assert windows >= 2 and attempts == 3 * windows and retried == windows and skipped == 0
    assert json.loads(r.stdout.decode().strip().splitlines()[-1])["windows"] == 2
