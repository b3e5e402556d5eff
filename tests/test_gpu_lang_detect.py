"""GPU tests of language detection (language "auto"): the kernel at op level, wh_lang_detect against the reference's
whisper_lang_auto_detect (oracle/_ref, bit for bit in the exact mode, within the reference's own thread-count movement on the timed
path), and the host library's runFull / runStreamed / beam search / whisper-main with the language left to the device.

The cases are those of tests/golden/ref_lang_detect.json (tests/golden/make_golden_lang_detect.py): every one of them is checked,
none is left out -- the generator kept only cases whose winner and transcript do not depend on the reference's thread count."""
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from oracle import ref, whisper_np as wn  # noqa: E402
from whisper_amd import binding, ggml_format as gf  # noqa: E402

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")
sys.path.insert(0, GOLDEN)
import make_golden_lang_detect as mk  # noqa: E402


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def ptr(t):
    return C.c_void_p(t.data_ptr())


class options:
    def __init__(self, **kw):
        self.kw = kw

    def __enter__(self):
        for k, v in self.kw.items():
            binding.set_option(k, v)

    def __exit__(self, *a):
        for k in self.kw:
            binding.set_option(k, binding.OPTION_DEFAULTS[k])


def fixture():
    with open(os.path.join(GOLDEN, "ref_lang_detect.json")) as f:
        return json.load(f)


# ---------------------------------------------------------------------------------------------------------------------
# 4. the kernel
# ---------------------------------------------------------------------------------------------------------------------
def _logit_rows(rows, cols, sot, n_lang, seed):
    """Seeded logits with -inf columns (inside and outside the language block), an exact tie for the first place inside the language block
    in every third row, the row maximum inside the block in every fifth."""
    rng = np.random.default_rng(seed)
    x = (3.0 * rng.standard_normal((rows, cols))).astype(np.float32)
    lo = sot + 1
    for r in range(rows):
        x[r, rng.integers(0, cols, cols // 9)] = -np.inf
        x[r, lo + rng.integers(0, n_lang, 5)] = -np.inf
        if r % 3 == 0:
            a, b = sorted(rng.choice(n_lang, 2, replace=False))
            x[r, lo:lo + n_lang] = np.minimum(x[r, lo:lo + n_lang], 6.0)
            x[r, lo + a] = x[r, lo + b] = 7.5
        if r % 5 == 1:
            x[r, lo + rng.integers(0, n_lang)] = 30.0
        if r % 7 == 2:
            x[r, cols - 1] = 25.0                                                   # the maximum in the partial last chunk of the row
    return x


@pytest.mark.parametrize("cols", [51865, 51866])
@pytest.mark.parametrize("rows", [1, 5, 40, 448])
def test_op_lang_probs_equals_the_vocabulary_softmax(rows, cols):
    """langProbsKernel writes, for the language columns, the bits launchVocabSoftMax writes there (both of its kernels), and the first argmax of those
    columns. At 448 x 51865 also against the float64 table softmax under test_gpu_beam_ops.test_vocab_soft_max_both_kernels' bound."""
    L = binding.lib()
    sot, n_lang = 50258, cols - 51766               # the multilingual vocabularies: 99 languages at 51865, 100 at the large-v3 shape
    x = _logit_rows(rows, cols, sot, n_lang, rows * 7919 + cols)
    xd = dev(x)
    got = {}
    for regs in (1, 0):
        with options(beam_regs=regs):
            probs = torch.full((rows, cols), float("nan"), dtype=torch.float32, device="cuda")
            binding.check(L.wh_op_vocab_soft_max(None, ptr(xd), ptr(probs), rows, cols))
            lang_p = torch.full((rows, n_lang), float("nan"), dtype=torch.float32, device="cuda")
            best = torch.full((rows,), -7, dtype=torch.int32, device="cuda")
            binding.check(L.wh_op_lang_probs(None, ptr(xd), rows, cols, sot, n_lang, ptr(lang_p), ptr(best)))
            torch.cuda.synchronize()
        want = probs.cpu().numpy()[:, sot + 1:sot + 1 + n_lang]
        got[regs] = lang_p.cpu().numpy()
        assert np.array_equal(got[regs].view(np.uint32), np.ascontiguousarray(want).view(np.uint32)), (rows, cols, regs, "langP differs from the softmax's columns")
        assert np.array_equal(best.cpu().numpy(), np.argmax(want, axis=1).astype(np.int32)), (rows, cols, regs, "best is not the first argmax")
    assert np.array_equal(got[0].view(np.uint32), got[1].view(np.uint32))
    assert np.array_equal(xd.cpu().numpy().view(np.uint32), x.view(np.uint32)), "the input was written"
    if rows == 448 and cols == 51865:
        full = wn.softmax_table(x)
        d = np.abs(got[1].astype(np.float64) - full[:, sot + 1:sot + 1 + n_lang].astype(np.float64))
        print("lang_probs 448 x 51865 against float64: maxdiff %.3e, %d of %d differ" % (d.max(), int((d > 0).sum()), d.size))
        assert d.max() < 1e-3 * full.max() and (d > 0).mean() < 0.01


def test_op_lang_probs_rejects_bad_sizes():
    L = binding.lib()
    x = torch.zeros((1, 1000), dtype=torch.float32, device="cuda")
    p = torch.zeros((1, 1100), dtype=torch.float32, device="cuda")
    b = torch.zeros((1,), dtype=torch.int32, device="cuda")
    for sot, n_lang in ((990, 10), (-1, 5), (0, 0), (0, 1025)):
        assert L.wh_op_lang_probs(None, ptr(x), 1, 1000, sot, n_lang, ptr(p), ptr(b)) == -1, (sot, n_lang)
    assert L.wh_op_lang_probs(None, None, 1, 1000, 0, 5, ptr(p), ptr(b)) == -1
    assert L.wh_op_lang_probs(None, ptr(x), 1, 52225, 50258, 99, ptr(p), ptr(b)) == -1          # the row no longer fits the registers


# ---------------------------------------------------------------------------------------------------------------------
# 5. / 6. wh_lang_detect against the reference's whisper_lang_auto_detect
# ---------------------------------------------------------------------------------------------------------------------
def _by_seed(cases):
    out = {}
    for c in cases:
        out.setdefault(c["seed"], []).append(c)
    return out


def _windows_with_idle_slots(mels):
    """case, idle, case, idle, ... : every recording in a slot of its own, windows of zeros in between"""
    wins = []
    for m in mels:
        wins += [(m, 0), (None, 0)]
    return wins[:-1]


def test_lang_detect_exact_mode_is_the_reference_bit_for_bit(ref_lib_available, tmp_path):
    """WH_FLAG_PARITY_EXACT, every fixture case: p on the language tokens bit-equal to the reference's probabilities there (the reference fed the
    device's spectrogram, at the same thread count), the same winner, and the host half on the device's p bit-equal to the reference's lang_probs --
    at batch 1 and with all recordings of a model in one batch (one recording per slot through wh_encode_windows, idle slots in between), on a
    greedy context and on a hypothesis-group context."""
    if not ref_lib_available:
        pytest.skip("oracle/_ref/libwhisper_ref.so not present")
    from whisper_amd import api
    n_threads = 4
    for seed, cases in _by_seed(fixture()["cases"]).items():
        model = mk.model_for(seed)
        path = str(tmp_path / ("m%d.bin" % seed))
        gf.write_model(path, model)
        m = binding.HipModel.from_ggml(model)
        assert m.lang_count() == 99
        ctx = binding.HipContext(m, 2 * len(cases))
        ctx.set_flags(binding.WH_FLAG_PARITY_EXACT, n_threads)
        mels = [ctx.mel_spectrogram(dev(mk.pcm_for(c["pcm"]))) for c in cases]
        want = []
        for c, mel in zip(cases, mels):
            w = ref.RefWhisper(path, n_threads=n_threads, log_level=0)
            w.set_mel_any(mel.cpu().numpy())
            want.append(mk.detect(w))
            w.close()
            assert want[-1][0] == c["winner_id"], c["name"]
        ctx.encode_windows(_windows_with_idle_slots(mels))
        p_all, best_all = ctx.lang_detect()
        for i, (c, mel) in enumerate(zip(cases, mels)):
            ctx.encode(mel)
            p1, best1 = ctx.lang_detect()
            for p, best, how in ((p1[0], best1[0], "batch 1"), (p_all[2 * i], best_all[2 * i], "one batch")):
                winner, rp, rlp, _ = want[i]
                assert np.array_equal(p.view(np.uint32), rp.view(np.uint32)), (c["name"], how, float(np.abs(p - rp).max()))
                assert best == winner == c["winner_id"], (c["name"], how)
                hb, hlp = api.finish_language_probs(p)
                assert hb == winner and np.array_equal(hlp.view(np.uint32), rlp.view(np.uint32)), (c["name"], how)
        ctx.close()
        # hypothesis groups: the first sequence of every group speaks for its window
        ctx = binding.HipContext(m, 1, hypotheses=5)
        ctx.set_flags(binding.WH_FLAG_PARITY_EXACT, n_threads)
        ctx.encode(mels[0])
        p5, best5 = ctx.lang_detect()
        assert np.array_equal(p5[0].view(np.uint32), want[0][1].view(np.uint32)) and best5[0] == want[0][0]
        ctx.close()
        m.close()


def test_lang_detect_exact_mode_at_the_large_v3_shape(ref_lib_available, tmp_path):
    """128 mel bins and the 51866-entry vocabulary: 100 language tokens behind sot = 50258. The reference's own whisper_lang_auto_detect cannot be asked
    at this shape (it takes a vocabulary for multilingual only at exactly 51865 entries, so its sot and language tokens sit one id lower): the oracle is
    its decoder, as in test_large_v3_shape -- [sot] at position 0 through whisper_decode on the device's spectrogram (ref_set_mel_any), the probabilities
    at the 100 language columns bit for bit."""
    if not ref_lib_available:
        pytest.skip("oracle/_ref/libwhisper_ref.so not present")
    import bench
    from whisper_amd import api
    model = gf.synth_model("test-d128-v3", seed=77, attn_sharpness=2.0)
    sot = gf.special_tokens(model.hparams)["sot"]
    assert sot == 50258 and model.hparams.n_vocab == 51866
    path = str(tmp_path / "v3.bin")
    gf.write_model(path, model)
    m = binding.HipModel.from_ggml(model)
    assert m.lang_count() == 100
    ctx = binding.HipContext(m, 1)
    ctx.set_flags(binding.WH_FLAG_PARITY_EXACT, 2)
    mel = ctx.mel_spectrogram(dev(bench.synth_pcm(1, seed=100)[0]))
    ctx.encode(mel)
    p, best = ctx.lang_detect()
    w = ref.RefWhisper(path, n_threads=2, log_level=0)
    w.set_mel_any(mel.cpu().numpy())
    w.encode(0)
    _, rp = w.decode([sot], 0)
    w.close()
    rp = np.ascontiguousarray(rp[-1][sot + 1:sot + 101])
    assert p.shape == (1, 100)
    assert np.array_equal(p[0].view(np.uint32), rp.view(np.uint32)), float(np.abs(p[0] - rp).max())
    assert best[0] == int(np.argmax(rp))
    hb, hlp = api.finish_language_probs(p[0][:99])                                # the host half looks at the 99 languages of the table
    assert hb == int(np.argmax(rp[:99])) and abs(float(hlp.sum()) - 1.0) < 1e-5
    ctx.close()
    m.close()


def test_lang_detect_timed_path_within_the_references_own_movement():
    """The timed kernels, every fixture case, none left out: the reference's winner, and |p - p_reference(4 threads)| on the language tokens within
    2 x the largest p_spread of the fixture -- p_spread is how far the reference's own p moves when only its thread count (the order of its FP16 P.V
    sums) changes; doubled because the timed path re-orders more than one reduction (the reasoning of tests/test_gpu_exact.py:185-196). lang_probs
    follow from p through a map of slope < 1 and are held to the same number. At batch 1, in one batch with idle slots, and on a hypothesis-group
    context; the language columns of wh_decode's probabilities are the same bits."""
    from whisper_amd import api
    fx = fixture()
    bound = 2.0 * max(c["p_spread"] for c in fx["cases"])
    worst = worst_lp = 0.0
    sp = gf.special_tokens(gf.hparams_for(mk.KIND))
    for seed, cases in _by_seed(fx["cases"]).items():
        m = binding.HipModel.from_ggml(mk.model_for(seed))
        ctx = binding.HipContext(m, 2 * len(cases))
        ctx5 = binding.HipContext(m, 1, hypotheses=5)
        mels = [ctx.mel_spectrogram(dev(mk.pcm_for(c["pcm"]))) for c in cases]
        ctx.encode_windows(_windows_with_idle_slots(mels))
        p_all, best_all = ctx.lang_detect()
        for i, (c, mel) in enumerate(zip(cases, mels)):
            ctx.encode(mel)
            p1, best1 = ctx.lang_detect()
            _, probs = ctx.decode(np.asarray([[sp["sot"]]], np.int32), 0)
            assert np.array_equal(p1[0].view(np.uint32), probs[0, sp["sot"] + 1:sp["sot"] + 100].view(np.uint32))
            ctx5.encode(mel)
            p5, best5 = ctx5.lang_detect()
            rp, rlp = mk.from_bits(c["p_bits"]), mk.from_bits(c["lang_probs_bits"])
            for p, best, how in ((p1[0], best1[0], "batch 1"), (p_all[2 * i], best_all[2 * i], "one batch"), (p5[0], best5[0], "5 hypotheses")):
                d = float(np.abs(p - rp).max())
                hb, hlp = api.finish_language_probs(p)
                dl = float(np.abs(hlp - rlp).max())
                worst, worst_lp = max(worst, d), max(worst_lp, dl)
                print("%-10s %-12s winner %s, max |p - p_reference| %.3e, lang_probs %.3e (bound %.3e)" % (c["name"], how, mk.LANG_CODES[best], d, dl, bound))
                assert best == hb == c["winner_id"], (c["name"], how)
                assert d <= bound and dl <= bound, (c["name"], how, d, dl, bound)
        ctx.close()
        ctx5.close()
        m.close()
    print("timed path: largest |p - p_reference(4 threads)| %.3e, lang_probs %.3e; bound 2 x p_spread = %.3e" % (worst, worst_lp, bound))


# ---------------------------------------------------------------------------------------------------------------------
# 7. / 8. the host library and the command-line tool
# ---------------------------------------------------------------------------------------------------------------------
def _check_segments(case, got):
    want = case["segments"]
    assert len(got) == len(want), (case["name"], [(g["t0"], g["t1"]) for g in got], [(w["t0"], w["t1"]) for w in want])
    for g, w in zip(got, want):
        assert [t["id"] for t in g["tokens"]] == w["tokens"], (case["name"], [t["id"] for t in g["tokens"]], w["tokens"])
        assert g["t0"] == w["t0"] * 100000 and g["t1"] == w["t1"] * 100000, (case["name"], g["t0"], g["t1"], w)      # 10 ms -> 100 ns ticks
        assert g["text"].decode() == w["text"]


def _strip(segs):
    return [(s["t0"], s["t1"], [t["id"] for t in s["tokens"]]) for s in segs]


def test_run_full_auto_matches_whisper_full_auto(tmp_path):
    """iContext::runFull with language "auto" (and with the empty language: key 0), every fixture case: ids, times and segment boundaries of the
    reference's whisper_full( "auto" ); detected_language names the reference's winner; detect_language returns it and its lang_probs. The first
    window is decoded on the encoder output detection left behind: the result equals the run with the language named (the fixture's generator
    asserts that the reference's two runs agree). runStreamed and beam search (width 5): equal to the same call with the winner named."""
    from whisper_amd import api
    fx = fixture()
    bound = 2.0 * max(c["p_spread"] for c in fx["cases"])
    for seed, cases in _by_seed(fx["cases"]).items():
        path = str(tmp_path / ("m%d.bin" % seed))
        gf.write_model(path, mk.model_for(seed))
        model = api.Model(path)
        assert model.is_multilingual()
        for c in cases:
            pcm = mk.pcm_for(c["pcm"])
            kw = dict(flags=api.NO_CONTEXT, prompt=c["prompt"], n_max_text_ctx=c["n_max_text_ctx"])
            ctx = model.create_context()
            assert ctx.detected_language is None
            for lang in ("auto", ""):
                assert ctx.run_full(pcm, language=lang, **kw) == 0
                _check_segments(c, ctx.results())
                code, p = ctx.detected_language
                assert code == c["winner"], (c["name"], code)
                assert abs(p - float(mk.from_bits(c["lang_probs_bits"])[c["winner_id"]])) <= bound
            assert ctx.run_full(pcm, language=c["winner"], **kw) == 0
            _check_segments(c, ctx.results())
            assert ctx.detected_language is None                                   # nothing is detected when the language is named
            code, probs = ctx.detect_language(pcm)
            assert code == c["winner"] and ctx.detected_language[0] == c["winner"]
            want = mk.from_bits(c["lang_probs_bits"])
            assert max(abs(probs[mk.LANG_CODES[i]] - float(want[i])) for i in range(7)) <= bound
            # less than a second of audio: S_FALSE as with a named language, nothing detected
            assert ctx.run_full(pcm[:8000], language="auto", **kw) == 1 and ctx.detected_language is None
            # runStreamed (every window normalised on its own: not the fixture's transcript) and beam search
            hr, _ = ctx.run_streamed(pcm, language=c["winner"], **kw)
            named = _strip(ctx.results())
            hr2, _ = ctx.run_streamed(pcm, language="auto", **kw)
            assert hr == hr2 == 0 and _strip(ctx.results()) == named and len(named) > 0, c["name"]
            assert ctx.run_full(pcm, language=c["winner"], beam_width=5, **kw) == 0
            named = _strip(ctx.results())
            assert ctx.run_full(pcm, language="auto", beam_width=5, **kw) == 0
            assert _strip(ctx.results()) == named and len(named) > 0 and ctx.detected_language[0] == c["winner"], c["name"]
            ctx.close()
        model.close()


def test_detect_language_rejects_bad_offsets_and_english_only_models(tmp_path):
    from whisper_amd import api
    c = fixture()["cases"][0]
    pcm = mk.pcm_for(c["pcm"])
    path = str(tmp_path / "ml.bin")
    gf.write_model(path, mk.model_for(c["seed"]))
    model = api.Model(path)
    ctx = model.create_context()
    for off in (-10, 10 * (len(pcm) // 160)):
        with pytest.raises(api.WhisperError) as e:
            ctx.detect_language(pcm, offset_ms=off)
        assert e.value.hr == 0x80070057                                            # E_INVALIDARG
    code, _ = ctx.detect_language(pcm, offset_ms=3000)
    assert code in mk.LANG_CODES
    ctx.close()
    model.close()
    # an .en model: "auto" behaves as "en" does (the language is not read), detection itself is an error
    path = str(tmp_path / "en.bin")
    en = gf.scripted_model([50363, 1000, 1001, 50463, 50256], 1, kind="test-d128")
    gf.write_model(path, en)
    model = api.Model(path)
    ctx = model.create_context()
    assert not model.is_multilingual()
    assert ctx.run_full(pcm, language="en", flags=api.NO_CONTEXT) == 0
    want = _strip(ctx.results())
    assert ctx.run_full(pcm, language="auto", flags=api.NO_CONTEXT) == 0 and _strip(ctx.results()) == want and ctx.detected_language is None
    with pytest.raises(api.WhisperError):
        ctx.detect_language(pcm)
    ctx.close()
    model.close()


def test_whisper_main_language_auto(tmp_path):
    """whisper-main -l auto on a fixture case: exit 0, the reference's log line names the reference's language, the transcript is the one -l <winner>
    writes; the same with --offset-t 15000. (The tool streams a 16-bit file: its transcript is compared with its own under the named language. The
    frame-0 rule itself is held against the reference in test_run_full_auto_with_an_offset_detects_on_frame_0.)"""
    from whisper_amd import build
    import wave
    c = next(x for x in fixture()["cases"] if len(mk.pcm_for(x["pcm"])) > 30 * 16000)
    pcm = mk.pcm_for(c["pcm"])
    path = str(tmp_path / "m.bin")
    gf.write_model(path, mk.model_for(c["seed"]))
    wav = str(tmp_path / "a.wav")
    with wave.open(wav, "wb") as f:
        f.setnchannels(1)
        f.setsampwidth(2)
        f.setframerate(16000)
        f.writeframes(np.clip(np.round(pcm * 32768.0), -32768, 32767).astype("<i2").tobytes())

    def run(*args):
        r = subprocess.run([build.CLI_BIN, "-m", path, "-f", wav, "-nc"] + list(args), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
        return r.returncode, r.stdout.decode(errors="replace"), r.stderr.decode(errors="replace")

    for extra in ([], ["-ot", "15000"]):
        rc, out, err = run("-l", "auto", *extra)
        assert rc == 0, err[-2000:]
        assert ("auto-detected language: %s (p = " % c["winner"]) in err, err[-2000:]
        rc2, out2, err2 = run("-l", c["winner"], *extra)
        assert rc2 == 0 and out == out2 and len(out.strip()) > 0 and "auto-detected" not in err2
    assert run("-l", "xx")[0] == 3


def test_run_full_auto_with_an_offset_detects_on_frame_0(tmp_path, ref_lib_available):
    """The frame-0 rule against the reference: runFull( "auto", offset_ms = 15000 ) on the fixture's offset case -- a recording whose language token at
    15 s is ANOTHER one than at frame 0 (the generator asserts it, with margins, at 1 / 4 / 8 reference threads) -- names the language of frame 0 and gives
    ids, times and segment boundaries of the reference's whisper_full( "auto" ) with the same offset; a detection at the offset names the other
    language, and under that language the reference's transcript is a different one. Where the oracle is present the same is held against a live run."""
    from whisper_amd import api
    c = fixture()["offset_case"]
    assert c["winner"] != c["winner_at_offset"] and c["transcript_differs_under_the_language_at_the_offset"]
    pcm = mk.pcm_for(c["pcm"])
    path = str(tmp_path / "m.bin")
    gf.write_model(path, mk.model_for(c["seed"]))
    model = api.Model(path)
    ctx = model.create_context()
    kw = dict(flags=api.NO_CONTEXT, prompt=c["prompt"], n_max_text_ctx=c["n_max_text_ctx"], offset_ms=c["offset_ms"])
    assert ctx.run_full(pcm, language="auto", **kw) == 0
    got = ctx.results()
    _check_segments(c, got)
    assert ctx.detected_language[0] == c["winner"]
    assert ctx.detect_language(pcm, offset_ms=c["offset_ms"])[0] == c["winner_at_offset"]
    assert ctx.run_full(pcm, language=c["winner_at_offset"], **kw) == 0 and _strip(ctx.results()) != _strip(got)
    if ref_lib_available:
        w = ref.RefWhisper(path, n_threads=4, log_level=0)
        w.pcm_to_mel(pcm)
        assert mk.LANG_CODES[mk.detect(w, 0)[0]] == c["winner"] and mk.LANG_CODES[mk.detect(w, c["offset_ms"])[0]] == c["winner_at_offset"]
        live = mk.full_range(w, pcm, "auto", c["offset_ms"])
        w.close()
        _check_segments(dict(c, segments=live), got)
    ctx.close()
    model.close()


def test_detect_language_entry_point_in_exact_mode_is_the_reference_bit_for_bit(tmp_path, ref_lib_available):
    """whisperc_detect_language itself (upload, spectrogram, encoder, [sot] step, the device's p, the host half, the copy into the caller's array) with the
    context's device half in WH_FLAG_PARITY_EXACT (whisperc_debug_context_flags): ALL 99 entries of probs bit-equal to the reference's lang_probs, the same
    winner, on every fixture case at offset 0 and on the offset case at 15 s. The reference is fed the device's spectrogram of the same samples (the same
    kernel through the compute layer's own context: the same bits), at the same thread count."""
    if not ref_lib_available:
        pytest.skip("oracle/_ref/libwhisper_ref.so not present")
    from whisper_amd import api
    fx = fixture()
    n_threads = 4
    todo = [(c, 0) for c in fx["cases"]] + [(fx["offset_case"], fx["offset_case"]["offset_ms"])]
    codes = api.language_codes()
    for seed in sorted({c["seed"] for c, _ in todo}):
        gmodel = mk.model_for(seed)
        path = str(tmp_path / ("m%d.bin" % seed))
        gf.write_model(path, gmodel)
        hm = binding.HipModel.from_ggml(gmodel)
        hctx = binding.HipContext(hm, 1)
        model = api.Model(path)
        ctx = model.create_context()
        ctx.set_device_flags(binding.WH_FLAG_PARITY_EXACT, n_threads)
        for c, off in [t for t in todo if t[0]["seed"] == seed]:
            pcm = mk.pcm_for(c["pcm"])
            mel = hctx.mel_spectrogram(dev(pcm))
            w = ref.RefWhisper(path, n_threads=n_threads, log_level=0)
            w.set_mel_any(mel.cpu().numpy())
            winner, _, rlp, _ = mk.detect(w, off)
            w.close()
            code, probs = ctx.detect_language(pcm, offset_ms=off)
            got = np.asarray([probs[k] for k in codes], np.float32)
            assert len(got) == len(rlp) == 99
            assert np.array_equal(got.view(np.uint32), rlp.view(np.uint32)), (c["name"], off, float(np.abs(got - rlp).max()))
            assert code == codes[winner] and ctx.detected_language[0] == code
        ctx.set_device_flags(0, 1)
        ctx.close()
        model.close()
        hctx.close()
        hm.close()


def test_auto_returns_what_a_named_language_returns_where_nothing_is_decoded(tmp_path):
    """Where StreamRun::begin returns before it reads the language -- the SpeedupAudio flag (E_NOTIMPL), an audio_ctx outside the model's (E_INVALIDARG),
    less than a second of audio (S_FALSE) -- "auto" returns exactly what "en" returns and detects nothing (languageDetectionMoot restates begin's three
    conditions: this test keeps the two in step)."""
    from whisper_amd import api
    c = fixture()["cases"][0]
    pcm = mk.pcm_for(c["pcm"])
    path = str(tmp_path / "m.bin")
    gf.write_model(path, mk.model_for(c["seed"]))
    model = api.Model(path)
    ctx = model.create_context()
    speedup = 0x200

    def outcome(lang, **kw):
        try:
            return ctx.run_full(kw.pop("pcm", pcm), language=lang, **kw)
        except api.WhisperError as e:
            return e.hr

    for kw, want in ((dict(flags=api.NO_CONTEXT | speedup), 0x80004001), (dict(flags=api.NO_CONTEXT, audio_ctx=100000), 0x80070057),
                     (dict(flags=api.NO_CONTEXT, pcm=pcm[:8000]), 1), (dict(flags=api.NO_CONTEXT, offset_ms=3000, duration_ms=900), 1)):
        named = outcome("en", **dict(kw))
        assert named == want, (kw.keys(), hex(named))
        assert outcome("auto", **dict(kw)) == named and ctx.detected_language is None, kw.keys()
    runner = model.create_batch_runner(max_slots=2, groups=1)
    hr, res, per = runner.run([pcm[:8000], pcm], language="auto", flags=api.NO_CONTEXT, prompt=c["prompt"], n_max_text_ctx=0)
    assert hr == 0 and per == [1, 0] and runner.languages[0] is None and runner.languages[1][0] == c["winner"]
    runner.close()
    ctx.close()
    model.close()


def test_batch_runner_auto_gives_every_stream_its_own_language(tmp_path, ref_lib_available):
    """iBatchRunner::run with language "auto": (1) per model of the fixture, its cases in one batch -- ids, times and segment boundaries of the reference's
    whisper_full( "auto" ), whisperc_tr_language = the reference's winner; (2) a mixed-language batch on one model -- recordings whose winners differ,
    a piece of a buffer (detected on its own first frame) and one too short to run, fewer slots than streams and more -- every stream's transcript and
    language equal iContext::runFull( "auto" ) on the same samples, and (oracle present) the reference's winner; a named language detects nothing."""
    from whisper_amd import api
    fx = fixture()
    for seed, cases in _by_seed(fx["cases"]).items():
        path = str(tmp_path / ("m%d.bin" % seed))
        gf.write_model(path, mk.model_for(seed))
        model = api.Model(path)
        runner = model.create_batch_runner(max_slots=4, groups=1)
        hr, res, per = runner.run([mk.pcm_for(c["pcm"]) for c in cases], language="auto", flags=api.NO_CONTEXT, prompt=[1000], n_max_text_ctx=0)
        assert hr == 0 and all(p == 0 for p in per)
        for c, r, lang in zip(cases, res, runner.languages):
            _check_segments(c, r)
            assert lang is not None and lang[0] == c["winner"], (c["name"], lang)
        runner.close()
        model.close()
    seed = fx["offset_case"]["seed"]                      # the model whose recordings differ in language
    path = str(tmp_path / "mixed.bin")
    gf.write_model(path, mk.model_for(seed))
    model = api.Model(path)
    bufs = [mk.pcm_for("jfk"), mk.pcm_for("quiet"), mk.pcm_for("mixed")]
    streams = [bufs[0], bufs[1], bufs[2], (bufs[2], 16000 * 12, 0), (bufs[1], 16000 * 9, 16000 * 14), (bufs[0], 0, 8000)]
    ctx = model.create_context()
    want = []
    for s in streams:
        pcm, first, count = (s, 0, 0) if not isinstance(s, tuple) else s
        piece = np.ascontiguousarray(pcm[first:first + count] if count else pcm[first:])
        hr = ctx.run_full(piece, language="auto", flags=api.NO_CONTEXT, prompt=[1000], n_max_text_ctx=0)
        shift = first * 10000000 // 16000
        want.append((hr, ctx.detected_language, [(t0 + shift, t1 + shift, ids) for (t0, t1, ids) in _strip(ctx.results())] if hr == 0 else []))
        if ref_lib_available and hr == 0:
            w = ref.RefWhisper(path, n_threads=4, log_level=0)
            w.pcm_to_mel(piece)
            assert mk.LANG_CODES[mk.detect(w)[0]] == want[-1][1][0]
            w.close()
    ctx.close()
    assert len({w[1][0] for w in want if w[1]}) >= 2 and want[5][0] == 1 and want[5][1] is None
    for slots, groups in ((2, 1), (3, 2), (64, 2)):
        runner = model.create_batch_runner(max_slots=slots, groups=groups)
        hr, res, per = runner.run(streams, language="auto", flags=api.NO_CONTEXT, prompt=[1000], n_max_text_ctx=0)
        assert hr == 0
        for i, w in enumerate(want):
            assert per[i] == w[0] and _strip(res[i] or []) == w[2], (slots, groups, i)
            assert (runner.languages[i][0] if runner.languages[i] else None) == (w[1][0] if w[1] else None), (slots, groups, i, runner.languages[i], w[1])
            if w[1]:                                     # the lock-step batch takes other products than one stream: the timed path's bound on lang_probs
                assert abs(runner.languages[i][1] - w[1][1]) <= 2.0 * max(c["p_spread"] for c in fx["cases"])
        hr, res, per = runner.run(streams[:2], language="en", flags=api.NO_CONTEXT, prompt=[1000], n_max_text_ctx=0)
        assert hr == 0 and runner.languages == [None, None]
        runner.close()
    model.close()
