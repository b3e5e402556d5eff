"""GPU tests of the speech-only filter: the pack kernel (whisper_amd/csrc/speech.hip; wh_speech_pack of include/whisper_hip.h), api.speech_spans, and filtered
runs through Context.run_full / run_streamed, BatchRunner.run / run_split, whisper-main --speech-only and whisper-mgpu -speech-only.

Every comparison is exact: the kernel copies bits, and a filtered run sees the samples an unfiltered run sees on the numpy-packed recording, so its tokens,
probabilities and text are that run's and its times are the restatement's map (tests/speech_spans_ref.py) of that run's times. glibc's log10f and numpy's
float32 log10 may differ by an ulp, so before a recording's spans are compared the restatement must show that no comparison of the decision loop is closer
than 64 float32 ulps (tests/test_vad_cpu.py's rule)."""
import ctypes as C
import importlib.util
import json
import os
import subprocess
import wave
from types import SimpleNamespace

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import speech_spans_ref as S  # noqa: E402
import vad_ref as V  # noqa: E402
from whisper_amd import api, binding, build, ggml_format as gf  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 1024                # uint32 words of a fill pattern on both sides of a destination
FILL = 0xDEADBEEF
MARGIN_ULPS = 64
INVALID = -1                # WH_E_INVALIDARG
E_INVALIDARG, E_NOTIMPL = 0x80070057, 0x80004001
R16 = 16000


# ---------------------------------------------------------------------------------------------------------------------
# the op
# ---------------------------------------------------------------------------------------------------------------------
def random_bits(n, seed):
    """random 32-bit patterns, every 7th a NaN with a random payload (quiet and signalling, both signs)"""
    rng = np.random.default_rng(seed)
    bits = rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)
    nan = (bits[::7] & np.uint32(0x807FFFFF)) | np.uint32(0x7F800000)
    bits[::7] = np.where(nan & np.uint32(0x007FFFFF), nan, nan | np.uint32(1))
    return bits


def device_pack(bits, channels, n_samples, spans, n_out=None, front=0):
    """wh_speech_pack of bits[: n_samples * channels] (uint32 patterns standing for FP32) into a destination between two guard regions; returns
    (rc, destination words, guards intact). front: 16-byte units the source is moved into its buffer."""
    flat = np.ascontiguousarray(np.asarray(spans, np.int64).reshape(-1, 2))
    total = int((flat[:, 1] - flat[:, 0]).sum()) if len(flat) else 0
    n_out = total if n_out is None else n_out
    src = torch.from_numpy(np.concatenate([np.full(4 * front, FILL, np.uint32), bits[:n_samples * channels]]).view(np.int32)).cuda()
    words = max(n_out, 0) * channels
    dst = torch.from_numpy(np.full(2 * GUARD + words, FILL, np.uint32).view(np.int32)).cuda()
    rc = binding.lib().wh_speech_pack(None, C.c_void_p(src.data_ptr() + 16 * front), channels, n_samples, flat.ctypes.data_as(C.c_void_p) if len(flat) else None,
                                      len(flat), C.c_void_p(dst.data_ptr() + 4 * GUARD), n_out)
    torch.cuda.synchronize()
    out = dst.cpu().numpy().view(np.uint32)
    intact = bool((out[:GUARD] == FILL).all() and (out[GUARD + words:] == FILL).all())
    return rc, out[GUARD:GUARD + words].copy(), intact


def op_cases():
    rng = np.random.default_rng(11)
    cases = {
        # one span = the whole buffer
        "whole_1000": (1000, [(0, 1000)]),
        # 40 spans of one frame each, every other frame: one workgroup crosses them all
        "forty_frames": (81 * 256, [(512 * i, 512 * i + 256) for i in range(40)]),
    }
    # a last span that ends at N with N % 4 = 1, 2, 3: the scalar tail
    for r in (1, 2, 3):
        N = 30 * 256 + 100 + r
        assert N % 4 == r
        cases["tail_%d" % r] = (N, [(256, 5 * 256), (20 * 256, N)])
    # 1000 random spans over 10^6 samples, on frame boundaries, the last one ending at N: more than one workgroup, spans crossing workgroup shares
    N = 1000000
    edges = np.sort(rng.choice(np.arange(1, N // 256), 1999, replace=False)) * 256
    spans = [(int(edges[2 * i]), int(edges[2 * i + 1])) for i in range(999)] + [(int(edges[-1]), N)]
    cases["thousand_spans"] = (N, spans)
    return cases


OP_CASES = op_cases()


@pytest.mark.parametrize("channels", [1, 2])
@pytest.mark.parametrize("name", sorted(OP_CASES))
def test_pack_is_the_concatenation_of_the_spans(name, channels):
    n, spans = OP_CASES[name]
    bits = random_bits(n * channels, 5 + channels)
    want = S.pack(bits, spans, channels)
    assert np.isnan(want.view(np.float32)).sum() > 10
    rc, got, intact = device_pack(bits, channels, n, spans)
    assert rc == 0 and intact
    assert got.dtype == np.uint32 and np.array_equal(got, want)
    if name == "thousand_spans":
        assert len(want) > 16384 * 4            # several workgroups
    # the host form is the same launch between an upload and a download
    out = np.full(len(want), FILL, np.uint32)
    flat = np.asarray(spans, np.int64)
    binding.check(binding.lib().wh_speech_pack_host(bits.ctypes.data_as(C.c_void_p), channels, n, flat.ctypes.data_as(C.c_void_p), len(flat),
                                                    out.ctypes.data_as(C.c_void_p), len(want) // channels))
    assert np.array_equal(out, want)


def test_pack_of_spans_off_the_vector_grid():
    """spans a caller made itself, on no 16-byte grid, and a source that is only 4-byte aligned: still the concatenation (copied value by value)"""
    n = 5000
    bits = random_bits(n * 2, 9)
    spans = [(1, 7), (7, 300), (301, 302), (1003, 4999)]
    for channels in (1, 2):
        rc, got, intact = device_pack(bits, channels, n, spans)
        assert rc == 0 and intact and np.array_equal(got, S.pack(bits[:n * channels], spans, channels))
    lib = binding.lib()
    src = torch.from_numpy(bits[:n + 1].view(np.int32)).cuda()
    dst = torch.from_numpy(np.full(2 * GUARD + 512, FILL, np.uint32).view(np.int32)).cuda()
    flat = np.asarray([(256, 768)], np.int64)
    binding.check(lib.wh_speech_pack(None, C.c_void_p(src.data_ptr() + 4), 1, n, flat.ctypes.data_as(C.c_void_p), 1, C.c_void_p(dst.data_ptr() + 4 * GUARD), 512))
    torch.cuda.synchronize()
    out = dst.cpu().numpy().view(np.uint32)
    assert np.array_equal(out[GUARD:GUARD + 512], bits[257:769]) and (out[:GUARD] == FILL).all() and (out[GUARD + 512:] == FILL).all()


def test_pack_refuses_bad_calls_without_a_launch():
    n = 4096
    bits = random_bits(n, 3)
    good = [(0, 256), (512, 1024)]

    def refused(channels, n_samples, spans, n_out):
        rc, got, intact = device_pack(bits, channels, n_samples, spans, n_out=n_out)
        assert intact and (got == FILL).all(), "a refused call wrote"
        return rc
    assert refused(1, n, good, 768 + 1) == INVALID and refused(1, n, good, 767) == INVALID          # nOut is not the total
    assert refused(1, n, [(512, 1024), (0, 256)], 768) == INVALID                                    # not ascending
    assert refused(1, n, [(0, 512), (256, 1024)], 1280) == INVALID                                   # overlapping
    assert refused(1, n, [(0, 256), (3840, 4097)], 513) == INVALID                                   # past the end
    assert refused(1, n, [(-256, 256)], 512) == INVALID                                              # before the start
    assert refused(1, n, [(256, 256)], 0) == INVALID and refused(1, n, [(512, 256)], 0) == INVALID   # empty, reversed
    assert refused(3, n // 4, good, 768) == INVALID and refused(0, n, good, 768) == INVALID          # channels
    assert refused(1, -1, [], 0) == INVALID
    lib = binding.lib()
    dst = torch.from_numpy(np.full(1024, FILL, np.uint32).view(np.int32)).cuda()
    src = torch.from_numpy(bits.view(np.int32)).cuda()
    flat = np.asarray(good, np.int64)
    fp = flat.ctypes.data_as(C.c_void_p)
    assert lib.wh_speech_pack(None, None, 1, n, fp, 2, C.c_void_p(dst.data_ptr()), 768) == INVALID
    assert lib.wh_speech_pack(None, C.c_void_p(src.data_ptr()), 1, n, fp, 2, None, 768) == INVALID
    assert lib.wh_speech_pack(None, C.c_void_p(src.data_ptr() + 2), 1, n, fp, 2, C.c_void_p(dst.data_ptr()), 768) == INVALID
    assert lib.wh_speech_pack(None, C.c_void_p(src.data_ptr()), 1, n, None, 2, C.c_void_p(dst.data_ptr()), 768) == INVALID
    many = np.asarray([(2 * i, 2 * i + 1) for i in range(65537)], np.int64)
    assert lib.wh_speech_pack(None, C.c_void_p(src.data_ptr()), 1, 200000, many.ctypes.data_as(C.c_void_p), 65537, C.c_void_p(dst.data_ptr()), 65537) == INVALID
    assert lib.wh_speech_pack_host(None, 1, n, fp, 2, None, 768) == INVALID
    torch.cuda.synchronize()
    assert (dst.cpu().numpy().view(np.uint32) == FILL).all()
    # no spans: success, nothing is touched -- not even null buffers
    rc, got, intact = device_pack(bits, 1, n, [], n_out=0)
    assert rc == 0 and intact
    assert lib.wh_speech_pack(None, None, 2, n, None, 0, None, 0) == 0
    assert lib.wh_speech_pack(None, C.c_void_p(src.data_ptr()), 1, n, None, 0, C.c_void_p(dst.data_ptr()), 0) == 0
    torch.cuda.synchronize()
    assert (dst.cpu().numpy().view(np.uint32) == FILL).all()


# ---------------------------------------------------------------------------------------------------------------------
# the recording, its spans, the model
# ---------------------------------------------------------------------------------------------------------------------
def _generator():
    spec = importlib.util.spec_from_file_location("make_golden_runfull", os.path.join(ROOT, "tests", "golden", "make_golden_runfull.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def quantise(raw):
    """what a 16-bit WAV file holds"""
    q = np.clip(np.round(raw * 32768.0), -32768, 32767).astype("<i2")
    return q, q.astype(np.float32) / np.float32(32768.0)


def restated_spans(pcm, *params):
    feat, _ = V.features(pcm)
    speech, _, margin = V.decide(feat)
    return S.spans(speech, len(pcm), *params), margin


@pytest.fixture(scope="module")
def rec():
    """The recording R and what the restatement says about it -- computed once, shared, left unchanged. Asserted before the device is touched."""
    mg = _generator()
    pieces = [mg.pcm_for("jfk"), mg.pcm_for("mixed")[:int(9.3 * R16)], mg.pcm_for("jfk")[:6 * R16]]
    raw, _ = V.composite(pieces, [3.0, 4.5, 2.6], 40, lead=2.7)
    q, pcm = quantise(raw)
    spans, margin = restated_spans(pcm)
    kept = S.offsets(spans)[-1]
    print("R: %.2f s, margin %.1f ulps, spans %s, %.2f s kept" % (len(pcm) / R16, margin, [(a / R16, b / R16) for a, b in spans], kept / R16))
    assert margin > MARGIN_ULPS
    assert len(spans) >= 2 and len(pcm) - kept >= 5 * R16
    packed = S.pack(pcm, spans)
    for a in (pcm, packed, q):
        a.setflags(write=False)
    return SimpleNamespace(mg=mg, pcm=pcm, q=q, spans=spans, packed=packed)


@pytest.fixture(scope="module")
def lib(tmp_path_factory, rec):
    path = str(tmp_path_factory.mktemp("speech") / "cond.bin")
    gf.write_model(path, rec.mg.model_for(10))
    m = api.Model(path)
    yield SimpleNamespace(path=path, model=m)
    m.close()


def key(segs, with_token_times=False):
    return [(s["t0"], s["t1"], s["text"], [t["id"] for t in s["tokens"]], [t["p"] for t in s["tokens"]],
             [(t["t0"], t["t1"]) for t in s["tokens"]] if with_token_times else None) for s in segs]


def mapped(segs, spans, with_token_times=False):
    """the restatement's map of an unfiltered run's results on the packed recording: t0 by the start rule, t1 by the end rule"""
    return [(S.start_ticks(spans, s["t0"]), S.end_ticks(spans, s["t1"]), s["text"], [t["id"] for t in s["tokens"]], [t["p"] for t in s["tokens"]],
             [(S.start_ticks(spans, t["t0"]), S.end_ticks(spans, t["t1"])) for t in s["tokens"]] if with_token_times else None) for s in segs]


def test_api_speech_spans_against_the_restatement(rec):
    assert api.speech_spans(rec.pcm) == rec.spans
    z = V.recordings()["zeros_in_the_middle"]
    want, margin = restated_spans(z)
    assert margin > MARGIN_ULPS and len(want) >= 1
    assert api.speech_spans(z) == want
    # other parameters reach the rules (seconds, rounded to frames); bad ones are refused
    want, _ = restated_spans(rec.pcm, 30, 5, 3)
    assert api.speech_spans(rec.pcm, min_silence=0.48, min_speech=0.08, pad=0.048) == want and want != rec.spans
    assert api.speech_spans(np.zeros(5 * R16, np.float32)) == [] and api.speech_spans(np.zeros(100, np.float32)) == []
    with pytest.raises(api.WhisperError) as e:
        api.speech_spans(rec.pcm, pad=-1.0)
    assert e.value.hr == E_INVALIDARG
    with pytest.raises(api.WhisperError):
        api.speech_spans(rec.pcm, min_silence=20000.0)


# ---------------------------------------------------------------------------------------------------------------------
# end to end
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["greedy", "beam2", "align"])
def test_run_full_is_the_unfiltered_run_on_the_packed_recording(rec, lib, mode):
    kw = dict(beam_width=2) if mode == "beam2" else dict(flags=api.ALIGN_TOKENS) if mode == "align" else {}
    tt = mode == "align"
    plain = lib.model.create_context()
    assert plain.run_full(rec.packed, **kw) == 0
    on_packed = plain.results()
    assert plain.speech_spans() == []
    assert plain.run_full(rec.pcm, **kw) == 0
    unfiltered = plain.results()
    plain.close()
    ctx = lib.model.create_context()
    ctx.set_speech_filter()
    assert ctx.run_full(rec.pcm, **kw) == 0
    got = ctx.results()
    assert ctx.speech_spans() == rec.spans
    ctx.close()
    assert len(on_packed) >= 2
    assert key(got, tt) == mapped(on_packed, rec.spans, tt)
    if tt:
        assert any(t["t1"] > t["t0"] > 0 for s in got for t in s["tokens"])
    assert [s["text"] for s in got] != [s["text"] for s in unfiltered]
    for s in got:
        assert any(a * 625 <= s["t0"] < b * 625 for a, b in rec.spans), s["t0"]
        assert s["t0"] <= s["t1"]
    # the times are the recording's, not the packed copy's: the first span begins 2.4 s into the recording
    assert all(g["t0"] > p["t0"] for g, p in zip(got, on_packed))


def test_run_streamed_is_the_unfiltered_streamed_run_on_the_packed_recording(rec, lib):
    plain = lib.model.create_context()
    hr, progress_plain = plain.run_streamed(rec.packed)
    assert hr == 0
    on_packed = plain.results()
    plain.close()
    ctx = lib.model.create_context()
    ctx.set_speech_filter()
    hr, progress = ctx.run_streamed(rec.pcm)
    assert hr == 0
    assert key(ctx.results()) == mapped(on_packed, rec.spans) and len(on_packed) >= 2
    assert ctx.speech_spans() == rec.spans
    # progress counts packed frames
    assert progress == progress_plain
    ctx.close()


def test_one_span_is_the_unfiltered_run_and_off_is_off(rec, lib):
    """min_silence so large that one span covers the recording (the pads reach both ends): the unfiltered results bit for bit. After set_speech_filter(None)
    the context decodes as one that never set it."""
    never = lib.model.create_context()
    assert never.run_full(rec.pcm) == 0
    want = key(never.results())
    hr, _ = never.run_streamed(rec.pcm)
    want_streamed = key(never.results())
    ctx = lib.model.create_context()
    ctx.set_speech_filter(min_silence=100.0, pad=5.0)
    assert ctx.run_full(rec.pcm) == 0
    assert ctx.speech_spans() == [(0, len(rec.pcm))] and key(ctx.results()) == want
    hr, _ = ctx.run_streamed(rec.pcm)
    assert hr == 0 and key(ctx.results()) == want_streamed
    ctx.set_speech_filter()
    assert ctx.run_full(rec.pcm) == 0 and key(ctx.results()) != want
    ctx.set_speech_filter(None)
    assert ctx.run_full(rec.pcm) == 0
    assert key(ctx.results()) == want and ctx.speech_spans() == []
    ctx.close()
    never.close()


def test_a_context_that_turned_the_filter_off_captures_what_a_fresh_one_does(rec, lib):
    """wh_debug_step_captures through the compute layer: the filter's device work (features, pack) sits in front of the spectrogram and captures no decode step;
    the same decode sequence on a context that ran wh_context_speech_filter and on one that did not instantiates the same number of graphs."""
    model = rec.mg.model_for(10)
    hm = binding.HipModel.from_ggml(model)
    sp = gf.special_tokens(model.hparams)
    counts = []
    for use_filter in (False, True):
        c = binding.HipContext(hm, 1)
        pcm_dev = torch.from_numpy(rec.pcm.copy()).cuda()
        source = pcm_dev
        if use_filter:
            packed, n_packed = C.c_void_p(), C.c_int64()
            flat = np.zeros((64, 2), np.int64)
            count = C.c_int32()
            torch.cuda.synchronize()
            binding.check(binding.lib().wh_context_speech_filter(c.handle, C.c_void_p(pcm_dev.data_ptr()), len(rec.pcm), None, None, C.byref(packed), None,
                                                                 C.byref(n_packed), flat.ctypes.data_as(C.c_void_p), 64, C.byref(count)))
            assert [tuple(int(v) for v in r) for r in flat[:count.value]] == rec.spans and n_packed.value == len(rec.packed)
            got = np.zeros(n_packed.value, np.float32)
            binding.check(binding.lib().wh_buffer_download(c.handle, got.ctypes.data_as(C.c_void_p), packed, 4 * n_packed.value))
            assert np.array_equal(got.view(np.uint32), rec.packed.view(np.uint32))
            source = torch.from_numpy(got).cuda()
        else:
            source = torch.from_numpy(rec.packed.copy()).cuda()
        before = c.step_captures()
        mel = c.mel_spectrogram(source)
        c.encode(mel)
        c.decode_window_start(np.asarray([[sp["sot"]]], np.int32), 6, force_first_timestamp=True, first_is_initial=True)
        ids, ps = c.decode_window_finish()
        counts.append((before, c.step_captures(), ids.tolist(), ps.tolist()))
        c.close()
    hm.close()
    assert counts[0] == counts[1]


def test_no_speech_short_speech_and_the_refusals(rec, lib):
    ctx = lib.model.create_context()
    ctx.set_speech_filter()
    # an all-zero recording: hr 0, no segment; so is one shorter than a frame
    assert ctx.run_full(np.zeros(8 * R16, np.float32)) == 0 and ctx.results() == [] and ctx.speech_spans() == []
    hr, _ = ctx.run_streamed(np.zeros(8 * R16, np.float32))
    assert hr == 0 and ctx.results() == []
    assert ctx.run_full(np.zeros(100, np.float32)) == 0 and ctx.results() == []
    # less than a second of packed speech: the loop's own S_FALSE. 0.5 s of the clip between silences, padded by 2 frames
    short = np.concatenate([V.gap(3.0, 1), rec.mg.pcm_for("jfk")[2 * R16:int(2.5 * R16)], V.gap(3.0, 2)]).astype(np.float32)
    spans, margin = restated_spans(short, 125, 16, 2)
    assert margin > MARGIN_ULPS and 0 < S.offsets(spans)[-1] < R16, spans
    ctx.set_speech_filter(pad=0.032)
    assert ctx.run_full(short) == 1 and ctx.results() == [] and ctx.speech_spans() == spans
    ctx.set_speech_filter()
    # the refusals, each a new combination
    for kw in (dict(offset_ms=1000), dict(duration_ms=5000)):
        with pytest.raises(api.WhisperError) as e:
            ctx.run_full(rec.pcm, **kw)
        assert e.value.hr == E_INVALIDARG
    with pytest.raises(api.WhisperError) as e:
        ctx.run_full(rec.pcm, flags=api.TOKEN_TIMESTAMPS)
    assert e.value.hr == E_NOTIMPL
    for bad in (dict(min_silence=-1.0), dict(pad=20000.0)):
        with pytest.raises(api.WhisperError) as e:
            ctx.set_speech_filter(**bad)
        assert e.value.hr == E_INVALIDARG
    # a refused set leaves the filter as it was; the run after the refusals is the filtered run
    assert ctx.run_full(rec.pcm) == 0 and ctx.speech_spans() == rec.spans
    ctx.set_speech_filter(None)
    assert ctx.run_full(rec.pcm, offset_ms=1000) == 0
    ctx.close()


def test_speakers_are_answered_on_the_original_stereo(rec, lib):
    """The left channel carries the first piece, the right channel the rest: the labels of the filtered run are those the original stereo PCM gives at the
    mapped times, not those of the packed positions."""
    n = len(rec.pcm)
    st = np.zeros((n, 2), np.float32)
    cut = (rec.spans[0][1] + rec.spans[1][0]) // 2
    st[:cut, 0] = rec.pcm[:cut]
    st[cut:, 1] = rec.pcm[cut:]
    ctx = lib.model.create_context()
    ctx.set_speech_filter()
    assert ctx.run_full(rec.pcm, stereo=st) == 0
    segs, labels = ctx.results(), ctx.speakers()
    ctx.close()
    assert len(labels) == len(segs) >= 3
    for s, label in zip(segs, labels):
        if s["t1"] <= cut * 625:
            assert label == api.SPEAKER_LEFT, (s["t0"], s["t1"])
        elif s["t0"] >= cut * 625:
            assert label == api.SPEAKER_RIGHT, (s["t0"], s["t1"])
    assert api.SPEAKER_LEFT in labels and api.SPEAKER_RIGHT in labels


def test_batch_runner_filters_every_stream_with_its_own_map(rec, lib):
    zeros = np.zeros(6 * R16, np.float32)
    part = np.ascontiguousarray(rec.pcm[:20 * R16])
    runner = lib.model.create_batch_runner(max_slots=2, groups=1)
    hr, never, _ = runner.run([rec.pcm, zeros, part])
    assert hr == 0
    runner.set_speech_filter()
    hr, got, per = runner.run([rec.pcm, zeros, part])
    assert hr == 0 and per == [0, 0, 0]
    ctx = lib.model.create_context()
    ctx.set_speech_filter()
    for pcm, g, spans in zip((rec.pcm, zeros, part), got, runner.speech_spans):
        assert ctx.run_full(pcm) == 0
        assert key(g) == key(ctx.results()) and spans == ctx.speech_spans()
    assert got[1] == [] and len(got[0]) >= 3 and len(got[2]) >= 1
    assert key(got[0]) != key(never[0])
    # a piece of a buffer: the piece's own spans and map, then the piece's offset
    first = 10 * R16
    hr, piece, per = runner.run([(rec.pcm, first, 25 * R16)])
    assert hr == 0 and ctx.run_full(np.ascontiguousarray(rec.pcm[first:first + 25 * R16])) == 0
    want = [(t0 + first * 625, t1 + first * 625) + tuple(rest[:-1]) for (t0, t1, *rest) in key(ctx.results())]
    assert [k[:-1] for k in key(piece[0])] == want and len(want) >= 1
    assert runner.speech_spans[0] == ctx.speech_spans()
    # refused per stream; off again: the runner that never set it
    with pytest.raises(api.WhisperError):
        runner.run([rec.pcm], flags=api.TOKEN_TIMESTAMPS)
    runner.set_speech_filter(None)
    hr, back, _ = runner.run([rec.pcm, zeros, part])
    assert hr == 0 and [key(b) for b in back] == [key(x) for x in never]
    ctx.close()
    runner.close()


@pytest.fixture(scope="module")
def long_rec(rec):
    """69.7 s: the pieces of R with longer silences between them, so that the planner cuts inside silences, the pieces' ends are trimmed and the last piece
    holds no speech at all"""
    mg = rec.mg
    pieces = [mg.pcm_for("jfk"), mg.pcm_for("mixed")[:int(15.3 * R16)], mg.pcm_for("jfk"), mg.pcm_for("jfk")[:int(8.0 * R16)]]
    raw, _ = V.composite(pieces, [6.0, 5.0, 7.0, 4.4], 41, lead=2.0)
    q, pcm = quantise(raw)
    assert 69 * R16 < len(pcm) < 70 * R16
    return SimpleNamespace(q=q, pcm=pcm)


def test_run_split_filters_the_pieces_one_by_one(rec, lib, long_rec, tmp_path):
    pcm = long_rec.pcm
    plan = api.plan_chunks(pcm)
    assert len(plan) == 4
    ctx = lib.model.create_context()
    ctx.set_speech_filter()
    want, trimmed, silent = [], 0, 0
    for f, c in plan:
        piece = np.ascontiguousarray(pcm[f:f + c])
        spans, margin = restated_spans(piece)
        assert margin > MARGIN_ULPS
        assert ctx.run_full(piece, flags=api.NO_CONTEXT) == 0 and ctx.speech_spans() == spans
        trimmed += c - S.offsets(spans)[-1]
        silent += not spans
        want.append([(t0 + f * 625, t1 + f * 625) + tuple(rest[:-1]) for (t0, t1, *rest) in key(ctx.results())])
    ctx.close()
    assert trimmed >= 15 * R16 and silent == 1 and want[-1] == []
    runner = lib.model.create_batch_runner(max_slots=4, groups=1)
    runner.set_speech_filter()
    hr, got, per, got_plan = runner.run_split(pcm)
    assert hr == 0 and got_plan == plan
    hr2, as_run, per2 = runner.run([(pcm, f, c) for f, c in plan], flags=api.NO_CONTEXT)
    assert hr2 == 0 and per == per2
    assert [key(g) for g in got] == [key(g) for g in as_run]
    assert [[k[:-1] for k in key(g)] for g in got] == want and sum(len(w) for w in want) >= 4
    runner.close()

    # whisper-mgpu -split silence -speech-only prints that transcript with those times
    wav = str(tmp_path / "long.wav")
    write_wav(wav, long_rec.q)
    out = str(tmp_path / "mgpu.txt")
    r = subprocess.run([build.MGPU_BIN, "-n", "1", "-m", lib.path, "-f", wav, "-o", out, "-timeout", "60", "-job-timeout", "240", "-split", "silence", "-speech-only"],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    print(r.stdout.decode(), r.stderr.decode()[-1500:])
    assert r.returncode == 0
    lines = open(out).read().splitlines()
    segs = [s for g in got for s in g]
    assert len(lines) == len(segs)
    for ln, s in zip(lines, segs):
        assert ln.endswith("] " + s["text"].decode()), (ln, s["text"])
        t0, t1 = float(ln[1:10]), float(ln[15:24])
        assert abs(t0 - s["t0"] / 1e7) < 0.006 and abs(t1 - s["t1"] / 1e7) < 0.006
    bad = subprocess.run([build.MGPU_BIN, "-n", "1", "-m", lib.path, "-f", wav, "-so-pad", "0.1"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    assert bad.returncode == 1 and b"need -speech-only" in bad.stderr


def write_wav(path, q):
    with wave.open(path, "wb") as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(16000)
        w.writeframes(q.tobytes())


def seconds_of(stamp):
    h, m, s = stamp.split(":")
    return int(h) * 3600 + int(m) * 60 + float(s)


def test_whisper_main_takes_the_option(rec, lib, tmp_path):
    """whisper-main --speech-only prints the filtered streamed run (the tool streams its input): the same text, the recording's times; the --so options reach
    the rules; without the option the unfiltered transcript."""
    wav = str(tmp_path / "rec.wav")
    write_wav(wav, rec.q)
    runs = {}
    for name, setting in (("plain", None), ("default", {}), ("tuned", dict(min_silence=1.0, min_speech=0.128, pad=0.16))):
        ctx = lib.model.create_context()                    # a fresh one, like the tool's
        if setting is not None:
            ctx.set_speech_filter(**setting)
        hr, _ = ctx.run_streamed(rec.pcm, flags=api.NO_CONTEXT)
        assert hr == 0
        runs[name] = ctx.results()
        ctx.close()
    assert [s["text"] for s in runs["default"]] != [s["text"] for s in runs["plain"]]

    def tool(*extra):
        r = subprocess.run([build.CLI_BIN, "-m", lib.path, "-f", wav, "-l", "en", "-nc"] + list(extra), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
        assert r.returncode == 0, r.stderr.decode(errors="replace")[-2000:]
        out = []
        for ln in r.stdout.decode().splitlines():
            if ln.startswith("[") and " --> " in ln and "]  " in ln:
                stamps, text = ln[1:].split("]  ", 1)
                a, b = stamps.split(" --> ")
                out.append((seconds_of(a), seconds_of(b), text))
        return out

    for name, extra in (("plain", ()), ("default", ("--speech-only",)), ("tuned", ("--speech-only", "--so-min-silence", "1.0", "--so-min-speech", "0.128", "--so-pad", "0.16"))):
        got, want = tool(*extra), runs[name]
        assert len(got) == len(want) >= 3, name
        for (t0, t1, text), s in zip(got, want):
            assert text == s["text"].decode() and abs(t0 - s["t0"] / 1e7) < 0.006 and abs(t1 - s["t1"] / 1e7) < 0.006, (name, t0, t1, s)
    bad = subprocess.run([build.CLI_BIN, "-m", lib.path, "-f", wav, "--so-pad", "0.1"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    assert bad.returncode == 2 and b"need --speech-only" in bad.stderr
    refused = subprocess.run([build.CLI_BIN, "-m", lib.path, "-f", wav, "-nc", "--speech-only", "-ot", "1000"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert refused.returncode == 10
    usage = subprocess.run([build.CLI_BIN, "-h"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=60)
    assert "speech-only" not in usage.stdout + usage.stderr
