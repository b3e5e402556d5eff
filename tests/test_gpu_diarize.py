"""GPU tests of stereo diarization end to end: iContext::detectSpeaker behind Context.run_full / run_streamed / BatchRunner.run (the speakers results carry)
and behind `whisper-main -di` (the labels of the console lines), on the scripted model of tests/golden/ref_hostloop.json that the CLI and host-API tests
use. The yardstick is the restatement of the reference's rule in tests/test_diarize_cpu.py, applied to the segment times the run returned."""
import json
import os
import struct
import subprocess

import numpy as np
import pytest

from whisper_amd import api, build, ggml_format as gf
from test_diarize_cpu import LEFT, NO_STEREO_DATA, OLE_E_BLANK, RIGHT, UNSURE, speakers_of

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "ref_hostloop.json")
LABELS = {LEFT: "(speaker 0)", RIGHT: "(speaker 1)", UNSURE: "(speaker ?)", NO_STEREO_DATA: ""}
# the scripted transcript cuts 9 s into the segments 0 - 2.4 s, 2.4 - 5 s, 5 - 7.2 s, 7.2 - 9.6 s; the loud channel of the recording changes with them
BOUNDS_S = (0.0, 2.4, 5.0, 7.2, 9.0)
LOUD = (LEFT, RIGHT, UNSURE, LEFT)


def stereo_noise(rate, seed):
    """9 s of noise at `rate`: per segment the left channel four times the right, the right four times the left, or both channels the same samples."""
    n = int(BOUNDS_S[-1] * rate)
    rng = np.random.default_rng(seed)
    st = 0.1 * rng.standard_normal((n, 2))
    t = np.arange(n) / rate
    for (a, b), loud in zip(zip(BOUNDS_S, BOUNDS_S[1:]), LOUD):
        m = (t >= a) & (t < b)
        if loud == LEFT:
            st[m, 1] *= 0.25
        elif loud == RIGHT:
            st[m, 0] *= 0.25
        else:
            st[m, 1] = st[m, 0]
    return st


def stamp(t10ms):
    ms = t10ms * 10
    return "%02d:%02d:%02d.%03d" % (ms // 3600000, ms // 60000 % 60, ms // 1000 % 60, ms % 1000)


def write_wav(path, rate, channels, width, frames):
    """frames: float [n, channels] in [-1, 1) -> integer PCM of `width` bytes per sample"""
    scale = 2.0 ** (8 * width - 1)
    q = np.clip(np.round(frames * scale), -scale, scale - 1).astype(np.int64)
    raw = q.astype("<i4").view(np.uint8).reshape(-1, 4)[:, :width].tobytes() if width != 2 else q.astype("<i2").tobytes()
    fmt = struct.pack("<HHIIHH", 1, channels, rate, rate * channels * width, channels * width, 8 * width)
    with open(path, "wb") as f:
        f.write(b"RIFF" + struct.pack("<I", 4 + 8 + len(fmt) + 8 + len(raw)) + b"WAVE" + b"fmt " + struct.pack("<I", len(fmt)) + fmt + b"data" + struct.pack("<I", len(raw)) + raw)


@pytest.fixture(scope="module")
def material(tmp_path_factory):
    d = tmp_path_factory.mktemp("diarize")
    case = [c for c in json.load(open(GOLDEN))["cases"] if c["name"] == "first_window_no_prompt"][0]
    assert case["n_samples"] == 16000 * 9 and [(s["t0"], s["t1"]) for s in case["segments"]] == [(0, 240), (240, 500), (500, 720), (720, 960)]
    out = {"case": case, "model": str(d / "m.bin"), "lang": case["lang"]}
    gf.write_model(out["model"], gf.scripted_model(case["script"], case["prompt_len"]))
    st = stereo_noise(16000, 41).astype(np.float32)
    out["stereo"] = st
    out["mono"] = ((st[:, 0] + st[:, 1]) * np.float32(0.5)).astype(np.float32)
    # the same kind of material at 44.1 kHz in 24 bits with a third, loud channel that diarization must not look at
    hi = stereo_noise(44100, 42)
    third = 0.5 * np.random.default_rng(43).standard_normal((len(hi), 1))
    out["wav3"] = str(d / "three_channels.wav")
    write_wav(out["wav3"], 44100, 3, 3, np.concatenate([hi, third], 1))
    out["wav1"] = str(d / "mono.wav")
    write_wav(out["wav1"], 16000, 1, 2, out["mono"][:, None])
    out["hi"] = hi.astype(np.float32)
    if not os.path.exists(build.CLI_BIN):
        build.build_all()
    out["model_handle"] = api.Model(out["model"])
    yield out
    out["model_handle"].close()


def times(results):
    return [(s["t0"], s["t1"]) for s in results]


def test_results_carry_the_speakers(material):
    """Context.run_full( mono, stereo = st ) and run_streamed: speakers() is the restatement on the returned segment times -- left, right, unsure, left (the last
    segment ends 0.6 s past the end of the recording: zero fill). Without stereo data every segment is 0xFF. detect_speaker outside a run is OLE_E_BLANK."""
    ctx = material["model_handle"].create_context()
    mono, st, lang = material["mono"], material["stereo"], material["lang"]
    want_times = [(s["t0"] * 100000, s["t1"] * 100000) for s in material["case"]["segments"]]
    with pytest.raises(api.WhisperError) as e:
        ctx.detect_speaker(0, 24_000_000)
    assert e.value.hr == OLE_E_BLANK
    assert ctx.run_full(mono, language=lang, flags=api.NO_CONTEXT, stereo=st) == 0
    res = ctx.results()
    assert times(res) == want_times
    want = speakers_of(res, st)
    assert want == list(LOUD)
    assert ctx.speakers() == want
    with pytest.raises(api.WhisperError) as e:                      # the run is over: its audio is no longer current
        ctx.detect_speaker(0, 24_000_000)
    assert e.value.hr == OLE_E_BLANK
    hr, _ = ctx.run_streamed(mono, language=lang, flags=api.NO_CONTEXT, stereo=st)
    assert hr == 0 and times(ctx.results()) == want_times and ctx.speakers() == want
    # the channels the other way round
    assert ctx.run_full(mono, language=lang, flags=api.NO_CONTEXT, stereo=st[:, ::-1]) == 0
    assert ctx.speakers() == [RIGHT, LEFT, UNSURE, RIGHT] == speakers_of(ctx.results(), st[:, ::-1])
    # a part of the recording: offset_ms moves the segments, their speakers follow
    assert ctx.run_full(mono, language=lang, flags=api.NO_CONTEXT, stereo=st, offset_ms=2400) == 0
    res = ctx.results()
    assert res and res[0]["t0"] == 24_000_000 and ctx.speakers() == speakers_of(res, st) and len(set(ctx.speakers())) >= 2
    # no stereo data
    assert ctx.run_full(mono, language=lang, flags=api.NO_CONTEXT) == 0
    assert ctx.speakers() == [NO_STEREO_DATA] * 4
    hr, _ = ctx.run_streamed(mono, language=lang, flags=api.NO_CONTEXT)
    assert hr == 0 and ctx.speakers() == [NO_STEREO_DATA] * 4
    with pytest.raises(ValueError):
        ctx.run_full(mono, language=lang, stereo=st[:-1])
    with pytest.raises(ValueError):
        ctx.run_streamed(mono, language=lang, stereo=st[:, :1])
    ctx.close()


def test_stereo_at_another_sample_rate(material):
    """sample_rate = 44100: the mono and each stereo channel are resampled (api.resample( ..., channel = c )); the speakers are the restatement's on that."""
    ctx = material["model_handle"].create_context()
    hi = material["hi"]
    mono = ((hi[:, 0] + hi[:, 1]) * np.float32(0.5)).astype(np.float32)
    assert ctx.run_full(mono, language=material["lang"], flags=api.NO_CONTEXT, sample_rate=44100, stereo=hi) == 0
    st16 = np.stack([api.resample(hi, 44100, channel=c) for c in range(2)], 1)
    assert st16.shape == (16000 * 9, 2)
    assert ctx.speakers() == speakers_of(ctx.results(), st16) == list(LOUD)
    hr, _ = ctx.run_streamed(mono, language=material["lang"], flags=api.NO_CONTEXT, sample_rate=44100, stereo=hi)
    assert hr == 0 and ctx.speakers() == list(LOUD)
    with pytest.raises(ValueError):
        ctx.run_full(mono, language=material["lang"], sample_rate=44100, stereo=material["stereo"])
    ctx.close()


def test_batch_runner_carries_the_speakers(material):
    """BatchRunner.run: a stereo recording, the same recording without stereo data, its channels swapped, and a piece of it (firstSample > 0): the speakers
    of every stream are the restatement's on the stream's segment times and piece."""
    mono, st, lang = material["mono"], material["stereo"], material["lang"]
    swapped = np.ascontiguousarray(st[:, ::-1])
    first = 16000 * 5
    runner = material["model_handle"].create_batch_runner(max_slots=4, groups=1)
    hr, out, per = runner.run([mono, mono, mono, (mono, first, 0)], language=lang, flags=api.NO_CONTEXT, stereo=[st, None, swapped, st])
    assert hr == 0 and per == [0, 0, 0, 0]
    assert runner.speakers[0] == speakers_of(out[0], st) == list(LOUD)
    assert runner.speakers[1] == [NO_STEREO_DATA] * len(out[1]) and len(out[1]) == 4
    assert runner.speakers[2] == speakers_of(out[2], swapped) == [RIGHT, LEFT, UNSURE, RIGHT]
    assert out[3] and out[3][0]["t0"] == first * 10_000_000 // 16000
    assert runner.speakers[3] == speakers_of(out[3], st[first:], first * 10_000_000 // 16000)
    assert runner.speakers[3][0] == UNSURE and LEFT in runner.speakers[3]
    hr, out, per = runner.run([mono], language=lang, flags=api.NO_CONTEXT)
    assert hr == 0 and runner.speakers == [[NO_STEREO_DATA] * 4]
    runner.close()


def cli(*args):
    r = subprocess.run([build.CLI_BIN] + list(args), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    return r.stdout.decode()


def test_whisper_main_diarize(material):
    """whisper-main -di on a 44.1 kHz, 24-bit, 3-channel WAV: every console line is the reference's `printf( "[%s --> %s]  %s%s\\n" )` with the label of the
    segment's louder channel among the FIRST TWO and no extra blank -- (speaker 0), (speaker 1), (speaker ?), (speaker 0). Without -di the same file prints
    no labels, which is the parent commit's output; a mono file with -di prints none either (its buffer has no stereo data, like the reference's)."""
    segs, model, lang = material["case"]["segments"], material["model"], material["lang"]
    st16 = api.load_audio(material["wav3"], stereo=True)
    assert st16.shape == (16000 * 9, 2)
    want = speakers_of([dict(t0=s["t0"] * 100000, t1=s["t1"] * 100000) for s in segs], st16)
    assert want == list(LOUD)

    def console(labels):
        return "\n" + "".join("[%s --> %s]  %s%s\n" % (stamp(s["t0"]), stamp(s["t1"]), LABELS[k], s["text"]) for s, k in zip(segs, labels))

    plain = console([NO_STEREO_DATA] * len(segs))
    got = cli("-m", model, "-f", material["wav3"], "-l", lang, "-nc", "-di")
    assert got == console(want), got
    assert "(speaker 0)" in got and "(speaker 1)" in got and "(speaker ?)" in got
    assert cli("-m", model, "-f", material["wav3"], "-l", lang, "-nc") == plain
    assert cli("-m", model, "-f", material["wav1"], "-l", lang, "-nc", "-di") == plain
    # token timestamps take the other road through the tool (loadAudioFile + runFull): the same labels
    assert cli("-m", model, "-f", material["wav3"], "-l", lang, "-nc", "-di", "-ml", "1000") == console(want)
