"""CPU tests of the speech-only filter's host rules: the span rules and the time map of whisper_amd/host/speechSpans.h through a stand-alone driver built
with the address and undefined-behaviour sanitizers, against the restatement of tests/speech_spans_ref.py; the declarations of the public faces. The pack
kernel and the filtered runs are tested in tests/test_gpu_speech_filter.py."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import speech_spans_ref as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = os.path.join(ROOT, "tests", "_build")
E_INVALIDARG = "failed 0x80070057"


@pytest.fixture(scope="module")
def driver():
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    os.makedirs(BUILD, exist_ok=True)
    exe = os.path.join(BUILD, "speech-spans-driver")
    src = os.path.join(ROOT, "tests", "speech_spans_cpu", "driver.cpp")
    host = os.path.join(ROOT, "whisper_amd", "host")
    deps = [src, os.path.join(host, "vad.h"), os.path.join(host, "speechSpans.h"), os.path.join(ROOT, "include", "whisperApi.h")]
    if not os.path.exists(exe) or any(os.path.getmtime(d) > os.path.getmtime(exe) for d in deps):
        r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I" + host,
                            "-I" + os.path.join(ROOT, "include"), src, "-o", exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        assert r.returncode == 0, r.stdout
    return exe


def run_driver(exe, tmp_path, speech, N, params=(0, 0, 0), queries=None):
    path = str(tmp_path / "flags.bin")
    with open(path, "wb") as f:
        f.write(np.ascontiguousarray(speech, np.uint8).tobytes())
    args = [exe, "spans" if queries is None else "map", path, str(N)] + [str(p) for p in params]
    if queries is not None:
        qpath = str(tmp_path / "queries.bin")
        with open(qpath, "wb") as f:
            f.write(np.ascontiguousarray(queries, "<i8").tobytes())
        args.append(qpath)
    r = subprocess.run(args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    out = r.stdout.splitlines()
    if not out[0].startswith("ok "):
        return out[0], None
    n = int(out[0].split()[1])
    spans = [tuple(int(v) for v in ln.split()) for ln in out[1:1 + n]]
    if queries is None:
        assert len(out) == 1 + n
        return spans, None
    assert out[1 + n] == "packed %d" % S.offsets(spans)[-1]
    rows = [tuple(int(v) for v in ln.split()) for ln in out[2 + n:]]
    assert len(rows) == len(queries)
    return spans, rows


def check_shape(spans, N):
    """ascending, disjoint, not touching, inside [0, N]; starts on frames, ends on frames except that the last may be N"""
    prev = -1
    for i, (a, b) in enumerate(spans):
        assert 0 <= a < b <= N and a > prev
        assert a % 256 == 0
        assert b % 256 == 0 or (i == len(spans) - 1 and b == N)
        prev = b


def random_flags(n, seed):
    """choppy flags: long stretches of speech and silence with single-frame flips inside both"""
    rng = np.random.default_rng(seed)
    flags = np.zeros(n, np.uint8)
    pos, on = 0, False
    while pos < n:
        length = int(rng.integers(1, 400))
        if on:
            flags[pos:pos + length] = 1
        pos += length
        on = not on
    flips = rng.random(n) < 0.03
    return flags ^ flips.astype(np.uint8)


@pytest.mark.parametrize("n_frames", [0, 1, 29, 2443, 225000])
@pytest.mark.parametrize("tail", [0, 100])
def test_random_flags_against_the_restatement(driver, tmp_path, n_frames, tail):
    N = n_frames * 256 + tail
    for seed in range(3):
        flags = random_flags(n_frames, 100 * n_frames + seed)
        for params in ((0, 0, 0), (10, 3, 2), (400, 1, 1)):
            want = S.spans(flags, N, *params)
            got, _ = run_driver(exe=driver, tmp_path=tmp_path, speech=flags, N=N, params=params)
            assert got == want, (n_frames, seed, params)
            check_shape(got, N)
    if n_frames >= 2443:
        assert len(S.spans(random_flags(n_frames, 100 * n_frames), N, 10, 3, 2)) >= 2      # the cases are not trivial


def flags_of(n, *runs):
    f = np.zeros(n, np.uint8)
    for a, b in runs:
        f[a:b] = 1
    return f


def test_hand_made_cases(driver, tmp_path):
    def both(flags, N, params=(0, 0, 0)):
        got, _ = run_driver(driver, tmp_path, flags, N, params)
        assert got == S.spans(flags, N, *params)
        return got
    n = 1000
    # all speech, with and without a partial last frame; no speech
    assert both(np.ones(n, np.uint8), n * 256) == [(0, n * 256)]
    assert both(np.ones(n, np.uint8), n * 256 + 255) == [(0, n * 256 + 255)]
    assert both(np.zeros(n, np.uint8), n * 256 + 7) == []
    assert both(np.zeros(0, np.uint8), 255) == []
    # a run of 15 frames is dropped, one of 16 is kept and padded by 25 on both sides
    assert both(flags_of(n, (400, 415)), n * 256) == []
    assert both(flags_of(n, (400, 416)), n * 256) == [(375 * 256, 441 * 256)]
    # short runs merge before they are dropped: 4 runs of 4 frames, 2 apart, make one run of 22
    assert both(flags_of(n, (400, 404), (406, 410), (412, 416), (418, 422)), n * 256) == [(375 * 256, 447 * 256)]
    # a gap of 124 frames merges, one of 125 does not (and its two paddings of 25 do not meet)
    assert both(flags_of(n, (100, 200), (324, 400)), n * 256) == [(75 * 256, 425 * 256)]
    assert both(flags_of(n, (100, 200), (325, 400)), n * 256) == [(75 * 256, 225 * 256), (300 * 256, 425 * 256)]
    # padding that merges neighbours: a gap of 50 frames is exactly two paddings (the runs touch), 51 leaves one frame between them
    assert both(flags_of(n, (100, 200), (250, 300)), n * 256, (40, 16, 25)) == [(75 * 256, 325 * 256)]
    assert both(flags_of(n, (100, 200), (251, 300)), n * 256, (40, 16, 25)) == [(75 * 256, 225 * 256), (226 * 256, 325 * 256)]
    # padding clamped at both ends; the clamped end takes the partial frame
    assert both(flags_of(n, (10, 60), (950, 990)), n * 256 + 9) == [(0, 85 * 256), (925 * 256, n * 256 + 9)]
    # a span that ends before the last frame does not take the partial frame
    assert both(flags_of(n, (100, 200)), n * 256 + 9) == [(75 * 256, 225 * 256)]


def test_parameters_refused(driver, tmp_path):
    flags = flags_of(100, (10, 60))
    for params in ((-1, 0, 0), (0, -1, 0), (0, 0, -1), ((1 << 20) + 1, 0, 0), (0, (1 << 20) + 1, 0), (0, 0, (1 << 20) + 1)):
        assert run_driver(driver, tmp_path, flags, 25600, params)[0] == E_INVALIDARG
        with pytest.raises(ValueError):
            S.spans(flags, 25600, *params)
    assert run_driver(driver, tmp_path, flags, 25600, (1 << 20, 1 << 20, 1 << 20))[0] == []
    # the flags must be the N / 256 frames of N samples
    assert run_driver(driver, tmp_path, flags, 25600 + 256)[0] == E_INVALIDARG
    assert run_driver(driver, tmp_path, flags, -1)[0] == E_INVALIDARG


def test_time_map(driver, tmp_path):
    n = 2443
    N = n * 256 + 100
    flags = flags_of(n, (100, 300), (500, 900), (1200, 1300), (2300, 2443))
    spans = S.spans(flags, N, 60, 16, 25)
    assert len(spans) == 4 and spans[-1][1] == N
    out = S.offsets(spans)
    packed = out[-1]
    rng = np.random.default_rng(5)
    # every join and its neighbours, both ends, and random ticks in between
    samples = sorted({0, 1, packed - 1, packed, packed + 5} | {o + d for o in out for d in (-2, -1, 0, 1, 2) if 0 <= o + d <= packed})
    ticks = [s * 625 + d for s in samples for d in (0, 1, 624)] + [int(t) for t in rng.integers(0, packed * 625, 300)]
    ticks = np.sort(np.asarray(ticks, np.int64))
    got, rows = run_driver(driver, tmp_path, flags, N, (60, 16, 25), ticks)
    assert got == spans
    for t, (st, et, ss, es) in zip(ticks.tolist(), rows):
        assert st == S.start_ticks(spans, t) and et == S.end_ticks(spans, t), t
        assert ss == S.map_start(spans, t // 625) and es == S.map_end(spans, t // 625), t
    # monotone in both rules; an end never lies before the start of the same packed time
    st, et = np.asarray([r[0] for r in rows]), np.asarray([r[1] for r in rows])
    assert (np.diff(st) >= 0).all() and (np.diff(et) >= 0).all()
    # every mapped start of a position inside the packed copy lies inside a span; an end inside one or at its end
    for t, s, e in zip(ticks.tolist(), st.tolist(), et.tolist()):
        if t < packed * 625:
            assert any(a * 625 <= s < b * 625 for a, b in spans), t
        if t <= packed * 625:
            assert any(a * 625 <= e <= b * 625 for a, b in spans), t
        else:                                       # behind the packed copy: as far behind the last span's end
            assert s == e == N * 625 + (t - packed * 625)
    # the join rule: packed position out[i] starts span i, but a range that ENDS there ends where span i - 1 ends
    for i in range(1, len(spans)):
        assert S.map_start(spans, out[i]) == spans[i][0] and S.map_end(spans, out[i]) == spans[i - 1][1]
        assert S.start_ticks(spans, out[i] * 625) == spans[i][0] * 625 and S.end_ticks(spans, out[i] * 625) == spans[i - 1][1] * 625
    # s = 0 and s = the packed length
    assert S.map_start(spans, 0) == S.map_end(spans, 0) == spans[0][0]
    assert S.map_start(spans, packed) == S.map_end(spans, packed) == spans[-1][1] == N


def test_time_map_is_the_identity_under_full_coverage(driver, tmp_path):
    n = 29
    N = n * 256 + 3
    flags = np.ones(n, np.uint8)
    ticks = np.asarray(sorted({0, 1, 624, 625, 626, N * 625 - 1, N * 625} | {int(t) for t in np.random.default_rng(2).integers(0, N * 625, 200)}), np.int64)
    spans, rows = run_driver(driver, tmp_path, flags, N, (0, 0, 0), ticks)
    assert spans == [(0, N)]
    for t, (st, et, ss, es) in zip(ticks.tolist(), rows):
        assert st == t and et == t and ss == es == t // 625
        assert S.start_ticks(spans, t) == t and S.end_ticks(spans, t) == t


# ---------------------------------------------------------------------------------------------------------------------
# declarations: every face names the feature
# ---------------------------------------------------------------------------------------------------------------------
def read(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


def test_declarations():
    api_h = read("include", "whisperApi.h")
    for name in ("struct sSpeechFilter", "setSpeechFilter", "speechSpans", "getSpeechSpans"):
        assert name in api_h, name
    hip_h = read("include", "whisper_hip.h")
    for name in ("wh_speech_pack", "wh_speech_pack_host", "wh_context_speech_filter"):
        assert re.search(r"WH_API int %s\(" % name, hip_h), name
    c_h = read("include", "whisper_c.h")
    for name in ("whisperc_set_speech_filter", "whisperc_speech_spans", "whisperc_result_speech_spans"):
        assert name in c_h, name
    from whisper_amd import binding
    for name in ("wh_speech_pack", "wh_speech_pack_host", "wh_context_speech_filter"):
        assert name in binding.EXPORTS
    assert "speech.hip" in __import__("whisper_amd.build", fromlist=["x"]).HIP_SOURCES
    assert "checkSpeechFilter" in read("whisper_amd", "host", "optionRules.h")


def test_defaults_match_the_header():
    h = read("whisper_amd", "host", "speechSpans.h")
    m = re.search(r"MIN_SILENCE_FRAMES = (\d+), MIN_SPEECH_FRAMES = (\d+), PAD_FRAMES = (\d+)", h)
    assert m and tuple(int(v) for v in m.groups()) == (S.MIN_SILENCE, S.MIN_SPEECH, S.PAD)
    assert "TICKS_PER_SAMPLE = %d" % S.TICKS in h
