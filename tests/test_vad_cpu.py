"""CPU tests of splitting a long recording at pauses: the voice-activity decision loop (whisper_amd/host/vad.h) and the chunk planner
(whisper_amd/host/chunkPlanner.h) through a stand-alone driver built with the address and undefined-behaviour sanitizers, against the numpy
restatement of tests/vad_ref.py; the library's whisperc_debug_vad_decide through ctypes; whisper-mgpu's -split option. The feature kernel itself
is tested in tests/test_gpu_vad.py.

glibc's log10f and numpy's float32 log10 may differ by an ulp, so before a recording is compared the restatement must show that no comparison of the
loop with finite sides is closer than 64 float32 ulps of its larger operand: the recordings (seeds, gap placement) are chosen so that this holds."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import vad_ref as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = os.path.join(ROOT, "tests", "_build")
MARGIN_ULPS = 64
E_INVALIDARG = "failed 0x80070057"


@pytest.fixture(scope="module")
def driver():
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    os.makedirs(BUILD, exist_ok=True)
    exe = os.path.join(BUILD, "vad-driver")
    src = os.path.join(ROOT, "tests", "vad_cpu", "driver.cpp")
    host = os.path.join(ROOT, "whisper_amd", "host")
    deps = [src, os.path.join(host, "vad.h"), os.path.join(host, "chunkPlanner.h"), os.path.join(ROOT, "include", "whisperApi.h")]
    if not os.path.exists(exe) or any(os.path.getmtime(d) > os.path.getmtime(exe) for d in deps):
        r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I" + host,
                            "-I" + os.path.join(ROOT, "include"), src, "-o", exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        assert r.returncode == 0, r.stdout
    return exe


def run_driver(exe, tmp_path, mode, data, *args):
    path = str(tmp_path / "case.bin")
    with open(path, "wb") as f:
        f.write(data)
    r = subprocess.run([exe, mode, path] + [str(a) for a in args], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    return r.stdout.splitlines()


def driver_decide(exe, tmp_path, feat):
    out = run_driver(exe, tmp_path, "decide", np.ascontiguousarray(feat, "<f4").tobytes())
    n, last = (int(v) for v in out[0].split())
    flags = np.frombuffer((out[1] if len(out) > 1 else "").encode(), np.uint8) - ord("0")
    assert len(flags) == n
    return flags.astype(np.uint8), last


def driver_plan(exe, tmp_path, speech, energy, N, max_len=0, min_len=0, pause_frames=0):
    data = np.ascontiguousarray(speech, np.uint8).tobytes() + np.ascontiguousarray(energy, "<f4").tobytes()
    out = run_driver(exe, tmp_path, "plan", data, N, max_len, min_len, pause_frames)
    if not out[0].startswith("ok "):
        return out[0]
    chunks = [tuple(int(v) for v in ln.split()) for ln in out[1:]]
    assert len(chunks) == int(out[0].split()[1])
    return chunks


# ---------------------------------------------------------------------------------------------------------------------
# recordings of the decision-loop tests (tests/test_gpu_vad.py runs two of them through api.vad)
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cases():
    out = {}
    for name, pcm in V.recordings().items():
        feat, _ = V.features(pcm)
        out[name] = (pcm, feat) + V.decide(feat)
    return out


NAMES = ("composite", "speech_first", "zeros_in_the_middle", "zeros_at_the_start", "fewer_than_30_frames", "no_frames")


@pytest.mark.parametrize("name", NAMES)
def test_decision_loop_against_the_restatement(driver, tmp_path, cases, name):
    pcm, feat, speech, last, margin = cases[name]
    print("%s: %d frames, %d speech, lastSpeech %d, smallest margin %.1f ulps, %d NaN and %d infinite SFM" %
          (name, len(feat), int(speech.sum()), last, margin, int(np.isnan(feat[:, 2]).sum()), int(np.isinf(feat[:, 2]).sum())))
    assert margin > MARGIN_ULPS
    assert len(feat) == len(pcm) // 256
    if name == "zeros_in_the_middle":
        assert np.isnan(feat[:, 2]).sum() >= 20 and (feat[np.isnan(feat[:, 2]), 0] == 0).all()
    if name == "zeros_at_the_start":
        assert feat[0, 0] == 0 and np.isnan(feat[0, 2])
    if name in ("composite", "speech_first", "zeros_in_the_middle"):
        assert 0.2 < speech.mean() < 0.9                     # the loop tells something apart
    got, got_last = driver_decide(driver, tmp_path, feat)
    assert np.array_equal(got, speech) and got_last == last


def test_decision_loop_special_values(driver, tmp_path):
    """NaN and infinities where C++ float comparisons send them: hand-made features, no logarithm near a threshold."""
    inf, nan = np.inf, np.nan
    rows = [[100, 0, 1], [100, 1000, 20], [nan, 1000, 20], [100, nan, 20], [100, 1000, nan], [inf, 0, 0], [100, inf, inf], [0, 0, nan], [1e30, 62.5, 3]]
    for first in ([100, 0, 1], [0, 0, nan], [nan, nan, nan], [inf, 0, 1]):
        feat = np.array([first] + rows * 5, np.float32)
        speech, last, margin = V.decide(feat)
        assert margin > MARGIN_ULPS
        got, got_last = driver_decide(driver, tmp_path, feat)
        assert np.array_equal(got, speech) and got_last == last, first


def test_library_decide_is_the_drivers(driver, tmp_path, cases):
    """whisperc_debug_vad_decide (host only: no device) through ctypes gives what the driver prints."""
    from whisper_amd import api
    for name in NAMES:
        feat = cases[name][1]
        want, want_last = driver_decide(driver, tmp_path, feat)
        got, last = api.vad_decide(feat)
        assert np.array_equal(got, want) and last == want_last, name
    assert api.lib().whisperc_debug_vad_decide(None, -1, None, None) & 0xFFFFFFFF == 0x80070057
    assert api.lib().whisperc_debug_vad_decide(None, 3, None, None) & 0xFFFFFFFF == 0x80004003


# ---------------------------------------------------------------------------------------------------------------------
# the planner
# ---------------------------------------------------------------------------------------------------------------------
def flags_with_pauses(n_frames, pauses, seed=0):
    """speech everywhere but in the pauses [a, b); energies: seeded noise, low in the pauses"""
    speech = np.ones(n_frames, np.uint8)
    energy = np.random.default_rng(seed).uniform(500, 3000, n_frames).astype(np.float32)
    for a, b in pauses:
        speech[a:b] = 0
        energy[a:b] *= 0.01
    return speech, energy


def check_plan(chunks, N, max_len=V.MAX_LEN, min_len=V.MIN_LEN):
    """the properties the plan has by construction"""
    assert chunks[0][0] == 0 and sum(c for _, c in chunks) == N
    for (f0, c0), (f1, _) in zip(chunks, chunks[1:]):
        assert f0 + c0 == f1 and f1 % 256 == 0
    assert all(c <= max_len for _, c in chunks)
    assert all(c >= min_len for _, c in chunks[:-1])
    if N >= V.MIN_TAIL:
        assert chunks[-1][1] >= V.MIN_TAIL
    if N <= max_len:
        assert len(chunks) == 1


def test_planner_cases(driver, tmp_path):
    fr = lambda samples: samples // 256

    def both(speech, energy, N, **kw):
        rules = []
        want = V.plan(speech, energy, N, rules=rules, **kw)
        got = driver_plan(driver, tmp_path, speech, energy, N, **kw)
        assert got == want, (got, want)
        check_plan(got, N, kw.get("max_len") or V.MAX_LEN, kw.get("min_len") or V.MIN_LEN)
        return got, rules

    N = 16000 * 70
    # a pause that straddles start + maxLen: the cut is clipped to hi = 1875 and still lies inside the pause
    speech, energy = flags_with_pauses(fr(N), [(1860, 1900)])
    got, rules = both(speech, energy, N)
    assert got[0] == (0, 480000) and rules[0] == "pause" and 1860 < 480000 // 256 < 1900
    # several pauses in the window: the last one wins; one beyond hi does not count
    speech, energy = flags_with_pauses(fr(N), [(1000, 1030), (1400, 1440), (1700, 1730), (1880, 1960)])
    got, rules = both(speech, energy, N)
    assert got[0] == (0, 256 * 1715) and rules[0] == "pause"
    # a pause whose middle lies beyond hi but which begins before it: clipped to hi
    speech, energy = flags_with_pauses(fr(N), [(1400, 1440), (1870, 1960)])
    assert both(speech, energy, N)[0][0] == (0, 256 * 1875)
    # a pause only before lo = 938: the energy rule, and the quietest 21 frames win
    speech, energy = flags_with_pauses(fr(N), [(500, 560)])
    energy[1500:1521] = 1.0
    got, rules = both(speech, energy, N)
    assert rules[0] == "energy" and got[0] == (0, 256 * 1510)
    # the energy rule takes the FIRST minimum
    speech = np.ones(fr(N), np.uint8)
    energy = np.full(fr(N), 7.0, np.float32)
    got, rules = both(speech, energy, N)
    assert set(rules) == {"energy"} and len(rules) == len(got) - 1 and got[0] == (0, 256 * 938)
    # a pause shorter than pauseFrames is none; with pause_frames = 10 it is one
    speech, energy = flags_with_pauses(fr(N), [(1500, 1515)])
    assert both(speech, energy, N)[1][0] == "energy"
    assert both(speech, energy, N, pause_frames=10)[0][0] == (0, 256 * 1507)
    # other lengths: 10 s pieces of at least 4 s
    speech, energy = flags_with_pauses(fr(N), [(p, p + 25) for p in range(300, 4300, 400)])
    got, _ = both(speech, energy, N, max_len=160000, min_len=64000)
    assert len(got) >= 7
    # the tail rule: N = maxLen is one chunk; maxLen + 1 and maxLen + 15999 leave a last chunk of at least a second
    for n in (480000, 480001, 480000 + 15999, 480000 + 16000, 16000 * 45):
        speech, energy = flags_with_pauses(fr(n), [(1860, fr(n))])
        got, _ = both(speech, energy, n)
        assert len(got) == (1 if n == 480000 else 2)
    # short recordings: one chunk, N < 16000 and N = 0 included
    for n in (0, 100, 255, 256, 15999, 16000):
        assert both(np.ones(fr(n), np.uint8), np.ones(fr(n), np.float32), n)[0] == [(0, n)]
    # energies that are NaN: the longest chunk
    speech = np.ones(fr(N), np.uint8)
    assert both(speech, np.full(fr(N), np.nan, np.float32), N)[0][0] == (0, 480000)


def test_planner_refuses_bad_parameters(driver, tmp_path):
    N = 16000 * 40
    speech, energy = flags_with_pauses(N // 256, [(1000, 1030)])
    for kw in (dict(max_len=480001), dict(min_len=15999), dict(max_len=100000, min_len=68001), dict(min_len=448001), dict(pause_frames=-1),
               dict(max_len=-5), dict(max_len=40000, min_len=16000)):
        with pytest.raises(ValueError):
            V.plan(speech, energy, N, **kw)
        assert driver_plan(driver, tmp_path, speech, energy, N, **kw) == E_INVALIDARG, kw
    # the limits themselves are accepted
    assert driver_plan(driver, tmp_path, speech, energy, N, max_len=48000, min_len=16000) == V.plan(speech, energy, N, max_len=48000, min_len=16000)
    # flags that do not belong to N
    assert driver_plan(driver, tmp_path, speech[:-1], energy[:-1], N) == E_INVALIDARG


def test_planner_properties_on_random_flags(driver, tmp_path):
    """200 seeded random flag arrays: partition, lengths, alignment -- and the driver's plan is the restatement's."""
    rng = np.random.default_rng(2024)
    for i in range(200):
        N = int(rng.integers(0, 16000 * 150))
        n = N // 256
        # runs of speech and silence of random lengths, so that pauses of every size occur
        speech = np.zeros(n, np.uint8)
        pos, state = 0, int(rng.integers(0, 2))
        while pos < n:
            run = int(rng.integers(1, 60 if state == 0 else 700))
            speech[pos:pos + run] = state
            pos, state = pos + run, 1 - state
        energy = rng.uniform(0, 3000, n).astype(np.float32)
        kw = {} if i % 3 else dict(max_len=int(rng.integers(48000, 480001)), pause_frames=int(rng.integers(1, 40)))
        if kw:
            kw["min_len"] = int(rng.integers(16000, kw["max_len"] - 32000 + 1))
        want = V.plan(speech, energy, N, **kw)
        check_plan(want, N, kw.get("max_len", V.MAX_LEN), kw.get("min_len", V.MIN_LEN))
        assert driver_plan(driver, tmp_path, speech, energy, N, **kw) == want, (i, N, kw)


def test_composite_plan_cuts_inside_pauses(cases):
    """The restatement alone on the 63 s composite: both cuts come from the pause rule and lie inside gaps of the recording."""
    pcm = cases["composite"][0]
    _, feat, speech, _, _ = cases["composite"]
    rules = []
    chunks = V.plan(speech, feat[:, 0], len(pcm), rules=rules)
    print(chunks, rules)
    check_plan(chunks, len(pcm))
    assert rules == ["pause", "pause"]
    # inside a pause: a run of at least 21 non-speech frames around the cut (the clip pauses between phrases too: not every pause is a noise gap)
    for first, _ in chunks[1:]:
        c = first // 256
        a, b = c, c
        while a > 0 and not speech[a - 1]:
            a -= 1
        while b < len(speech) and not speech[b]:
            b += 1
        assert not speech[c] and b - a >= V.PAUSE_FRAMES and a < c < b, (first, a, b)


# ---------------------------------------------------------------------------------------------------------------------
# whisper-mgpu -split
# ---------------------------------------------------------------------------------------------------------------------
def test_mgpu_split_option():
    from whisper_amd import build
    if not os.path.exists(build.MGPU_BIN):
        build.build_all()
    run = lambda *a: subprocess.run([build.MGPU_BIN] + list(a), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    r = run("-m", "none.bin", "-f", "none.wav", "-split", "bogus")
    assert r.returncode == 1 and b"usage: whisper-mgpu" in r.stderr and b"fixed or silence" in r.stderr
    r = run("-m", "none.bin", "-f", "none.wav", "-split", "silence", "-per-recording")
    assert r.returncode == 1 and b"usage: whisper-mgpu" in r.stderr and b"-per-recording" in r.stderr
    r = run("-h")
    assert r.returncode == 1 and b"-split fixed|silence" in r.stderr
    # the option alone is not a complete call
    r = run("-split", "silence")
    assert r.returncode == 1 and b"-m and -f are required" in r.stderr
