"""CPU tests of the decoding fallback: the Python restatement of Philox4x32-10 against the published vectors, the statistics of the restatement's draws, and
the host rules of whisper_amd/host/decodeFallback.h -- temperature schedule, scores, gates and the plan's paths -- through a stand-alone driver, built plain
and with the address and undefined-behaviour sanitizers, against the restatement of tests/fallback_ref.py. The kernels are tested in tests/test_gpu_fallback.py."""
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

import fallback_ref as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = os.path.join(ROOT, "tests", "_build")
INF = float("inf")


def test_philox_published_vectors():
    """The known-answer vectors of the Random123 distribution (kat_vectors, philox4x32 10 rounds)."""
    vec = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
           ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
           ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]
    for counter, key, want in vec:
        assert F.philox4x32_10(counter, key) == want, (counter, key)
    # the uniform number takes the first two words: 53 bits, below 1
    x = F.philox4x32_10((5, 2, 9, 0), (0x89abcdef, 0x01234567))
    u = F.uniform(0x0123456789abcdef, 9, 5, 2)
    assert u == ((x[0] << 21) | (x[1] >> 11)) / 2.0 ** 53 and 0.0 <= u < 1.0


def test_draws_follow_the_row():
    """Chi-square of the restatement's draws on the 4-token row (0.5, 0.25, 0.125, 0.125) over 4096 positions: 3 degrees of freedom, 16.27 is the 0.1 % point."""
    p = np.zeros(8, np.float32)
    p[:4] = (0.5, 0.25, 0.125, 0.125)
    counts = np.zeros(4)
    for pos in range(4096):
        tok, _ = F.draw(p, 7, 4, 5, 6, 0, 0, F.uniform(1234, 7, pos, 0))
        counts[tok] += 1
    expect = 4096 * p[:4].astype(np.float64)
    chi2 = float(((counts - expect) ** 2 / expect).sum())
    print("counts", counts, "chi2 %.3f" % chi2)
    assert counts.sum() == 4096 and chi2 < 16.27


def test_draw_rules_of_the_restatement():
    """The branches of the draw on rows small enough to work out by hand."""
    beg, sot, solm, tnot = 7, 4, 5, 6
    p = np.array([0.1, 0.2, 0.0, 0.1, 0.3, 0.1, 0.1, 0.05, 0.05], np.float32)      # text 0 .. 3, specials 4 .. 6 (0.5 of the mass), timestamps 7, 8
    # the specials are never drawn, whatever u
    toks = {F.draw(p, beg, sot, solm, tnot, 0, 0, u)[0] for u in np.linspace(0, 0.999999, 97)}
    assert toks == {0, 1, 3, 7, 8}
    # forced timestamps: the timestamps only; u = 0 takes the first one with mass
    assert {F.draw(p, beg, sot, solm, tnot, 1, 0, u)[0] for u in (0.0, 0.49, 0.51, 0.99)} == {7, 8}
    # the sum rule: timestamps outweigh the best text token
    q = np.array([0.1, 0.1, 0, 0, 0, 0, 0, 0.4, 0.4], np.float32)
    assert F.draw(q, beg, sot, solm, tnot, 0, 0, 0.3)[0] == 7 and F.draw(q, beg, sot, solm, tnot, 0, 0, 0.7)[0] == 8
    # one allowed token with mass, and none at all
    one = np.zeros(9, np.float32)
    one[3] = 0.25
    one[5] = 0.75
    assert all(F.draw(one, beg, sot, solm, tnot, 0, 0, u)[0] == 3 for u in (0.0, 0.5, 1.0 - 2.0 ** -53))
    assert F.draw(np.zeros(9, np.float32), beg, sot, solm, tnot, 0, 0, 0.5)[0] is None


# ---------------------------------------------------------------------------------------------------------------------
# decodeFallback.h through its driver
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=["plain", "sanitized"])
def driver(request):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    os.makedirs(BUILD, exist_ok=True)
    exe = os.path.join(BUILD, "fallback-driver-" + request.param)
    src = os.path.join(ROOT, "tests", "fallback_cpu", "driver.cpp")
    host = os.path.join(ROOT, "whisper_amd", "host")
    deps = [src, os.path.join(host, "decodeFallback.h"), os.path.join(ROOT, "include", "whisperApi.h")]
    if not os.path.exists(exe) or any(os.path.getmtime(d) > os.path.getmtime(exe) for d in deps):
        flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if request.param == "sanitized" else ["-O2"]
        r = subprocess.run(["g++", "-std=c++17", "-Wall"] + flags + ["-I" + host, "-I" + os.path.join(ROOT, "include"), src, "-o", exe],
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        assert r.returncode == 0, r.stdout
    return exe


def run_driver(exe, *args):
    r = subprocess.run([exe] + [str(a) for a in args], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    return r.stdout.splitlines()


def fmt(prm):
    return "%.9g %.9g %.9g %.9g %d" % (prm["inc"], prm["lpt"], prm["et"], prm["nth"], prm["seed"])


def test_header_names_no_device_symbol():
    text = open(os.path.join(ROOT, "whisper_amd", "host", "decodeFallback.h")).read()
    code = "\n".join(ln.split("//")[0] for ln in text.splitlines())
    assert "wh_" not in code and "whisper_hip.h" not in text


@pytest.mark.parametrize("inc", [0.2, 0.4, 0.3, 0.0, -1.0])
def test_schedule(driver, inc):
    want = F.schedule(inc)
    got = [np.float32(v) for v in run_driver(driver, "schedule", inc)[0].split()]
    assert got == want
    assert len(want) == {0.2: 6, 0.4: 3, 0.3: 4, 0.0: 1, -1.0: 1}[inc] and want[0] == 0


def token_lists():
    rng = np.random.default_rng(11)
    distinct = lambda n: [(100 + i, float(rng.uniform(0.2, 0.9))) for i in range(n)]
    cases = {
        "32 distinct": (distinct(32), 32, 0),
        "33 distinct": (distinct(33), 33, 0),
        "33 with one id repeated": ([(7, 0.9)] * 33, 33, 0),
        "32 with one id repeated": ([(7, 0.9)] * 32, 32, 0),
        "40 whose last 32 hold 3 ids": (distinct(8) + [(i % 3, 0.8) for i in range(32)], 40, 0),
        "p = 0 and a denormal": ([(1, 0.0), (2, 1e-45), (3, 0.5)], 3, 0),
        "resultLen = 0": (distinct(5), 0, 0),
        "resultLen below the list's length": (distinct(20), 11, 0),
        "a failed scan": (distinct(10), 10, 1),
        "low probabilities": ([(i, 0.05) for i in range(12)], 12, 0),
    }
    return cases


@pytest.mark.parametrize("name", sorted(token_lists()))
def test_scores_and_verdicts(driver, tmp_path, name):
    tokens, result_len, scan_failed = token_lists()[name]
    for prm, no_speech in ((F.DEFAULTS, 0.1), (F.DEFAULTS, 0.9), (dict(F.DEFAULTS, lpt=-INF, et=-INF), 0.9), (dict(F.DEFAULTS, lpt=INF, nth=2.0), 0.9),
                           (dict(F.DEFAULTS, lpt=INF, nth=-1.0), 0.0)):
        path = str(tmp_path / "case.txt")
        with open(path, "w") as f:
            f.write("%s\n%d %.9g %d %d\n" % (fmt(prm), scan_failed, no_speech, result_len, len(tokens)))
            f.write("".join("%d %.9g\n" % (i, np.float32(p)) for i, p in tokens))
        avg, ent, failed, silent = run_driver(driver, "verdict", path)[0].split()
        w_avg, w_ent = F.score(tokens, result_len)
        assert math.isclose(float(avg), w_avg, rel_tol=1e-13, abs_tol=1e-300) and math.isclose(float(ent), w_ent, rel_tol=1e-13, abs_tol=1e-15), (avg, w_avg, ent, w_ent)
        assert int(failed) == F.attempt_failed(prm, scan_failed, result_len, w_avg, w_ent), (name, prm)
        assert int(silent) == F.attempt_silent(prm, scan_failed, w_avg, no_speech), (name, prm)
    # what the cases are there for, under the defaults
    w_avg, w_ent = F.score(tokens, result_len)
    failed = F.attempt_failed(F.DEFAULTS, scan_failed, result_len, w_avg, w_ent)
    if name == "32 distinct" or name == "33 distinct":
        assert math.isclose(w_ent, math.log(32)) and not failed
    if name == "33 with one id repeated":
        assert w_ent == 0 and failed
    if name == "32 with one id repeated":
        assert w_ent == 0 and not failed                      # the entropy judges more than 32 tokens only
    if name == "40 whose last 32 hold 3 ids":
        assert w_ent < 2.4 and failed
    if name == "p = 0 and a denormal":
        assert math.isclose(w_avg, (2 * math.log(F.FLT_MIN) + math.log(0.5)) / 3) and failed
    if name in ("resultLen = 0", "a failed scan", "low probabilities"):
        assert failed


def test_plan_paths(driver, tmp_path):
    good, bad, silent_bad = (0, 10, -0.3, 3.0, 0.1), (0, 10, -2.0, 3.0, 0.1), (0, 10, -2.0, 3.0, 0.9)
    scan_failed, scan_failed_silent, empty, looping = (1, 0, 0.0, 0.0, 0.1), (1, 5, -2.0, 1.0, 0.99), (0, 0, 0.0, 0.0, 0.1), (0, 40, -0.2, 1.0, 0.1)
    cases = [
        (F.DEFAULTS, 300, [good]),                                           # accepted at once
        (F.DEFAULTS, 300, [bad, looping, good]),                             # two retries, then accepted
        (F.DEFAULTS, 0, [bad] * 6),                                          # exhaustion: handed over at temperature 1.0
        (F.DEFAULTS, 2999, [bad, bad, silent_bad]),                          # silence wins on a later attempt
        (F.DEFAULTS, 100, [silent_bad]),                                     # ... and on the first
        (F.DEFAULTS, 100, [scan_failed_silent, good]),                       # a failed scan is never silence: it is retried
        (F.DEFAULTS, 100, [scan_failed] * 6),                                # ... and handed over failed
        (F.DEFAULTS, 100, [empty, good]),
        (dict(F.DEFAULTS, inc=0.0), 700, [bad]),                             # no temperatures: handed over right away
        (dict(F.DEFAULTS, inc=-1.0), 700, [good]),
        (dict(F.DEFAULTS, inc=0.4), 700, [bad] * 3),
        (dict(F.DEFAULTS, lpt=-INF, et=-INF), 5, [bad]),                     # gates off: everything that has tokens passes
        (dict(F.DEFAULTS, lpt=INF, nth=2.0), 5, [good] * 6),                 # every attempt fails, nothing is silent
        (dict(F.DEFAULTS, lpt=INF, nth=-1.0), 5, [good]),                    # everything is silent
        (F.DEFAULTS, 2 ** 29 + 3, [bad, good]),                              # the nonce wraps in 32 bits
    ]
    seen = set()
    for prm, seek, attempts in cases:
        path = str(tmp_path / "plan.txt")
        with open(path, "w") as f:
            f.write("%s %d\n" % (fmt(prm), seek))
            f.write("".join("%d %d %.17g %.17g %.9g\n" % a for a in attempts))
        got = [ln.split() for ln in run_driver(driver, "plan", path)]
        got = [(int(a), float(np.float32(b)), int(c), int(d), int(e)) for a, b, c, d, e in got]
        want = F.plan(prm, seek, attempts)
        assert got == [(a, float(np.float32(b)), c, d, e) for a, b, c, d, e in want], (prm, seek, attempts)
        seen.add(want[-1][-1])
        assert [w[2] for w in want] == [(seek * 8 + i) % 2 ** 32 for i in range(len(want))]
    assert seen == {F.ACCEPT, F.SKIP, F.HAND_OVER}
    assert F.plan(F.DEFAULTS, 0, [bad] * 6)[-1][:2] == (5, 1.0)


def test_draw_cases_of_the_gpu_test_stay_clear_of_the_boundaries():
    """The rows, seed and nonce tests/test_gpu_fallback.py draws with: in the restatement no draw lies within 1e-10 W of a prefix boundary (where another
    summation order could choose the neighbouring token), so the GPU test leaves none out; and every branch occurs."""
    from types import SimpleNamespace
    from whisper_amd import ggml_format as gf
    closest, none_allowed, n = 1.0, 0, 0
    for V in (51865, 51866):
        sp = gf.special_tokens(SimpleNamespace(n_vocab=V))
        for kinds, probs, positions in F.draw_batches(V, sp):
            u = F.uniforms(F.DRAW_SEED, F.DRAW_NONCE, positions)
            for force in (0, 1):
                for initial in (0, 1):
                    for r, kind in enumerate(kinds):
                        tok, margin = F.draw(probs[r], sp["beg"], sp["sot"], sp["solm"], sp["not_"], force, initial, u[r])
                        n += 1
                        if tok is None:
                            none_allowed += 1
                            assert kind in ("only_specials", "zero", "one_allowed", "specials", "softmax") and (kind in ("only_specials", "zero") or force or initial)
                            continue
                        closest = min(closest, margin)
                        assert tok not in (sp["sot"], sp["solm"], sp["not_"]) and probs[r][tok] > 0
                        ts_end, _, _, only_ts = F.sample_best_stats(probs[r], V, sp["beg"], force, initial)
                        assert tok < ts_end and (tok >= sp["beg"] or not only_ts)
                        if kind == "ts_above" and not initial:
                            assert only_ts
                        if kind == "softmax" and not force:
                            assert not only_ts
    print("%d draws, %d without an allowed token, closest approach to a boundary %.3e W" % (n, none_allowed, closest))
    assert closest > 1e-10 and none_allowed > 0


def test_whisper_main_takes_the_options_without_showing_them():
    """--fallback, -tpi, -lpt, -et, -nth are parsed out before the reference's parser sees the line: --dump-options and the usage text stay the reference's."""
    from whisper_amd import build
    if not os.path.exists(build.CLI_BIN):
        build.build_all()
    run = lambda *a: subprocess.run([build.CLI_BIN] + list(a), stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=60)
    plain = run("--dump-options", "-f", "a.wav")
    with_them = run("--dump-options", "--fallback", "-tpi", "0.4", "-f", "a.wav", "-lpt", "-0.5", "-et", "2.0", "-nth", "0.3")
    assert plain.returncode == 0 and with_them.returncode == 0 and with_them.stdout == plain.stdout and "a.wav" in plain.stdout
    usage = run("-h")
    for name in ("--fallback", "-tpi", "-lpt", "-nth"):
        assert name not in usage.stdout + usage.stderr
    r = run("-f", "a.wav", "-tpi")
    assert r.returncode == 2 and "-tpi needs a number" in r.stderr
