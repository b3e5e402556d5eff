"""CPU tests of live capture at another rate than 16 kHz.

1. The index rule (tests/capture_rate_ref.py, the twin of the rule in include/whisper_hip.h at wh_capture_create_rate): which outputs of the stream appear on
   which append / flush / skip. Sample values are slices of resample_ref.resample over the stream with the skipped frames zeroed, so they are exact by
   construction; what is tested is that the spans tile the whole-buffer result, that an output appears exactly when its last tap has arrived, and that a
   filter which keeps nothing but the last K - 1 input frames -- the state the kernel keeps -- gives those values.
2. The host session (whisper_amd/host/capture.cpp) through a stand-alone driver, tests/capture_rate_cpu/driver.cpp, built with the address and
   undefined-behaviour sanitizers: capture.cpp as it ships over counting stubs of the six wh_capture_* entries a 16 kHz capture uses and a scripted table
   of the three a capture at another rate adds (captureRate.h).
The device half is tested in tests/test_gpu_capture_rate.py."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import capture_rate_ref as CR
import resample_ref as RR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = os.path.join(ROOT, "tests", "_build")
HOST = os.path.join(ROOT, "whisper_amd", "host")
RATES = [48000, 44100, 11025, 8000]
DESIGNS = {}


def design(rate):
    if rate not in DESIGNS:
        DESIGNS[rate] = RR.design(rate)
    return DESIGNS[rate]


def stream(rate):
    """3 K + 997 frames of float32 noise with a full-scale stretch"""
    K = design(rate)[3]
    rng = np.random.default_rng(rate)
    x = (0.3 * rng.standard_normal(3 * K + 997)).astype(np.float32)
    x[K:K + 50] = rng.choice(np.array([-1.0, 1.0], np.float32), 50)
    return x


def chunkings(rate, n):
    L, M, half, K, _ = design(rate)
    rng = np.random.default_rng(7)
    out = {"whole": [n], "ones": [1] * n}
    sizes = [half - 1, half, half + 1, K - 2, K - 1, K, K + 1, 1, 2 * K + 3]
    mix = []
    while sum(mix) < n:
        mix.append(int(rng.choice(sizes)))
    mix[-1] -= sum(mix) - n
    out["around_half_and_K"] = [c for c in mix if c > 0]
    for c in (half, K - 1, K, K + 1):
        out[str(c)] = [c] * (n // c) + ([n % c] if n % c else [])
    return out


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def history_filter(rate, x, ops):
    """The streaming filter with the state the kernel keeps and nothing else: the last K - 1 input frames and the three counters. An output is the float64 sum
    resample_ref.resample forms, over a window made of the history and the chunk only."""
    L, M, half, K, taps = design(rate)
    s = CR.Stream(L, M, half, K)
    hist = np.zeros(K - 1, np.float32)
    pos, outs = 0, []
    for op in ops:
        n_in0 = s.n_in
        if op == "flush":
            first, last = s.flush()
            window = np.concatenate([hist, np.zeros(half + 1, np.float32)])
        elif isinstance(op, tuple):
            s.skip(op[1])
            pos += op[1]
            hist = np.zeros(K - 1, np.float32)
            outs.append(None)
            continue
        else:
            chunk = x[pos:pos + op]
            pos += op
            first, last = s.append(op)
            window = np.concatenate([hist, chunk])
            hist = window[len(window) - (K - 1):].copy()
        n = np.arange(first, last, dtype=np.int64)
        base, ph = (n * M) // L, (n * M) % L
        # window[ 0 ] is stream frame n_in0 - ( K - 1 )
        idx = (base - half - (n_in0 - (K - 1)))[:, None] + np.arange(K)[None, :]
        assert len(n) == 0 or (idx.min() >= 0 and idx.max() < len(window)), "K - 1 frames of history are not enough"
        outs.append((window.astype(np.float64)[idx] * taps[ph].astype(np.float64)).sum(1).astype(np.float32) if len(n) else np.zeros(0, np.float32))
    return s, outs


@pytest.mark.parametrize("rate", RATES)
def test_any_chunking_plus_flush_is_the_whole_buffer(rate):
    L, M, half, K, taps = design(rate)
    x = stream(rate)
    whole = RR.resample(x, L, M, half, K, taps).astype(np.float32)
    assert len(whole) == RR.out_len(len(x), L, M)
    for name, chunks in chunkings(rate, len(x)).items():
        s, spans = CR.run((L, M, half, K), chunks + ["flush"])
        # the spans tile [0, out_len) in order
        assert spans[0][0] == 0 and all(a[1] == b[0] for a, b in zip(spans, spans[1:])) and spans[-1][1] == len(whole), name
        assert np.array_equal(bits(np.concatenate([whole[a:b] for a, b in spans])), bits(whole))
        # an output appears with the append that brings its last tap, frame base + half + 1, and not before
        n_in = 0
        for c, (a, b) in zip(chunks, spans):
            n_in += c
            assert b == 0 or (((b - 1) * M) // L + half + 1 <= n_in - 1), (name, n_in, b)
            assert (b * M) // L + half + 1 > n_in - 1, (name, n_in, b)
        # the state the kernel keeps is enough, and gives the same values
        _, outs = history_filter(rate, x, chunks + ["flush"])
        got = np.concatenate(outs)
        assert np.array_equal(bits(got), bits(whole)), (name, np.flatnonzero(bits(got) != bits(whole))[:5])


@pytest.mark.parametrize("rate", RATES)
def test_an_append_below_the_look_ahead_gives_nothing(rate):
    L, M, half, K, _ = design(rate)
    s = CR.Stream(L, M, half, K)
    assert s.append(half + 1) == (0, 0)             # the last tap of output 0 is frame half + 1
    assert s.append(1) == (0, CR.ceil_div(L, M))    # frame half + 1 has arrived: the outputs with base 0
    s = CR.Stream(L, M, half, K)
    for _ in range(half + 1):
        assert s.append(1) == (0, 0)
    # the look-ahead in time, as the documents state it
    ms = 1000.0 * (half + 1) / rate
    assert (2.1 <= ms < 2.25) if rate >= 22050 else (3.15 < ms < 3.25) if rate == 11025 else (4.3 < ms < 4.45)
    # a stream shorter than the look-ahead comes out whole with the flush
    s = CR.Stream(L, M, half, K)
    assert s.append(half) == (0, 0) and s.flush() == (0, RR.out_len(half, L, M))


@pytest.mark.parametrize("rate", RATES)
def test_skip_returns_the_clock_and_what_follows_is_the_zeroed_streams_tail(rate):
    L, M, half, K, taps = design(rate)
    x = stream(rate)
    n = len(x)
    for before, skipped, chunk in ((K + 5, 2 * half + 3, K - 1), (3, 1, 1), (half, half, half + 1), (2 * K, K + 100, 333), (0, 7, K)):
        s = CR.Stream(L, M, half, K)
        first = s.append(before)
        assert first == (0, s.ready(before))
        n_out = s.n_out
        grown = s.skip(skipped)
        z = before + skipped
        assert s.z == z and grown == CR.ceil_div(z * L, M) - n_out and s.n_out == CR.ceil_div(z * L, M)
        # a second skip right behind it moves the clock by exactly its own outputs
        ops = [before, ("skip", skipped)]
        rest = n - z
        ops += [chunk] * (rest // chunk) + ([rest % chunk] if rest % chunk else []) + ["flush"]
        tail = RR.resample(s.zeroed(x), L, M, half, K, taps).astype(np.float32)
        st, spans = CR.run((L, M, half, K), ops)
        assert spans[1] == (n_out, CR.ceil_div(z * L, M))
        assert spans[2][0] == CR.ceil_div(z * L, M) and spans[-1][1] == len(tail) == RR.out_len(n, L, M)
        _, outs = history_filter(rate, x, ops)
        got = np.concatenate([o for o in outs[2:]])
        want = tail[CR.ceil_div(z * L, M):]
        assert np.array_equal(bits(got), bits(want)), (before, skipped, chunk)
        # what came before the skip is the untouched stream's head
        head = RR.resample(x, L, M, half, K, taps).astype(np.float32)[:n_out]
        assert np.array_equal(bits(outs[0]), bits(head))
    # two skips in a row, and a skip of nothing
    s = CR.Stream(L, M, half, K)
    a, b = s.skip(10), s.skip(5)
    assert a + b == CR.ceil_div(15 * L, M) and s.skip(0) == 0 and s.z == 15


def test_the_twin_refuses_an_append_after_the_flush():
    s = CR.Stream(*design(48000)[:4])
    s.append(1000)
    s.flush()
    with pytest.raises(AssertionError):
        s.append(1)


# ---- 2. the host session ---------------------------------------------------------------------------------------------------------------------------------
DRIVER_SOURCES = [os.path.join(ROOT, "tests", "capture_rate_cpu", "driver.cpp"), os.path.join(HOST, "capture.cpp"), os.path.join(HOST, "support.cpp"),
                  os.path.join(ROOT, "tests", "hostloop_cpu", "fake_device.cpp")]


@pytest.fixture(scope="module")
def rows():
    ref_dir = os.path.join(ROOT, "oracle", "_ref")
    if not os.path.exists(os.path.join(ref_dir, "libwhisper_ref.so")):
        pytest.skip("oracle/_ref/libwhisper_ref.so not built: the CPU device double links against it")
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    os.makedirs(BUILD, exist_ok=True)
    exe = os.path.join(BUILD, "capture-rate-driver")
    deps = DRIVER_SOURCES + [os.path.join(HOST, h) for h in ("captureLoop.h", "captureRate.h", "vad.h", "hostCommon.h")] + [os.path.join(ROOT, "include", "whisperApi.h")]
    if not os.path.exists(exe) or any(os.path.getmtime(d) > os.path.getmtime(exe) for d in deps):
        r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I" + HOST, "-I" + os.path.join(ROOT, "include")] +
                           DRIVER_SOURCES + ["-o", exe, "-L" + ref_dir, "-lwhisper_ref", "-Wl,-rpath," + ref_dir, "-lpthread"], stdout=subprocess.PIPE,
                           stderr=subprocess.STDOUT, text=True)
        assert r.returncode == 0, r.stdout
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    return {ln.split("\t")[0]: ln.split("\t")[1:] for ln in r.stdout.splitlines()}


def ints(field):
    return [int(v) for v in field.split(",")] if field else []


S_OK, E_NOTIMPL, E_INVALIDARG = "0x00000000", "0x80004001", "0x80070057"


def test_a_16_khz_capture_never_calls_the_table(rows):
    """name, hr, old-entry calls "create,append,clear,take,size,destroy", table calls "create,flush,skip", pieces "start:count,...", appended frames"""
    for name in ("plain_16k", "at_rate_16000"):
        hr, old, table, pieces = rows[name][:4]
        assert hr == S_OK and ints(table) == [0, 0, 0], name
        create, append, clear, take, size, destroy = ints(old)
        # 40 chunks of 1600 frames of scripted speech: one create, one append per chunk, no size question, pieces at maxDuration and at the end
        assert (create, append, size, destroy) == (1, 40, 0, 1), name
        assert pieces == "0:48000,48000:16000", name


def test_at_48_khz_the_clock_advances_by_the_outputs_reported(rows):
    hr, old, table, pieces, appended = rows["rate_48k"][:5]
    assert hr == S_OK
    create, append, clear, take, size, destroy = ints(old)
    t_create, t_flush, t_skip = ints(table)
    # the object is made by the table's create, never by wh_capture_create; the end of the stream flushes exactly once
    assert (create, t_create, t_flush, t_skip) == (0, 1, 1, 0) and append == 40 and destroy == 1
    # the scripted device reports ( frames - 7 ) / 3 outputs for the first chunk, frames / 3 afterwards and 2 for the flush: 40 chunks of 4800 frames
    reported = [(4800 - 7) // 3] + [1600] * 39 + [2]
    assert ints(appended) == [4800] * 40
    total = sum(reported)
    # piece starts are sums of reported outputs: the first piece ends with the first read that brings the buffer to 48000 samples
    sums = np.cumsum(reported)
    first_end = int(sums[np.argmax(sums >= 48000)])
    assert pieces == "0:%d,%d:%d" % (first_end, first_end, total - first_end)


def test_a_discarded_read_calls_skip_and_uploads_nothing(rows):
    hr, old, table, pieces, appended, skipped = rows["stall_48k"][:6]
    assert hr == S_OK
    create, append, clear, take, size, destroy = ints(old)
    t_create, t_flush, t_skip = ints(table)
    assert 5 <= t_skip <= 16 and append + t_skip == 68 and len(ints(appended)) == append
    assert ints(skipped) == [480] * t_skip
    # the clock went on over the discarded reads: the scripted skip reports 480 / 3 + 1 outputs, and the piece behind the stall starts that much later
    spans = [tuple(int(v) for v in p.split(":")) for p in pieces.split(",")]
    assert len(spans) == 3 and spans[0][0] == 0 and spans[1][0] == spans[0][1]
    gap = spans[2][0] - (spans[1][0] + spans[1][1])
    assert gap == t_skip * 161, (spans, t_skip)
    # the end of the stream is the flush as one last read -- or, while stalled, a skip of nothing -- exactly once
    assert t_flush + ints(rows["stall_48k"][6])[0] == 1


def test_without_a_table_another_rate_is_not_implemented(rows):
    hr, old, table, pieces = rows["no_table"][:4]
    assert hr == E_NOTIMPL and ints(old) == [0] * 6 and pieces == ""
    assert "sample rate" in rows["no_table"][-1]


def test_rates_out_of_range_are_refused(rows):
    assert rows["create_999"][0] == E_INVALIDARG and rows["create_384001"][0] == E_INVALIDARG
    assert rows["create_1000"][0] == S_OK and rows["create_384000"][0] == S_OK


# ---- the faces ---------------------------------------------------------------------------------------------------------------------------------------------
def test_declarations_and_exports():
    from whisper_amd import api, binding, build
    if not os.path.exists(api.HOST_LIB_PATH):
        build.build_all()
    out = subprocess.run(["nm", "-D", "--defined-only", "-C", api.HOST_LIB_PATH], stdout=subprocess.PIPE, text=True, check=True).stdout
    assert "Whisper::createPcmCaptureAtRate(" in out and "Whisper::createPcmCapture(" in out
    header = open(os.path.join(ROOT, "include", "whisper_c.h")).read()
    lib = ctypes.CDLL(api.HOST_LIB_PATH)
    assert re.search(r"\bwhisperc_capture_create_rate\s*\(", header) and hasattr(lib, "whisperc_capture_create_rate")
    hip = open(os.path.join(ROOT, "include", "whisper_hip.h")).read()
    dev = subprocess.run(["nm", "-D", "--defined-only", binding.LIB_PATH], stdout=subprocess.PIPE, text=True, check=True).stdout
    for name in ("wh_capture_create_rate", "wh_capture_flush", "wh_capture_skip", "wh_op_capture_append_rate"):
        assert re.search(r"\b%s\s*\(" % name, hip) and (" T " + name) in dev and name in binding.EXPORTS, name
    # capture.cpp reaches the new entries through the table only: the refusal driver of tests/test_capture_cpu.py links it against six stubs
    text = open(os.path.join(HOST, "capture.cpp")).read()
    assert not re.search(r"\bwh_capture_(create_rate|flush|skip)\b", text)


def test_capture_object_at_a_rate_needs_no_device():
    from whisper_amd import api, build
    if not os.path.exists(api.HOST_LIB_PATH):
        build.build_all()
    for bad in (999, 384001, 0, -16000):
        with pytest.raises(api.WhisperError) as e:
            api.Capture(sample_rate=bad)
        assert e.value.hr == 0x80070057
    # writes are split at one second of INPUT, and without NoDrop the queue holds maxDuration + 1 s of input frames: 4 s of 48 kHz = 192000
    cap = api.Capture(sample_rate=48000)
    for _ in range(60):
        cap.write(np.zeros(4800, np.int16))
    assert cap.dropped_chunks() == 60 - (192000 // 4800 + 1)
    cap.release()
    cap = api.Capture(sample_rate=8000)
    # 4 s of 8 kHz = 32000 frames; a write of 2.5 s is queued as 8000 + 8000 + 4000
    cap.write(np.zeros(20000, np.float32))
    cap.write(np.zeros(8000, np.float32))
    cap.write(np.zeros(8000, np.float32))           # 28000 were queued, not more than the limit: 36000 now
    assert cap.dropped_chunks() == 0
    cap.write(np.zeros(8000, np.float32))           # the oldest chunk, a second, goes
    assert cap.dropped_chunks() == 1
    cap.release()


def test_cli_parses_the_capture_rate():
    import json
    from whisper_amd import build
    if not os.path.exists(build.CLI_BIN):
        build.build_all()
    run = lambda *a: subprocess.run([build.CLI_BIN] + list(a), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=30)
    r = run("--dump-options", "--capture", "-", "--capture-rate", "48000")
    assert r.returncode == 0
    second = json.loads(r.stdout.decode().splitlines()[1])
    assert second["rate"] == 48000 and second["capture"] == "-" and list(second)[-1] == "rate"
    # the line is what it was when the option is not given
    assert "rate" not in json.loads(run("--dump-options", "--capture", "-").stdout.decode().splitlines()[1])
    for bad in (["--capture", "-", "--capture-rate", "999"], ["--capture", "-", "--capture-rate", "384001"], ["--capture", "-", "--capture-rate"],
                ["--capture", "-", "--capture-rate", "abc"]):
        r = run(*bad)
        assert r.returncode == 2 and b"error:" in r.stderr, bad
    assert b"capture" not in run("-h").stderr
