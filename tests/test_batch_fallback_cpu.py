"""CPU tests of the decoding fallback in the lock-step batch scheduler (Whisper::setBatchDecodingFallback): whisper_amd/host/batchScheduler.cpp compiled
UNCHANGED next to the unchanged test double of the compute layer (tests/hostloop_cpu/fake_device.cpp) and tests/batch_fallback_cpu/driver.cpp, whose
injected sampling hooks record every ( slot, temperature, seed, nonce ) of every round and answer a scripted no-speech probability. The double decodes
greedily whatever the temperature, so a retried window reproduces its tokens: the scheduler is what is tested -- a retried window keeps its slot, its seek
and its prompt and costs one slot-round; the neighbours move on; a silent window leaves nothing behind; a failure in the middle of retries retires every
stream. The GPU twin: tests/test_gpu_batch_fallback.py."""
import ctypes as C
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import test_hostloop_cpu as H
from test_batch_cpu import StreamDesc, recordings
from whisper_amd import ggml_format as gf

ROOT = H.ROOT
LIB = os.path.join(H.BUILD, "libbatch_fallback_cpu.so")
STANDALONE = os.path.join(H.BUILD, "batch-fallback-sanitized")
HOST = os.path.join(ROOT, "whisper_amd", "host")
SOURCES = [os.path.join(ROOT, "tests", "batch_fallback_cpu", "driver.cpp")] + [os.path.join(HOST, f) for f in ("batchScheduler.cpp", "support.cpp", "tokenTimestamps.cpp")]
DEPS = SOURCES + [os.path.join(HOST, f) for f in os.listdir(HOST) if f.endswith(".h")] + [os.path.join(ROOT, "include", h) for h in ("whisperApi.h", "whisper_hip.h")] + \
       [os.path.join(ROOT, "tests", "hostloop_cpu", f) for f in ("fake_device.cpp", "batch_driver.cpp")]
INCLUDES = ["-I" + os.path.join(ROOT, "include"), "-I" + HOST]
E_NOTIMPL, E_FAIL = 0x80004001, 0x80004005
BASE_SEED = 1000
INC = 0.2
NEVER = dict(inc=INC, lpt=-1e30, et=-1.0, nth=2.0)          # gates nothing can fail
ALWAYS = dict(inc=INC, lpt=1e30, et=-1.0, nth=2.0)          # every attempt fails on its log-probability, nothing is silence


class RowRecord(C.Structure):
    _fields_ = [("round", C.c_int32), ("context", C.c_int32), ("slot", C.c_int32), ("temperature", C.c_float), ("seed", C.c_uint64), ("nonce", C.c_uint32),
                ("gather", C.c_int32)]


def _stale(target):
    return not os.path.exists(target) or any(os.path.getmtime(d) > os.path.getmtime(target) for d in DEPS + [os.path.join(H.REF_DIR, "libwhisper_ref.so")])


def _need_reference():
    if not os.path.exists(os.path.join(H.REF_DIR, "libwhisper_ref.so")):
        pytest.skip("oracle/_ref/libwhisper_ref.so not built")
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    os.makedirs(H.BUILD, exist_ok=True)


@pytest.fixture(scope="module")
def lib():
    _need_reference()
    if _stale(LIB):
        cmd = ["g++", "-std=c++17", "-O1", "-fPIC", "-shared"] + INCLUDES + SOURCES + \
              ["-o", LIB, "-L" + H.REF_DIR, "-lwhisper_ref", "-Wl,-rpath," + H.REF_DIR, "-Wl,-Bsymbolic", "-Wl,--no-undefined", "-lpthread"]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        assert r.returncode == 0, r.stdout
    L = C.CDLL(LIB)
    run_args = [C.c_char_p, C.c_int, C.c_uint32, C.c_uint32, C.c_int, C.POINTER(C.c_int32), C.c_int, C.POINTER(C.POINTER(C.c_float)), C.POINTER(C.c_int32),
                C.c_int, C.POINTER(StreamDesc), C.c_int, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int]
    L.bt_run.argtypes = run_args
    L.bf_run.argtypes = run_args + [C.c_int, C.c_float, C.c_float, C.c_float, C.c_float, C.c_uint64, C.c_int]
    L.bt_result.restype = C.c_char_p
    L.bf_result.restype = C.c_char_p
    L.bf_script_no_speech.argtypes = [C.c_int, C.POINTER(C.c_float), C.c_int, C.c_float]
    L.bf_rows.argtypes = [C.POINTER(RowRecord), C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.fake_device_counters.argtypes = [np.ctypeslib.ndpointer(dtype=np.int64, flags="C_CONTIGUOUS")]
    L.bf_install_hooks(1)
    return L


@pytest.fixture(scope="module")
def model_path(tmp_path_factory):
    model = gf.conditioned_model(gf.conditioned_layout(gf.hparams_for("test-d128-ml")), 4, kind="test-d128-ml", seed=10)
    path = str(tmp_path_factory.mktemp("bf") / "m.bin")
    gf.write_model(path, model)
    return path


def counters(L):
    v = np.zeros(6, np.int64)
    L.fake_device_counters(v)
    return v


def run(L, path, streams, slots, groups=1, chunk=4, lookahead=0, fallback=None, on=1, rules=0, flags=H.FLAG_NO_CONTEXT, n_max_text_ctx=0, offset_ms=0, plain=False):
    """bf_run (or the unchanged bt_run when plain): (hr, result, row records, no-speech reads, what the run's own device contexts counted)"""
    bufs = [np.ascontiguousarray(b, np.float32) for b in buffers()]
    ptrs = (C.POINTER(C.c_float) * len(bufs))(*[b.ctypes.data_as(C.POINTER(C.c_float)) for b in bufs])
    lens = (C.c_int32 * len(bufs))(*[len(b) for b in bufs])
    descs = (StreamDesc * len(streams))(*[StreamDesc(b, f, n) for (b, f, n) in streams])
    pt = (C.c_int32 * 1)(1000)
    common = (path.encode(), rules, flags, H.language_key("en"), n_max_text_ctx, C.cast(pt, C.POINTER(C.c_int32)), 1, ptrs, lens, len(bufs), descs, len(streams),
              slots, groups, chunk, lookahead, 4)
    before = counters(L)
    if plain:
        hr = L.bt_run(*common)
        return hr, json.loads(L.bt_result().decode()), [], 0, None
    f = fallback or NEVER
    hr = L.bf_run(*common, on if fallback is not None else 0, f["inc"], f["lpt"], f["et"], f["nth"], BASE_SEED, offset_ms)
    n, reads, off = C.c_int(), C.c_int(), C.c_int()
    L.bf_rows(None, 0, C.byref(n), C.byref(reads), C.byref(off))
    rows = (RowRecord * max(1, n.value))()
    L.bf_rows(rows, n.value, C.byref(n), None, None)
    recs = [dict(round=r.round, context=r.context, slot=r.slot, T=r.temperature, seed=r.seed, nonce=r.nonce, gather=r.gather) for r in rows[:n.value]]
    res = json.loads(L.bf_result().decode())
    return hr, res, recs, reads.value, np.asarray(res.get("counters", [0] * 6), np.int64) - before


def buffers():
    """test_batch_cpu's recordings, and a sixth of 61 s: several windows whatever the timestamps"""
    r = recordings()
    return r + [np.concatenate([r[4], r[1], r[0]]).astype(np.float32)]


def transcripts(res):
    return [(st["hr"], [(s["t0"], s["t1"], s["text"], s["tokens"]) for s in st["segments"]]) for st in res["streams"]]


STREAMS = [(0, 0, 0), (1, 0, 0), (2, 0, 0), (3, 0, 0), (4, 0, 0), (4, 16000 * 5, 16000 * 9)]


def check_rows(recs, res, n_streams):
    """What every round uploaded: idle slots greedy; a stream's rows carry seed + index, nonce = seek * 8 + k and T = k * inc formed in float; the attempts
    of a window are consecutive rounds of ONE context in ONE slot, k = 0, 1, 2 ...; the gather is on exactly when a slot of the round is at attempt 0."""
    by_window = {}
    for r in recs:
        if r["seed"] == 0:
            assert r["T"] == 0 and r["nonce"] == 0                                   # an idle slot
            continue
        stream, k, seek = r["seed"] - BASE_SEED, r["nonce"] & 7, r["nonce"] >> 3
        assert 0 <= stream < n_streams
        assert np.float32(r["T"]) == np.float32(k) * np.float32(INC), r
        by_window.setdefault((stream, seek), []).append(r)
    for rnd in {(r["context"], r["round"]) for r in recs}:
        rows = [r for r in recs if (r["context"], r["round"]) == rnd]
        assert {r["gather"] for r in rows} == {int(any(r["seed"] != 0 and r["nonce"] & 7 == 0 for r in rows))}, rows
    for (stream, seek), rows in by_window.items():
        # (a window the stop rules made the stream visit again starts over at k = 0: split the visits)
        visits = []
        for r in rows:
            if r["nonce"] & 7 == 0:
                visits.append([])
            visits[-1].append(r)
        for v in visits:
            assert [r["nonce"] & 7 for r in v] == list(range(len(v))), (stream, seek, v)
            assert len({(r["context"], r["slot"]) for r in v}) == 1, (stream, seek, v)      # the retrying stream keeps its slot
            ctx_rounds = sorted({r["round"] for r in recs if r["context"] == v[0]["context"]})
            at = ctx_rounds.index(v[0]["round"])
            assert [r["round"] for r in v] == ctx_rounds[at:at + len(v)], (stream, seek)     # one slot-round per attempt, back to back
        stats = [w for w in res["streams"][stream]["stats"] if w["seek"] == seek]
        assert [w["attempts"] for w in stats] == [len(v) for v in visits], (stream, seek, stats)
    return by_window


def test_feature_off_and_no_hooks(lib, model_path):
    """Never set, set and turned off again, or no hooks installed: the transcripts and device counters of the unchanged harness, no hook is called.
    Turning the feature on without hooks is E_NOTIMPL."""
    hr0, plain, _, _, _ = run(lib, model_path, STREAMS, 2, 2, plain=True)
    assert hr0 == 0 and sum(len(s["segments"]) for s in plain["streams"]) >= 6
    c0 = run(lib, model_path, STREAMS, 2, 2)[4]
    assert c0[2] >= 6 and c0[0] == 3                                                 # windows encoded; two groups and the loader
    for on in (0, 2):
        hr, res, recs, reads, c = run(lib, model_path, STREAMS, 2, 2, fallback=ALWAYS if on else None, on=on)
        assert hr == 0 and transcripts(res) == transcripts(plain) and recs == [] and reads == 0
        assert np.array_equal(c, c0) and all(st["stats"] == [] for st in res["streams"])
    lib.bf_install_hooks(0)
    try:
        hr, res, recs, _, c = run(lib, model_path, STREAMS, 2, 2)
        assert hr == 0 and transcripts(res) == transcripts(plain) and np.array_equal(c, c0)
        hr, res, recs, _, c = run(lib, model_path, STREAMS, 2, 2, fallback=ALWAYS)
        assert hr & 0xFFFFFFFF == E_NOTIMPL and res == {}
    finally:
        lib.bf_install_hooks(1)


@pytest.mark.parametrize("slots", [1, 2, 5])
def test_every_attempt_fails(lib, model_path, slots):
    """logprob_thold above every score, inc 0.2: six attempts per window at T = k * 0.2 formed in float, the last handed over -- the feature-off transcripts,
    six times the windows encoded; 5 slots for the 5 streams that run leave no slot idle, 1 and 2 slots refill."""
    hr0, off, _, _, c0 = run(lib, model_path, STREAMS, slots)
    hr, res, recs, reads, c = run(lib, model_path, STREAMS, slots, fallback=ALWAYS)
    assert hr0 == 0 and hr == 0 and transcripts(res) == transcripts(off)
    assert c0[2] > 0 and c[2] == 6 * c0[2] and c[3] == 6 * c0[3], (c0, c)           # windows encoded, window starts
    for st in res["streams"]:
        for w in st["stats"]:
            assert w["attempts"] == 6 and np.float32(w["temperature"]) == np.float32(5) * np.float32(INC) and not w["skipped"], w
    windows = check_rows(recs, res, len(STREAMS))
    assert len(windows) == sum(len({w["seek"] for w in st["stats"]}) for st in res["streams"]) >= 6
    assert reads == len({(r["context"], r["round"]) for r in recs if r["gather"]})
    if slots == 5:
        assert any(r["seed"] == 0 for r in recs)                                     # streams retire at different rounds: idle slots at T = 0
    print("slots %d: %d rounds, %d windows, %d encoded against %d" % (slots, len({(r["context"], r["round"]) for r in recs}), len(windows), c[2], c0[2]))


def test_a_retrying_stream_keeps_its_slot_while_neighbours_move_on(lib, model_path):
    """A threshold midway between two neighbouring greedy scores: the windows above it pass at once, those below take six rounds in their slots -- and
    meanwhile the neighbour's slot moves on to new windows and is refilled with the next stream. Transcripts: feature-off."""
    hr, res, _, _, _ = run(lib, model_path, STREAMS, 2, fallback=NEVER)
    assert hr == 0
    scores = sorted({w["avg_logprob"] for st in res["streams"] for w in st["stats"]})
    assert len(scores) >= 4 and all(w["attempts"] == 1 for st in res["streams"] for w in st["stats"])
    mid = len(scores) // 2
    thold = 0.5 * (scores[mid - 1] + scores[mid])
    hr0, off, _, _, c0 = run(lib, model_path, STREAMS, 2)
    hr, res, recs, _, c = run(lib, model_path, STREAMS, 2, fallback=dict(NEVER, lpt=thold))
    assert hr == 0 and transcripts(res) == transcripts(off)
    n_low = 0
    for st in res["streams"]:
        for w in st["stats"]:
            assert w["attempts"] == (6 if w["avg_logprob"] < thold else 1), w
            n_low += w["avg_logprob"] < thold
    assert 0 < n_low < sum(len(st["stats"]) for st in res["streams"])
    assert c[2] == c0[2] + 5 * n_low                                                 # one slot-round per retry
    check_rows(recs, res, len(STREAMS))
    # a round in which one slot is mid-retry while the other slot holds another stream than in the round before
    rounds = sorted({r["round"] for r in recs})
    at = {(r["round"], r["slot"]): r for r in recs}
    moved = 0
    for a, b in zip(rounds, rounds[1:]):
        for slot in (0, 1):
            mine, other, other_before = at[(b, slot)], at[(b, 1 - slot)], at[(a, 1 - slot)]
            moved += mine["nonce"] & 7 > 0 and other["seed"] != 0 and other["seed"] != other_before["seed"]
    print("refills next to a retrying stream:", moved)
    assert moved >= 1


def test_a_silent_window_is_skipped_and_leaves_nothing_behind(lib, model_path):
    """Carry-over on (every window's prompt holds its stream's past text), temperatureInc 0 (one attempt, handed over), the script calls the first window of
    stream 0 silent: it is skipped -- no segment from it -- and the stream goes on exactly as a run of the same recording that STARTS at the next window:
    nothing of the skipped window reached the next prompt. Stream 1, never silent, is untouched."""
    streams = [(5, 0, 0), (4, 0, 0)]
    kw = dict(rules=1, flags=0, n_max_text_ctx=16)
    gates = dict(inc=0.0, lpt=1e30, et=-1.0, nth=0.5)
    hr0, off, _, _, _ = run(lib, model_path, streams, 2, **kw)
    silent = (C.c_float * 1)(0.9)
    lib.bf_script_no_speech(0, silent, 1, 0.25)
    try:
        hr, res, recs, _, _ = run(lib, model_path, streams, 2, fallback=gates, **kw)
    finally:
        lib.bf_script_no_speech(0, None, 0, 0.0)
    assert hr0 == 0 and hr == 0
    st0, st1 = res["streams"]
    assert [w["skipped"] for w in st0["stats"]] == [1] + [0] * (len(st0["stats"]) - 1) and len(st0["stats"]) >= 2
    assert st0["stats"][0]["no_speech"] == pytest.approx(0.9) and all(w["no_speech"] == 0.25 for w in st0["stats"][1:] + st1["stats"])
    assert all(w["attempts"] == 1 and w["temperature"] == 0 for w in st0["stats"] + st1["stats"]) and all(r["T"] == 0 for r in recs)
    assert transcripts(res)[1] == transcripts(off)[1] and not any(w["skipped"] for w in st1["stats"])
    next_seek = st0["stats"][1]["seek"]
    assert st0["segments"] and all(s["t0"] >= next_seek * 100000 for s in st0["segments"])
    hr, later, _, _, _ = run(lib, model_path, streams[:1], 1, offset_ms=next_seek * 10, **kw)
    assert hr == 0 and transcripts(later)[0] == transcripts(res)[0]
    assert transcripts(res)[0] != transcripts(off)[0]                                # the first window did carry text


def test_a_failure_in_the_middle_of_retries_retires_every_stream(lib, model_path):
    """The upload of round 3 fails while both slots are at their third attempt: the run answers the failure, the streams in the slots end with E_FAIL and no
    result, the runner gives its device contexts back, and the next run is as good as ever."""
    before = counters(lib)[0]
    lib.bf_fail_upload_at_round(3)
    try:
        hr, res, recs, _, _ = run(lib, model_path, STREAMS, 2, fallback=ALWAYS)
    finally:
        lib.bf_fail_upload_at_round(-1)
    assert hr < 0 and res["hr"] == hr
    assert [st["hr"] & 0xFFFFFFFF for st in res["streams"][:2]] == [E_FAIL, E_FAIL] and all(st["segments"] == [] for st in res["streams"])
    assert {r["nonce"] & 7 for r in recs if r["round"] == 2} == {2} and max(r["round"] for r in recs) == 2
    assert counters(lib)[0] == before
    hr0, off, _, _, _ = run(lib, model_path, STREAMS, 2)
    hr, res, _, _, _ = run(lib, model_path, STREAMS, 2, fallback=ALWAYS)
    assert hr == 0 and transcripts(res) == transcripts(off)


def test_driver_under_sanitizers(lib, model_path, tmp_path):
    """The driver once more as a program of its own (its own main), host code only, built with -fsanitize=address,undefined: the scenarios above, no report."""
    _need_reference()
    if _stale(STANDALONE):
        cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-DBF_STANDALONE"] + INCLUDES + SOURCES + \
              ["-o", STANDALONE, "-L" + H.REF_DIR, "-lwhisper_ref", "-Wl,-rpath," + H.REF_DIR, "-lpthread"]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        assert r.returncode == 0, r.stdout
    pcm = recordings()[4][:16000 * 24]
    pcm_path = str(tmp_path / "pcm.f32")
    np.ascontiguousarray(pcm, "<f4").tofile(pcm_path)
    r = subprocess.run([STANDALONE, model_path, pcm_path], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    print(r.stdout[-3000:])
    assert r.returncode == 0 and "standalone ok" in r.stdout and "ERROR: AddressSanitizer" not in r.stdout and "runtime error" not in r.stdout, r.stdout[-4000:]
