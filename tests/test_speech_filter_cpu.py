"""CPU tests of the speech filter above its rules (those are tests/test_speech_spans_cpu.py's):

  * the lock-step scheduler: whisper_amd/host/batchScheduler.cpp compiled UNCHANGED next to the unchanged test double of the compute layer and
    tests/speech_filter_cpu/batch_driver.cpp, whose injected packer (batchSpeech.h) is a host copy with a detector of its own (a frame is speech when a sample
    exceeds 0.005 in magnitude). Every stream must be transcribed from ITS packed samples and report ITS mapped times: the transcript of the packed samples run
    as a recording of their own through the unchanged harness, the times through the restatement's map, then the stream's offset in its buffer;
  * argument checks of the flat C layer that need no device, and the tools' option parsing.
The GPU twin: tests/test_gpu_speech_filter.py."""
import ctypes as C
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import speech_spans_ref as S
import test_hostloop_cpu as H
from test_batch_cpu import StreamDesc, recordings
from whisper_amd import ggml_format as gf

ROOT = H.ROOT
HOST = os.path.join(ROOT, "whisper_amd", "host")
LIB = os.path.join(H.BUILD, "libspeech_filter_cpu.so")
SOURCES = [os.path.join(ROOT, "tests", "speech_filter_cpu", "batch_driver.cpp")] + [os.path.join(HOST, f) for f in ("batchScheduler.cpp", "support.cpp", "tokenTimestamps.cpp")]
DEPS = SOURCES + [os.path.join(HOST, f) for f in os.listdir(HOST) if f.endswith(".h")] + [os.path.join(ROOT, "include", h) for h in ("whisperApi.h", "whisper_hip.h")] + \
       [os.path.join(ROOT, "tests", "hostloop_cpu", f) for f in ("fake_device.cpp", "batch_driver.cpp")]
INCLUDES = ["-I" + os.path.join(ROOT, "include"), "-I" + HOST]
E_POINTER, E_INVALIDARG, E_NOTIMPL = 0x80004003, 0x80070057, 0x80004001
THRESHOLD = np.float32(0.005)
PARAMS = (60, 8, 10)            # frames: min silence 0.96 s, min speech 0.128 s, pad 0.16 s
R16 = 16000


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(os.path.join(H.REF_DIR, "libwhisper_ref.so")):
        pytest.skip("oracle/_ref/libwhisper_ref.so not built")
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    os.makedirs(H.BUILD, exist_ok=True)
    if not os.path.exists(LIB) or any(os.path.getmtime(d) > os.path.getmtime(LIB) for d in DEPS + [os.path.join(H.REF_DIR, "libwhisper_ref.so")]):
        cmd = ["g++", "-std=c++17", "-O1", "-fPIC", "-shared"] + INCLUDES + SOURCES + \
              ["-o", LIB, "-L" + H.REF_DIR, "-lwhisper_ref", "-Wl,-rpath," + H.REF_DIR, "-Wl,-Bsymbolic", "-Wl,--no-undefined", "-lpthread"]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        assert r.returncode == 0, r.stdout
    L = C.CDLL(LIB)
    run_args = [C.c_char_p, C.c_int, C.c_uint32, C.c_uint32, C.c_int, C.POINTER(C.c_int32), C.c_int, C.POINTER(C.POINTER(C.c_float)), C.POINTER(C.c_int32),
                C.c_int, C.POINTER(StreamDesc), C.c_int, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int]
    L.bt_run.argtypes = run_args
    L.sf_run.argtypes = run_args + [C.c_int] * 4
    L.bt_result.restype = C.c_char_p
    L.sf_result.restype = C.c_char_p
    L.sf_install_hook(1)
    return L


@pytest.fixture(scope="module")
def model_path(tmp_path_factory):
    model = gf.conditioned_model(gf.conditioned_layout(gf.hparams_for("test-d128-ml")), 4, kind="test-d128-ml", seed=10)
    path = str(tmp_path_factory.mktemp("speech") / "m.bin")
    gf.write_model(path, model)
    return path


def buffers():
    """recordings with stretches of exact silence: in front, in the middle, behind; one that is silence only; one without any (a single span: not packed)"""
    jfk, two, quiet, _, three = recordings()
    z = lambda seconds: np.zeros(int(seconds * R16), np.float32)
    return [np.concatenate([z(3.0), jfk, z(4.0), two[:12 * R16], z(2.5)]),
            z(5.0),
            np.concatenate([three[:20 * R16], z(3.2), jfk[:6 * R16 + 77]]),
            jfk[R16:9 * R16].copy()]


STREAMS = [(0, 0, 0), (1, 0, 0), (2, 0, 0), (0, 2 * R16, 24 * R16), (3, 0, 0), (2, 21 * R16, 0)]


def piece(bufs, desc):
    b, first, count = desc
    return bufs[b][first:first + count] if count else bufs[b][first:]


def spans_of(pcm):
    n = len(pcm) // 256
    flags = (np.abs(pcm[:n * 256].reshape(n, 256)).max(1) > THRESHOLD).astype(np.uint8) if n else np.zeros(0, np.uint8)
    return S.spans(flags, len(pcm), *PARAMS)


def call(L, fn, path, bufs, streams, slots, groups, extra=()):
    bufs = [np.ascontiguousarray(b, np.float32) for b in bufs]
    ptrs = (C.POINTER(C.c_float) * len(bufs))(*[b.ctypes.data_as(C.POINTER(C.c_float)) for b in bufs])
    lens = (C.c_int32 * len(bufs))(*[len(b) for b in bufs])
    descs = (StreamDesc * len(streams))(*[StreamDesc(b, f, n) for (b, f, n) in streams])
    pt = (C.c_int32 * 1)(1000)
    hr = fn(path.encode(), 0, H.FLAG_NO_CONTEXT, H.language_key("en"), 0, C.cast(pt, C.POINTER(C.c_int32)), 1, ptrs, lens, len(bufs), descs, len(streams),
            slots, groups, 4, 0, 4, *extra)
    return hr, json.loads((L.bt_result if fn is L.bt_run else L.sf_result)().decode())


def transcripts(res):
    return [(st["hr"], [(s["t0"], s["t1"], s["text"], s["tokens"]) for s in st["segments"]]) for st in res["streams"]]


@pytest.fixture(scope="module")
def expected(lib, model_path):
    """Per stream: its spans, and the transcript of its packed samples run as a recording of its own by the unchanged harness, with the times mapped by the
    restatement and the stream's offset added afterwards. A stream without speech: hr 0 and nothing."""
    bufs = buffers()
    spans = [spans_of(piece(bufs, d)) for d in STREAMS]
    packed = [S.pack(piece(bufs, d), sp) for d, sp in zip(STREAMS, spans)]
    live = [i for i, p in enumerate(packed) if len(p)]
    hr, res = call(lib, lib.bt_run, model_path, [packed[i] for i in live], [(k, 0, 0) for k in range(len(live))], 2, 1)
    assert hr == 0
    want = [(0, []) for _ in STREAMS]
    for k, i in enumerate(live):
        shift = STREAMS[i][1] * 625
        st = res["streams"][k]
        want[i] = (st["hr"], [(S.start_ticks(spans[i], s["t0"]) + shift, S.end_ticks(spans[i], s["t1"]) + shift, s["text"], s["tokens"]) for s in st["segments"]])
    return bufs, spans, want


def test_the_cases_are_what_they_should_be(expected):
    bufs, spans, want = expected
    assert [len(s) for s in spans] == [2, 0, 2, 2, 1, 1]
    assert spans[4] == [(0, len(bufs[3]))]                                       # one span that covers the recording
    assert spans[2][-1][1] == len(bufs[2]) and len(bufs[2]) % 256 != 0            # the last span takes the partial frame
    assert spans[3] != spans[0]                                                   # the piece has its own spans
    assert sum(len(w[1]) for w in want) >= 8 and want[1] == (0, [])
    # a mapped time lies behind its packed time wherever silence was removed in front of it
    assert want[0][1][0][0] >= spans[0][0][0] * 625 > 0


@pytest.mark.parametrize("slots,groups", [(1, 1), (2, 1), (3, 2), (8, 1)])
def test_every_stream_gets_its_own_spans_and_its_own_map(lib, model_path, expected, slots, groups):
    bufs, spans, want = expected
    hr, res = call(lib, lib.sf_run, model_path, bufs, STREAMS, slots, groups, (1,) + PARAMS)
    assert hr == 0
    assert transcripts(res) == want
    assert [[tuple(s) for s in st["spans"]] for st in res["streams"]] == spans
    assert all(st["result"] == 1 for st in res["streams"])                       # the silent stream too: an empty result, S_OK
    assert res["packer_calls"] == len(STREAMS)


def test_off_is_the_unchanged_scheduler_and_no_packer_is_not_implemented(lib, model_path, expected):
    bufs, _, want = expected
    hr0, plain = call(lib, lib.bt_run, model_path, bufs, STREAMS, 2, 2)
    assert hr0 == 0 and transcripts(plain) != want
    for mode in (0, 2):
        hr, res = call(lib, lib.sf_run, model_path, bufs, STREAMS, 2, 2, (mode,) + PARAMS)
        assert hr == 0 and transcripts(res) == transcripts(plain) and res["packer_calls"] == 0
        assert all(st["spans"] == [] for st in res["streams"])
    # the argument check comes first, then the missing packer
    for bad in ((-1, 0, 0), (0, (1 << 20) + 1, 0), (0, 0, -5)):
        hr, res = call(lib, lib.sf_run, model_path, bufs, STREAMS, 2, 2, (1,) + bad)
        assert hr & 0xFFFFFFFF == E_INVALIDARG and res == {}
    lib.sf_install_hook(0)
    try:
        hr, res = call(lib, lib.sf_run, model_path, bufs, STREAMS, 2, 2, (1,) + PARAMS)
        assert hr & 0xFFFFFFFF == E_NOTIMPL and res == {}
        hr, res = call(lib, lib.sf_run, model_path, bufs, STREAMS, 2, 2, (1, -1, 0, 0))
        assert hr & 0xFFFFFFFF == E_INVALIDARG
        hr, res = call(lib, lib.sf_run, model_path, bufs, STREAMS, 2, 2, (0,) + PARAMS)
        assert hr == 0 and transcripts(res) == transcripts(plain)
    finally:
        lib.sf_install_hook(1)


def test_the_refusals_fail_their_stream_alone(lib, model_path, expected):
    """TokenTimestamps with the filter on: every stream answers E_NOTIMPL -- through its own HRESULT, before anything is uploaded"""
    bufs, _, _ = expected
    bufs_c = [np.ascontiguousarray(b, np.float32) for b in bufs]
    ptrs = (C.POINTER(C.c_float) * len(bufs_c))(*[b.ctypes.data_as(C.POINTER(C.c_float)) for b in bufs_c])
    lens = (C.c_int32 * len(bufs_c))(*[len(b) for b in bufs_c])
    descs = (StreamDesc * 2)(StreamDesc(0, 0, 0), StreamDesc(1, 0, 0))
    pt = (C.c_int32 * 1)(1000)
    hr = lib.sf_run(model_path.encode(), 0, H.FLAG_NO_CONTEXT | 0x100, H.language_key("en"), 0, C.cast(pt, C.POINTER(C.c_int32)), 1, ptrs, lens, len(bufs_c), descs, 2,
                    2, 1, 4, 0, 4, 1, *PARAMS)
    res = json.loads(lib.sf_result().decode())
    assert hr & 0xFFFFFFFF == E_NOTIMPL and [st["hr"] & 0xFFFFFFFF for st in res["streams"]] == [E_NOTIMPL, E_NOTIMPL] and res["packer_calls"] == 0


# ---------------------------------------------------------------------------------------------------------------------
# flat C, Python, tools: what needs no device
# ---------------------------------------------------------------------------------------------------------------------
def test_flat_c_argument_checks_and_exports():
    from whisper_amd import api, binding
    L = api.lib()
    n = C.c_uint32(0)
    assert L.whisperc_set_speech_filter(None, 1, 0, 0, 0) & 0xFFFFFFFF == E_POINTER
    assert L.whisperc_batch_set_speech_filter(None, 0, 0, 0, 0) & 0xFFFFFFFF == E_POINTER
    assert L.whisperc_result_speech_spans(None, None, 0, C.byref(n)) & 0xFFFFFFFF == E_POINTER
    assert L.whisperc_tr_speech_spans(None, None, 0, C.byref(n)) & 0xFFFFFFFF == E_POINTER
    assert L.whisperc_speech_spans(None, 0, 0, 0, 0, None, 0, None) & 0xFFFFFFFF == E_POINTER
    # the parameters are refused before the device is asked for anything
    pcm = np.zeros(1000, np.float32)
    assert L.whisperc_speech_spans(pcm.ctypes.data_as(C.c_void_p), len(pcm), -1, 0, 0, None, 0, C.byref(n)) & 0xFFFFFFFF == E_INVALIDARG
    assert L.whisperc_speech_spans(pcm.ctypes.data_as(C.c_void_p), len(pcm), 0, 0, (1 << 20) + 1, None, 0, C.byref(n)) & 0xFFFFFFFF == E_INVALIDARG
    for f in (api.speech_spans, api.Context.set_speech_filter, api.Context.speech_spans, api.BatchRunner.set_speech_filter):
        assert callable(f)
    assert api._speech_frames(2.0, 0.256, 0.4) == (S.MIN_SILENCE, S.MIN_SPEECH, S.PAD) and api._speech_frames(0, 0, 0) == (0, 0, 0)
    # the compute layer's own argument checks come before any device call
    H_ = binding.lib()
    assert H_.wh_speech_pack(None, None, 3, 0, None, 0, None, 0) == -1
    assert H_.wh_speech_pack(None, None, 1, 100, None, 0, None, 0) == 0
    assert H_.wh_speech_pack_host(None, 1, 100, None, 1, None, 10) == -1
    assert H_.wh_context_speech_filter(None, None, 0, None, None, None, None, None, None, 0, None) == -1


def test_the_tools_take_the_options():
    """whisper-main: --speech-only and the three --so options are parsed out, with their values, before the reference's parser sees the line, so
    --dump-options and the usage text stay the reference's. whisper-mgpu: -speech-only parses (the line then fails for its missing -m and -f, not with
    the usage text an unknown option gets)."""
    from whisper_amd import build
    if not os.path.exists(build.CLI_BIN) or not os.path.exists(build.MGPU_BIN):
        build.build_all()
    run_main = lambda *a: subprocess.run([build.CLI_BIN] + list(a), stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=60)
    plain = run_main("--dump-options", "-f", "a.wav")
    with_it = run_main("--dump-options", "--speech-only", "--so-min-silence", "1.5", "--so-min-speech", "0.1", "--so-pad", "0.2", "-f", "a.wav")
    assert plain.returncode == 0 and with_it.returncode == 0 and with_it.stdout == plain.stdout and "a.wav" in plain.stdout
    for name in ("--so-min-silence", "--so-min-speech", "--so-pad"):
        missing = run_main("--dump-options", "--speech-only", "-f", "a.wav", name)
        assert missing.returncode == 2 and "needs a number" in missing.stderr
        alone = run_main("--dump-options", name, "1.0", "-f", "a.wav")
        assert alone.returncode == 2 and "need --speech-only" in alone.stderr
    usage = run_main("-h")
    assert "speech-only" not in usage.stdout + usage.stderr and "--so-" not in usage.stdout + usage.stderr
    for args in (["-speech-only"], ["--speech-only", "-so-min-silence", "1.0", "-so-min-speech", "0.1", "-so-pad", "0.2"]):
        r = subprocess.run([build.MGPU_BIN] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=60)
        assert r.returncode == 1 and "-m and -f are required" in r.stderr and "usage:" not in r.stderr
    r = subprocess.run([build.MGPU_BIN, "-so-pad", "0.2"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=60)
    assert r.returncode == 1 and "need -speech-only" in r.stderr
