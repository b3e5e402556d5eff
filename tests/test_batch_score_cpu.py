"""Whisper::scoreBatch in the lock-step scheduler, on the CPU: batchScheduler.cpp over the test double of the compute layer (tests/hostloop_cpu/fake_device.cpp,
unchanged) with a scorer of its own installed -- wh_score_tokens played by the double's per-slot reference models (tests/hostloop_cpu/batch_score_driver.cpp).
Every request must receive the records of ITS clip and tokens, held against the rows of WhisperNP.decode (the reference's numerics), whatever maxSlots and the
order of the requests, for pieces of one buffer and with a failing request beside good ones. Without a scorer the call answers E_NOTIMPL."""
import ctypes as C
import json
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

import token_score_ref as TS
from oracle import whisper_np as wn
from whisper_amd import ggml_format as gf

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))
import make_golden_score as mk  # noqa: E402

BUILD = os.path.join(HERE, "_build")
REF_DIR = os.path.join(ROOT, "oracle", "_ref")
LIB = os.path.join(BUILD, "libbatch_score_cpu.so")
SOURCES = [os.path.join(HERE, "hostloop_cpu", "batch_score_driver.cpp")] + \
          [os.path.join(ROOT, "whisper_amd", "host", f) for f in ("batchScheduler.cpp", "support.cpp", "tokenTimestamps.cpp")]
E_NOTIMPL, E_INVALIDARG = 0x80004001, 0x80070057
THREADS = 4
# The double runs the reference itself; WhisperNP restates it within tests/test_oracle.py's bound on a logit, E2E_MAX = 4e-3. A log-probability is a logit minus
# the row's log-sum-exp, each of which moves by at most that: 2 x E2E_MAX. best and rank may differ only by ids WhisperNP holds closer than that to the maximum
# resp. to the target's logit.
FLIP = 2 * 4e-3


class RequestDesc(C.Structure):
    _fields_ = [("buffer", C.c_int32), ("promptOff", C.c_int32), ("promptCount", C.c_int32), ("tokenOff", C.c_int32), ("tokenCount", C.c_int32), ("flags", C.c_uint32),
                ("firstSample", C.c_int64), ("countSamples", C.c_int64)]


@pytest.fixture(scope="module")
def lib():
    """Linked with --no-undefined like tests/test_batch_cpu.py's library: the scheduler holds no reference to the compute layer's scoring entry."""
    if not os.path.exists(os.path.join(REF_DIR, "libwhisper_ref.so")):
        pytest.skip("oracle/_ref/libwhisper_ref.so not built (needs the reference tree)")
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    os.makedirs(BUILD, exist_ok=True)
    hdr = [os.path.join(ROOT, "whisper_amd", "host", f) for f in os.listdir(os.path.join(ROOT, "whisper_amd", "host")) if f.endswith(".h")]
    deps = SOURCES + hdr + [os.path.join(HERE, "hostloop_cpu", f) for f in ("fake_device.cpp", "batch_driver.cpp")] + [os.path.join(REF_DIR, "libwhisper_ref.so")]
    if not os.path.exists(LIB) or any(os.path.getmtime(d) > os.path.getmtime(LIB) for d in deps):
        cmd = ["g++", "-std=c++17", "-O1", "-fPIC", "-shared", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "whisper_amd", "host"),
               "-I" + os.path.join(HERE, "hostloop_cpu")] + SOURCES + \
              ["-o", LIB, "-L" + REF_DIR, "-lwhisper_ref", "-Wl,-rpath," + REF_DIR, "-Wl,-Bsymbolic", "-Wl,--no-undefined", "-lpthread"]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        assert r.returncode == 0, r.stdout
    L = C.CDLL(LIB)
    L.bs_run.argtypes = [C.c_char_p, C.POINTER(C.POINTER(C.c_float)), C.POINTER(C.c_int32), C.c_int, C.POINTER(RequestDesc), C.c_int, C.POINTER(C.c_int32), C.c_uint32, C.c_int]
    L.bs_result.restype = C.c_char_p
    return L


def _run(L, path, buffers, requests, slots):
    """requests: (buffer, first, count, prompt, tokens, flags)"""
    bufs = [np.ascontiguousarray(b, np.float32) for b in buffers]
    ptrs = (C.POINTER(C.c_float) * len(bufs))(*[b.ctypes.data_as(C.POINTER(C.c_float)) for b in bufs])
    lens = (C.c_int32 * len(bufs))(*[len(b) for b in bufs])
    pool, descs = [], []
    for b, first, count, prompt, tokens, flags in requests:
        descs.append(RequestDesc(b, len(pool), len(prompt), len(pool) + len(prompt), len(tokens), flags, first, count))
        pool += list(prompt) + list(tokens)
    pool_c = (C.c_int32 * max(len(pool), 1))(*pool)
    hr = L.bs_run(path.encode(), ptrs, lens, len(bufs), (RequestDesc * len(descs))(*descs), len(descs), pool_c, slots, THREADS) & 0xFFFFFFFF
    return hr, json.loads(L.bs_result().decode())


def test_every_request_receives_the_records_of_its_own_clip_and_tokens(lib, tmp_path):
    model = mk.model()
    sp = gf.special_tokens(model.hparams)
    path = str(tmp_path / "m.bin")
    gf.write_model(path, model)
    rng = np.random.default_rng(41)
    bufs = [(0.3 * rng.standard_normal(16000 * 5)).astype(np.float32), (0.3 * rng.standard_normal(16000 * 2)).astype(np.float32)]
    head = [sp["sot"], sp["sot"] + 1, sp["transcribe"], sp["not_"]]
    # two pieces of one buffer, a whole buffer with a past prompt and timestamps among the tokens, and a request that fails its checks between them
    good = [(0, 0, 16000 * 2, head, [2065, 2131, 2195], 0), (0, 16000 * 2, 0, head, [400, 401, 402, 403, 404, 405, 406], 0),
            (1, 0, 0, [sp["prev"], 1500] + head[:3], [sp["beg"] + 3, 2065, 2131, sp["beg"] + 40], 0)]
    bad = (1, 0, 0, head, [model.hparams.n_vocab], 0)
    requests = [good[0], bad, good[1], good[2]]
    # the yardstick: WhisperNP on the request's own clip, the records of the definition from the logits of every fed row
    npm, want = wn.WhisperNP(model), {}
    for r in good:
        b, first, count, prompt, tokens, _ = r
        clip = bufs[b][first:first + count] if count else bufs[b][first:]
        npm.encode(wn.log_mel_spectrogram(clip, model.filters), 0, n_threads=THREADS)
        row = list(prompt) + list(tokens) + [sp["eot"]]
        logits, _ = npm.decode(row, 0, n_threads=THREADS)
        want[id(r)] = []
        for i in range(len(prompt), len(row)):
            x = logits[i - 1].astype(np.float64)
            srt = np.sort(x)
            # ids an order may flip with: those within FLIP of the target's logit, and the runner-up when it is within FLIP of the maximum
            want[id(r)].append(TS.score_row(x, row[i]) + (int((np.abs(np.delete(x, row[i]) - x[row[i]]) < FLIP).sum()), bool(srt[-1] - srt[-2] < FLIP)))
    worst = 0.0
    for slots, order in ((1, 1), (2, -1), (5, 1)):
        reqs = requests[::order]
        hr, got = _run(lib, path, bufs, reqs, slots)
        assert hr == E_INVALIDARG, (slots, hex(hr))                               # the first failure, and the good requests scored all the same
        assert got["calls"] == {1: [1, 1, 1], 2: [2, 1], 5: [3]}[slots], (slots, got["calls"])
        for r, g in zip(reqs, got["requests"]):
            if r is bad:
                assert g["hr"] & 0xFFFFFFFF == E_INVALIDARG and all(rec[3] == -7 for rec in g["records"])
                continue
            assert g["hr"] == 0 and len(g["records"]) == len(r[4]) + 1
            for rec, w in zip(g["records"], want[id(r)]):
                assert (rec[2] == w[2] or w[5]) and abs(rec[3] - w[3]) <= w[4] and rec[4] == 0, (slots, rec, w)
                worst = max(worst, abs(rec[0] - w[0]), abs(rec[1] - w[1]))
                assert abs(rec[0] - w[0]) <= FLIP and abs(rec[1] - w[1]) <= FLIP, (slots, rec, w)
        # a request's records are its own: no other request's expected records fit them
        firsts = {id(r): g["records"][0][0] for r, g in zip(reqs, got["requests"]) if r is not bad}
        for r in good:
            assert all(abs(firsts[id(r)] - want[id(o)][0][0]) > 10 * FLIP for o in good if o is not r)
    print("largest |record - WhisperNP| %.3e (bound %.1e)" % (worst, FLIP))
    # no scorer installed: E_NOTIMPL, nothing written
    lib.bs_install_scorer(0)
    try:
        hr, got = _run(lib, path, bufs, [good[0]], 2)
        assert hr == E_NOTIMPL and got["calls"] == [] and got["requests"][0]["records"][0][3] == -7
    finally:
        lib.bs_install_scorer(1)
    # forced alignment is not available in a batch runner
    hr, got = _run(lib, path, bufs, [(0, 0, 16000 * 2, head, [2065, 2131], 1)], 2)
    assert hr == E_NOTIMPL and got["requests"][0]["hr"] & 0xFFFFFFFF == E_NOTIMPL
