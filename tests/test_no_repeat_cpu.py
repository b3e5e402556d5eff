"""CPU tests of no-repeat n-grams ("No-repeat n-grams"):

  * the numpy restatement (tests/no_repeat_ref.py) against a brute-force enumeration of all n-grams, n = 1 .. 8, and by hand-written expectations;
  * the lock-step scheduler: whisper_amd/host/batchScheduler.cpp compiled UNCHANGED next to the unchanged test double of the compute layer and
    tests/no_repeat_cpu/batch_driver.cpp, whose injected hook (batchNoRepeat.h) records every call. The hook filters nothing, so the transcripts must be those
    of a runner on which nothing was set: what is tested is who is told what, and when;
  * argument checks of the flat C layer that need no device, and the tools' option parsing.
The GPU twin: tests/test_gpu_no_repeat.py."""
import ctypes as C
import json
import os
import shutil
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest

import no_repeat_ref as R
import test_hostloop_cpu as H
from test_batch_cpu import StreamDesc, recordings
from whisper_amd import ggml_format as gf

ROOT = H.ROOT
HOST = os.path.join(ROOT, "whisper_amd", "host")
LIB = os.path.join(H.BUILD, "libno_repeat_cpu.so")
SOURCES = [os.path.join(ROOT, "tests", "no_repeat_cpu", "batch_driver.cpp")] + [os.path.join(HOST, f) for f in ("batchScheduler.cpp", "support.cpp", "tokenTimestamps.cpp")]
DEPS = SOURCES + [os.path.join(HOST, f) for f in os.listdir(HOST) if f.endswith(".h")] + [os.path.join(ROOT, "include", h) for h in ("whisperApi.h", "whisper_hip.h")] + \
       [os.path.join(ROOT, "tests", "hostloop_cpu", f) for f in ("fake_device.cpp", "batch_driver.cpp")]
INCLUDES = ["-I" + os.path.join(ROOT, "include"), "-I" + HOST]
E_POINTER, E_INVALIDARG, E_NOTIMPL = 0x80004003, 0x80070057, 0x80004001
NO_CALL = -100


def layout(n_vocab):
    sp = gf.special_tokens(SimpleNamespace(n_vocab=n_vocab))
    return sp["eot"], sp["beg"]


# ---------------------------------------------------------------------------------------------------------------------
# the restatement
# ---------------------------------------------------------------------------------------------------------------------
def brute_force(history, n, eot):
    """All n-grams of the history as a set of tuples; t is forbidden when ( the last n - 1 tokens ) + ( t, ) is one of them -- Hugging Face's
    _get_ngrams / _get_generated_ngrams -- and t is a text token."""
    h = [int(t) for t in history]
    if len(h) < n:
        return []
    grams = {tuple(h[i:i + n]) for i in range(len(h) - n + 1)}
    tail = tuple(h[len(h) - n + 1:]) if n > 1 else ()
    return sorted({g[-1] for g in grams if g[:-1] == tail and g[-1] < eot})


@pytest.mark.parametrize("n", range(1, 9))
def test_the_restatement_against_brute_force(n):
    eot, beg = layout(51865)
    rng = np.random.default_rng(100 + n)
    total = 0
    for h in R.histories(rng, 12, 40, eot, beg):
        for L in range(len(h) + 1):
            got = R.banned(h[:L], n, eot)
            assert got == brute_force(h[:L], n, eot), (n, h[:L])
            assert all(t < eot for t in got) and (L >= n or got == [])
            total += len(got)
    assert total > 0                                                             # n-grams do recur on six ids, even at n = 8 (the a b a b loop)


def test_the_restatement_by_hand():
    eot, beg = layout(51865)
    a, b, c, ts = 5, 6, 7, beg + 10
    assert R.banned([], 1, eot) == [] and R.banned([a], 2, eot) == [] and R.banned([a, b], 3, eot) == []
    assert R.banned([a, b, a], 1, eot) == [a, b]                                 # n = 1: no text token twice
    assert R.banned([a, eot, ts], 1, eot) == [a]                                 # eot and timestamps are never forbidden
    assert R.banned([a, b, a], 2, eot) == [b]                                    # a b a -> b would repeat ( a, b )
    assert R.banned([a, b, c, a], 2, eot) == [b] and R.banned([a, b, c, a, b], 2, eot) == [c]
    assert R.banned([a, a], 2, eot) == [a]                                       # i = L - n: the n-gram that ends at the last token counts
    assert R.banned([a, b, c, a, b], 3, eot) == [c] and R.banned([a, b, c, b], 3, eot) == []
    assert R.banned([ts, a, ts], 2, eot) == [a]                                  # timestamps are part of the history ...
    assert R.banned([a, ts, a], 2, eot) == []                                    # ... but never a forbidden column
    assert R.banned([a, eot, a], 2, eot) == []
    x = np.arange(20, dtype=np.float32)
    y = R.apply(x, [3, 4, 3], 2, 10)
    assert np.isneginf(y[4]) and np.array_equal(np.delete(y, 4), np.delete(x, 4))
    assert R.violations([a, b, a, b], 2, eot) == [3] and R.violations([a, b, a, c, a, ts, a, eot], 2, eot) == []
    assert R.violations([a, b, c, a, b, c], 3, eot) == [5] and R.violations([a, b, c, a, b, c], 4, eot) == []
    assert R.violations([a, a], 1, eot) == [1] and R.violations([ts, ts, eot, eot], 1, eot) == []
    al = R.alphabet(eot, beg)
    assert len(al) == 6 and eot in al and sum(t >= beg for t in al) == 2 and sum(t < eot for t in al) == 3


# ---------------------------------------------------------------------------------------------------------------------
# the scheduler over the test double
# ---------------------------------------------------------------------------------------------------------------------
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
    L.nr_run.argtypes = run_args + [C.POINTER(C.c_int32), C.c_int]
    L.bt_result.restype = C.c_char_p
    L.nr_result.restype = C.c_char_p
    L.nr_install_hook(1)
    return L


@pytest.fixture(scope="module")
def model_path(tmp_path_factory):
    model = gf.conditioned_model(gf.conditioned_layout(gf.hparams_for("test-d128-ml")), 4, kind="test-d128-ml", seed=10)
    path = str(tmp_path_factory.mktemp("nrn") / "m.bin")
    gf.write_model(path, model)
    return path


STREAMS = [(0, 0, 0), (1, 0, 0), (2, 0, 0), (3, 0, 0), (4, 0, 0), (4, 16000 * 5, 16000 * 9)]


def run(L, path, slots, groups, script=(), plain=False):
    bufs = [np.ascontiguousarray(b, np.float32) for b in recordings()]
    ptrs = (C.POINTER(C.c_float) * len(bufs))(*[b.ctypes.data_as(C.POINTER(C.c_float)) for b in bufs])
    lens = (C.c_int32 * len(bufs))(*[len(b) for b in bufs])
    descs = (StreamDesc * len(STREAMS))(*[StreamDesc(b, f, n) for (b, f, n) in STREAMS])
    pt = (C.c_int32 * 1)(1000)
    common = (path.encode(), 0, H.FLAG_NO_CONTEXT, H.language_key("en"), 0, C.cast(pt, C.POINTER(C.c_int32)), 1, ptrs, lens, len(bufs), descs, len(STREAMS),
              slots, groups, 4, 0, 4)
    if plain:
        hr = L.bt_run(*common)
        return hr, json.loads(L.bt_result().decode())
    a = (C.c_int32 * len(script))(*script)
    hr = L.nr_run(*common, a, len(script))
    return hr, json.loads(L.nr_result().decode())


def transcripts(res):
    return [(st["hr"], [(s["t0"], s["t1"], s["text"], s["tokens"]) for s in st["segments"]]) for st in res["streams"]]


@pytest.mark.parametrize("slots,groups", [(1, 1), (2, 1), (5, 1), (2, 2), (5, 2)])
def test_every_context_gets_n_before_its_first_window(lib, model_path, slots, groups):
    """1 / 2 / 5 slots, 1 / 2 groups, five runs of one runner: n = 2 before run 0, nothing before run 1, n = 3 before run 2, 0 before run 3, n = 3 again before run
    4. Every context the runner creates hears each new n exactly once, before it started a window of that
    run; runs that change nothing tell nobody. The recording hook filters nothing: the transcripts are those of the unchanged harness."""
    hr0, plain = run(lib, model_path, slots, groups, plain=True)
    hr, res = run(lib, model_path, slots, groups, script=[2, NO_CALL, 3, 0, 3])
    assert hr0 == 0 and hr == 0 and transcripts(res) == transcripts(plain) and sum(len(s["segments"]) for s in plain["streams"]) >= 6
    calls = res["calls"]
    used = res["counters"][0] - 1                                                # the groups' contexts alive at the end, without the loader
    assert used == min(groups, len(STREAMS) // 2)
    by_run = {r: [c for c in calls if c["run"] == r] for r in range(5)}
    assert by_run[1] == [] and len(calls) == 4 * used
    starts = {}
    for r, n in ((0, 2), (2, 3), (3, 0), (4, 3)):
        assert sorted(c["context"] for c in by_run[r]) == list(range(used)) and all(c["n"] == n for c in by_run[r]), (r, by_run[r])
        for c in by_run[r]:
            # told before the context's first window of that run: its count of window starts is what the run before left
            assert c["starts"] >= starts.get(c["context"], 0) and (r > 0 or c["starts"] == 0), c
            starts[c["context"]] = c["starts"]
    assert all(c["starts"] > 0 for c in by_run[2])                               # ... and the earlier runs did start windows


def test_off_only_no_hook_and_bad_n(lib, model_path):
    """Never set, only ever 0, or set and cleared before a run: the hook is not called. Without the hook n != 0 is E_NOTIMPL and 0 is S_OK. n = 9 and n = -1
    are E_INVALIDARG, with the hook and without it (the argument check comes first). Results: the unchanged harness's, every time."""
    hr0, plain = run(lib, model_path, 2, 2, plain=True)
    assert hr0 == 0
    for script in ([NO_CALL], [0], [102], [100], [0, 103], [108, NO_CALL]):
        hr, res = run(lib, model_path, 2, 2, script=script)
        assert hr == 0 and res["calls"] == [] and transcripts(res) == transcripts(plain), script
    for script in ([9], [-1], [NO_CALL, 9], [2, -1]):
        hr, res = run(lib, model_path, 2, 2, script=script)
        assert hr & 0xFFFFFFFF == E_INVALIDARG and res == {}, script
    lib.nr_install_hook(0)
    try:
        for script in ([1], [NO_CALL, 8], [103]):
            hr, res = run(lib, model_path, 2, 2, script=script)
            assert hr & 0xFFFFFFFF == E_NOTIMPL and res == {}, script
        for script in ([9], [-1]):
            hr, res = run(lib, model_path, 2, 2, script=script)
            assert hr & 0xFFFFFFFF == E_INVALIDARG and res == {}, script
        for script in ([NO_CALL], [0], [0, 0]):
            hr, res = run(lib, model_path, 2, 2, script=script)
            assert hr == 0 and res["calls"] == [] and transcripts(res) == transcripts(plain), script
    finally:
        lib.nr_install_hook(1)


# ---------------------------------------------------------------------------------------------------------------------
# flat C, Python, tools: what needs no device
# ---------------------------------------------------------------------------------------------------------------------
def test_flat_c_argument_checks_and_exports():
    from whisper_amd import api, binding
    L = api.lib()
    assert L.whisperc_set_no_repeat_ngram(None, 2) & 0xFFFFFFFF == E_POINTER
    assert L.whisperc_batch_set_no_repeat_ngram(None, 0) & 0xFFFFFFFF == E_POINTER
    assert "wh_context_set_no_repeat" in binding.EXPORTS and "wh_op_no_repeat_ngram" in binding.EXPORTS
    assert callable(api.Context.set_no_repeat_ngram) and callable(api.BatchRunner.set_no_repeat_ngram) and callable(binding.HipContext.set_no_repeat)
    # the compute layer's own argument checks come before any device call
    H_ = binding.lib()
    assert H_.wh_context_set_no_repeat(None, 2) != 0
    assert H_.wh_op_no_repeat_ngram(None, None, 1, 8, 2, 2, None, 1, None, None, 4) != 0


def test_the_tools_take_the_option():
    """whisper-main: -nrn N / --no-repeat-ngram N are parsed out, with their value, before the reference's parser sees the line, so --dump-options and the usage
    text stay the reference's. whisper-mgpu: -nrn N parses (the line then fails for its missing -m and -f, not with the usage text an unknown option gets)."""
    from whisper_amd import build
    if not os.path.exists(build.CLI_BIN) or not os.path.exists(build.MGPU_BIN):
        build.build_all()
    run_main = lambda *a: subprocess.run([build.CLI_BIN] + list(a), stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=60)
    plain = run_main("--dump-options", "-f", "a.wav")
    for name in ("-nrn", "--no-repeat-ngram"):
        with_it = run_main("--dump-options", name, "3", "-f", "a.wav")
        assert plain.returncode == 0 and with_it.returncode == 0 and with_it.stdout == plain.stdout and "a.wav" in plain.stdout
        missing = run_main("--dump-options", "-f", "a.wav", name)
        assert missing.returncode == 2 and "needs a number" in missing.stderr
    usage = run_main("-h")
    assert "-nrn" not in usage.stdout + usage.stderr and "no-repeat" not in usage.stdout + usage.stderr
    for name in ("-nrn", "--no-repeat-ngram"):
        r = subprocess.run([build.MGPU_BIN, name, "3"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=60)
        assert r.returncode == 1 and "-m and -f are required" in r.stderr and "usage:" not in r.stderr
    usage = subprocess.run([build.MGPU_BIN, "-nrx"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=60)
    assert usage.returncode == 1 and "usage: whisper-mgpu" in usage.stderr and "-nrn" not in usage.stderr
