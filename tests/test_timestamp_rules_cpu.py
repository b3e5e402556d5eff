"""CPU tests of the timestamp rules ("Timestamp rules"):

  * the numpy restatement (tests/timestamp_rules_ref.py) on the histories the GPU tests drive the kernel through, by hand-written expectations, and against
    transformers' WhisperTimeStampLogitsProcessor, whose __call__ is openai-whisper's ApplyTimestampRules, on inputs where that class's other clauses stay
    silent: its -inf set must be ours plus <|notimestamps|>;
  * the lock-step scheduler: whisper_amd/host/batchScheduler.cpp compiled UNCHANGED next to the unchanged test double of the compute layer and
    tests/timestamp_rules_cpu/batch_driver.cpp, whose injected hook (batchTimestampRules.h) records every call. The hook filters nothing, so the transcripts
    must be those of a runner on which nothing was set: what is tested is who is told what, and when;
  * argument checks of the flat C layer that need no device, and the tools' option parsing.
The GPU twin: tests/test_gpu_timestamp_rules.py."""
import ctypes as C
import json
import os
import shutil
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest

import test_hostloop_cpu as H
import timestamp_rules_ref as R
from test_batch_cpu import StreamDesc, recordings
from whisper_amd import ggml_format as gf

ROOT = H.ROOT
HOST = os.path.join(ROOT, "whisper_amd", "host")
LIB = os.path.join(H.BUILD, "libtimestamp_rules_cpu.so")
SOURCES = [os.path.join(ROOT, "tests", "timestamp_rules_cpu", "batch_driver.cpp")] + [os.path.join(HOST, f) for f in ("batchScheduler.cpp", "support.cpp", "tokenTimestamps.cpp")]
DEPS = SOURCES + [os.path.join(HOST, f) for f in os.listdir(HOST) if f.endswith(".h")] + [os.path.join(ROOT, "include", h) for h in ("whisperApi.h", "whisper_hip.h")] + \
       [os.path.join(ROOT, "tests", "hostloop_cpu", f) for f in ("fake_device.cpp", "batch_driver.cpp")]
INCLUDES = ["-I" + os.path.join(ROOT, "include"), "-I" + HOST]
E_POINTER, E_INVALIDARG, E_NOTIMPL = 0x80004003, 0x80070057, 0x80004001

# the vocabulary layouts: the synthetic test models' and the real checkpoints' (.en, multilingual, large-v3)
LAYOUTS = [51864, 51865, 51866]


def layout(n_vocab):
    sp = gf.special_tokens(SimpleNamespace(n_vocab=n_vocab))
    return sp["eot"], sp["beg"], sp["not_"]


# ---------------------------------------------------------------------------------------------------------------------
# the restatement
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V", LAYOUTS)
def test_the_restatement_by_hand(V):
    """Every history of the issue, the expected ranges written out."""
    eot, beg, _ = layout(V)
    assert 0 < eot < beg < V and V - beg in (1501, 1502)
    h = R.histories(eot, beg, V)
    ts, ts2 = beg + 37, beg + 301
    want = {
        "empty": [],
        "ts": [(beg, V), (beg, ts + 1)],                     # fewer than two sampled: "the one before" counts as a timestamp
        "text": [],
        "text_ts": [(0, eot), (beg, ts)],                    # the pair must close; it may close at the time it opened
        "ts_ts": [(beg, V), (beg, ts2 + 1)],
        "ts_text": [(beg, ts + 1)],
        "ts_ts_text_ts": [(0, eot), (beg, ts2)],
        "last_is_beg": [(0, eot)],                           # [beg, beg) is empty
        "closed_at_beg": [(beg, V), (beg, beg + 1)],
        "last_is_top": [(0, eot), (beg, V - 1)],
        "closed_at_top": [(beg, V), (beg, V)],
        "text_after_top": [(beg, V)],                        # last + 1 held to nVocab
    }
    assert set(want) == set(h)
    for name, hist in h.items():
        assert R.masked_ranges(hist, eot, beg, V) == want[name], name
        m = R.mask(hist, eot, beg, V)
        ref = np.zeros(V, bool)
        for lo, hi in want[name]:
            ref[lo:hi] = True
        assert np.array_equal(m, ref), name
        assert not m[eot:beg].any(), name                    # eot and the special ids always stay: a row keeps mass
    x = np.arange(V, dtype=np.float32)
    y = R.apply(x, h["text_ts"], eot, beg)
    assert np.isneginf(y[:eot]).all() and np.array_equal(y[eot:beg], x[eot:beg]) and np.isneginf(y[beg:ts]).all() and np.array_equal(y[ts:], x[ts:])
    assert R.violations([ts, 5, ts2, ts2, 7, eot], eot, beg, V) == []
    assert R.violations([ts, 5, ts2, ts], eot, beg, V) == [3]                       # back in time
    assert R.violations([ts, 5, ts2, 6], eot, beg, V) == [3]                        # text behind an open pair
    assert R.violations([ts, ts], eot, beg, V) == [1]                               # the window's first timestamp opens nothing a second one could close
    assert R.violations([ts, 5, ts2, ts2, ts2 + 1], eot, beg, V) == [4]             # a third timestamp in a row
    assert R.violations([ts, 5, ts2, ts2, 6, ts2], eot, beg, V) == [5]              # a segment of zero length


@pytest.mark.parametrize("V", LAYOUTS)
def test_the_restatement_against_transformers(V):
    """WhisperTimeStampLogitsProcessor.__call__ on [prompt | history]: timestamp logits 30 below the text logits keep its probability-mass clause silent, a
    history of at least one token its initial-timestamp clause. Its -inf set = ours + <|notimestamps|>, every other score unchanged."""
    torch = pytest.importorskip("torch")
    try:
        from transformers.generation.logits_process import WhisperTimeStampLogitsProcessor
    except Exception as e:                                                          # noqa: BLE001 -- the cross-check alone is skipped
        pytest.skip("transformers' WhisperTimeStampLogitsProcessor is not importable: %r" % (e,))
    eot, beg, tnot = layout(V)
    assert tnot + 1 == beg
    cfg = SimpleNamespace(no_timestamps_token_id=tnot, eos_token_id=eot, bos_token_id=eot, max_initial_timestamp_index=50, _detect_timestamp_from_logprob=True)
    prompt = [eot + 1, eot + 2, eot + 3]
    proc = WhisperTimeStampLogitsProcessor(cfg, begin_index=len(prompt))
    rng = np.random.default_rng(V)
    checked = 0
    for name, hist in R.histories(eot, beg, V).items():
        if not hist:
            continue
        scores = rng.standard_normal(V).astype(np.float32)
        scores[beg:] -= 30.0
        out = proc(torch.tensor([prompt + hist], dtype=torch.long), torch.from_numpy(scores)[None, :])[0].numpy()
        theirs = np.isneginf(out)
        ours = R.mask(hist, eot, beg, V)
        ours_plus = ours.copy()
        ours_plus[tnot] = True
        assert np.array_equal(theirs, ours_plus), name
        assert np.array_equal(out[~theirs].view(np.uint32), scores[~theirs].view(np.uint32)), name
        checked += 1
    assert checked >= 9


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
    L.tr_run.argtypes = run_args + [C.POINTER(C.c_int32), C.c_int]
    L.bt_result.restype = C.c_char_p
    L.tr_result.restype = C.c_char_p
    L.tr_install_hook(1)
    return L


@pytest.fixture(scope="module")
def model_path(tmp_path_factory):
    model = gf.conditioned_model(gf.conditioned_layout(gf.hparams_for("test-d128-ml")), 4, kind="test-d128-ml", seed=10)
    path = str(tmp_path_factory.mktemp("tsr") / "m.bin")
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
    hr = L.tr_run(*common, a, len(script))
    return hr, json.loads(L.tr_result().decode())


def transcripts(res):
    return [(st["hr"], [(s["t0"], s["t1"], s["text"], s["tokens"]) for s in st["segments"]]) for st in res["streams"]]


@pytest.mark.parametrize("slots,groups", [(1, 1), (2, 1), (5, 1), (2, 2), (5, 2)])
def test_every_group_is_told_once_per_change(lib, model_path, slots, groups):
    """1 / 2 / 5 slots, 1 / 2 groups, four runs of one runner: on before run 0, nothing before run 1, off before run 2, on twice before run 3. Every group's
    context hears each change exactly once, before it started a window of that run; run 1 tells nobody. The recording hook filters nothing: the transcripts
    are those of the unchanged harness."""
    hr0, plain = run(lib, model_path, slots, groups, plain=True)
    hr, res = run(lib, model_path, slots, groups, script=[1, -1, 0, 3])
    assert hr0 == 0 and hr == 0 and transcripts(res) == transcripts(plain) and sum(len(s["segments"]) for s in plain["streams"]) >= 6
    calls = res["calls"]
    used = res["counters"][0] - 1                                                # the groups' contexts alive at the end, without the loader
    assert used == min(groups, len(STREAMS) // 2)
    by_run = {r: [c for c in calls if c["run"] == r] for r in range(4)}
    assert by_run[1] == [] and len(calls) == 3 * used
    starts = {}
    for r, on in ((0, 1), (2, 0), (3, 1)):
        assert sorted(c["context"] for c in by_run[r]) == list(range(used)) and all(c["on"] == on for c in by_run[r]), (r, by_run[r])
        for c in by_run[r]:
            # told before the context's first window of that run: its count of window starts is what the run before left
            assert c["starts"] >= starts.get(c["context"], 0) and (r > 0 or c["starts"] == 0), c
            starts[c["context"]] = c["starts"]
    assert all(c["starts"] > 0 for c in by_run[2])                               # ... and the earlier runs did start windows


def test_off_only_and_no_hook(lib, model_path):
    """Never set, only ever off, or on and off again before a run: the hook is not called. Without the hook turning the rules on is E_NOTIMPL and turning them
    off S_OK. Results: the unchanged harness's, every time."""
    hr0, plain = run(lib, model_path, 2, 2, plain=True)
    assert hr0 == 0
    for script in ([-1], [0], [2], [0, 2]):
        hr, res = run(lib, model_path, 2, 2, script=script)
        assert hr == 0 and transcripts(res) == transcripts(plain), script
        # on and off again is two changes: a group hears the state it must be in, off, once -- or nothing
        assert all(c["on"] == 0 for c in res["calls"]) and (res["calls"] == [] or 2 in script), script
    lib.tr_install_hook(0)
    try:
        for script in ([1], [-1, 1], [3]):
            hr, res = run(lib, model_path, 2, 2, script=script)
            assert hr & 0xFFFFFFFF == E_NOTIMPL and res == {}, script
        for script in ([-1], [0], [0, 0]):
            hr, res = run(lib, model_path, 2, 2, script=script)
            assert hr == 0 and res["calls"] == [] and transcripts(res) == transcripts(plain), script
    finally:
        lib.tr_install_hook(1)


# ---------------------------------------------------------------------------------------------------------------------
# flat C, Python, tools: what needs no device
# ---------------------------------------------------------------------------------------------------------------------
def test_flat_c_argument_checks_and_exports():
    from whisper_amd import api, binding
    L = api.lib()
    assert L.whisperc_set_timestamp_rules(None, 1) & 0xFFFFFFFF == E_POINTER
    assert L.whisperc_batch_set_timestamp_rules(None, 0) & 0xFFFFFFFF == E_POINTER
    assert "wh_context_set_timestamp_rules" in binding.EXPORTS and "wh_op_timestamp_rules" in binding.EXPORTS
    assert callable(api.Context.set_timestamp_rules) and callable(api.BatchRunner.set_timestamp_rules) and callable(binding.HipContext.set_timestamp_rules)
    # the compute layer's own argument checks come before any device call
    H_ = binding.lib()
    assert H_.wh_context_set_timestamp_rules(None, 1) != 0
    assert H_.wh_op_timestamp_rules(None, None, 1, 8, 2, 4, None, 1, None) != 0


def test_the_tools_take_the_option():
    """whisper-main: -tsr / --timestamp-rules are parsed out before the reference's parser sees the line, so --dump-options and the usage text stay the
    reference's. whisper-mgpu: -tsr parses (the line then fails for its missing -m and -f, not with the usage text an unknown option gets)."""
    from whisper_amd import build
    if not os.path.exists(build.CLI_BIN) or not os.path.exists(build.MGPU_BIN):
        build.build_all()
    run_main = lambda *a: subprocess.run([build.CLI_BIN] + list(a), stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=60)
    plain = run_main("--dump-options", "-f", "a.wav")
    for name in ("-tsr", "--timestamp-rules"):
        with_it = run_main("--dump-options", name, "-f", "a.wav")
        assert plain.returncode == 0 and with_it.returncode == 0 and with_it.stdout == plain.stdout and "a.wav" in plain.stdout
    usage = run_main("-h")
    assert "-tsr" not in usage.stdout + usage.stderr and "timestamp-rules" not in usage.stdout + usage.stderr
    for name in ("-tsr", "--timestamp-rules"):
        r = subprocess.run([build.MGPU_BIN, name], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=60)
        assert r.returncode == 1 and "-m and -f are required" in r.stderr and "usage:" not in r.stderr
    usage = subprocess.run([build.MGPU_BIN, "-tsx"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=60)
    assert usage.returncode == 1 and "usage: whisper-mgpu" in usage.stderr and "-tsr" not in usage.stderr
