"""CPU tests of phrase boosting ("Phrase boosting"): the compiled automaton (wh_boost_compile) and the host twin of one step of the kernel
(wh_boost_step_host) against the brute-force restatement, tests/phrase_boost_ref.py, bit for bit; the limits and refusals. No device is needed.
The GPU twin: tests/test_gpu_phrase_boost.py."""
import ctypes as C

import numpy as np
import pytest

import phrase_boost_ref as R
from whisper_amd import binding

EOT, V = 50257, 51865
BOOST = 2.5
SETS = R.sets(EOT)


def _unpack(tables):
    nodes, entries = int(tables[0]), int(tables[1])
    off = tables[4:4 + nodes + 1]
    tok = tables[5 + nodes:5 + nodes + entries]
    nxt = tables[5 + nodes + entries:5 + nodes + 2 * entries]
    assert len(tables) == 5 + nodes + 2 * entries and tables[3] == 0
    assert tables[2:3].view(np.float32)[0] == np.float32(BOOST)
    return nodes, off, tok, nxt


def _delta(off, tok, nxt, n, t):
    """n's entry, else the root's, else the root -- the rule the header states"""
    for m in (n, 0):
        seg = tok[off[m]:off[m + 1]]
        i = int(np.searchsorted(seg, t))
        if i < len(seg) and seg[i] == t:
            return int(nxt[off[m] + i])
    return 0


@pytest.mark.parametrize("name", sorted(SETS))
def test_tables_against_the_restatement(name):
    """For random histories with timestamps and eot mixed in: the state the tables reach stands for the longest suffix of h that begins a phrase (one node per
    such suffix, one suffix per node), and the tokens offered there -- the node's and the root's -- are O(h) by brute force. Every node's tokens ascend."""
    phrases = SETS[name]
    tables = binding.boost_compile(phrases, EOT, V, BOOST)
    nodes, off, tok, nxt = _unpack(tables)
    assert off[0] == 0 and off[nodes] == len(tok) and nodes == 1 + len({tuple(p[:k]) for p in phrases for k in range(1, len(p) + 1)})
    for n in range(nodes):
        seg = tok[off[n]:off[n + 1]]
        assert (np.diff(seg) > 0).all() and ((seg >= 0) & (seg < EOT)).all()
    means, node_of = {0: ()}, {(): 0}
    for s in R.histories(phrases, EOT, V, seed=len(name)):
        n = 0
        for k, t in enumerate(s):
            n = _delta(off, tok, nxt, n, t) if t < EOT else 0
            h = R.tail(s[:k + 1], EOT)
            want = R.longest(phrases, h)
            assert means.setdefault(n, want) == want and node_of.setdefault(want, n) == n, (s[:k + 1], n)
            got = set(tok[off[n]:off[n + 1]].tolist()) | set(tok[off[0]:off[1]].tolist())
            assert got == R.offered(phrases, h), (s[:k + 1], n)
    assert len(means) > 1


def _row(rng):
    x = (3.0 * rng.standard_normal(V)).astype(np.float32)
    x[rng.integers(0, V, 200)] = -np.inf
    x.view(np.uint32)[rng.integers(0, V, 200)] = 0x7FC00000 | rng.integers(1, 1 << 20, 200).astype(np.uint32)      # NaNs with payloads
    return x


@pytest.mark.parametrize("name", sorted(SETS))
def test_host_step_is_the_restatement_bit_for_bit(name):
    """wh_boost_step_host fed a history token by token behind a reset 1: after every step the row is the restatement's, bit for bit -- the offered columns hold
    x + boost (-inf stays -inf), every other float, NaN payloads included, keeps its bits. Resets 1 and 2 boost the root's offers; an armed state folds nothing."""
    phrases = SETS[name]
    tables = binding.boost_compile(phrases, EOT, V, BOOST)
    rng = np.random.default_rng(len(name) + 100)
    boosted = 0
    for s in R.histories(phrases, EOT, V, seed=len(name) + 1, count=3):
        x = _row(rng)
        state, got = binding.boost_step_host(tables, 12345 % int(tables[0]), 0, 1, x, EOT)
        assert state == 0 and np.array_equal(got.view(np.uint32), R.apply(x, phrases, [], EOT, BOOST).view(np.uint32))
        for k, t in enumerate(s):
            x = _row(rng)
            state, got = binding.boost_step_host(tables, state, t, 0, x, EOT)
            want = R.apply(x, phrases, s[:k + 1], EOT, BOOST)
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), s[:k + 1]
            boosted += int((got.view(np.uint32) != x.view(np.uint32)).sum())
        x = _row(rng)
        state, got = binding.boost_step_host(tables, state, 0, 2, x, EOT)
        assert state == -1 and np.array_equal(got.view(np.uint32), R.apply(x, phrases, [], EOT, BOOST).view(np.uint32))
        state, got = binding.boost_step_host(tables, state, phrases[0][0], 0, x, EOT)                  # armed: the fed token is no sample
        assert state == 0 and np.array_equal(got.view(np.uint32), R.apply(x, phrases, [], EOT, BOOST).view(np.uint32))
    assert boosted > 0


def _compile_rc(phrases, boost, eot=EOT, v=V):
    tokens, lens = binding.pack_phrases(phrases)
    n = C.c_int64(-1)
    rc = binding.lib().wh_boost_compile(tokens.ctypes.data_as(C.c_void_p), lens.ctypes.data_as(C.c_void_p), len(lens), tokens.shape[1], eot, v, boost, None, 0, C.byref(n))
    return rc, n.value, binding.lib().wh_last_error().decode(errors="replace") if rc else ""


def test_limits_and_refusals():
    ok = [[5, 6], [7]]
    assert _compile_rc(ok, 1.0)[0] == 0
    n = C.c_int64(-1)
    assert binding.lib().wh_boost_compile(None, None, 0, 0, EOT, V, 0.0, None, 0, C.byref(n)) == 0 and n.value == 0       # count == 0: off
    assert len(binding.boost_compile([], EOT, V, 1.0)) == 0
    rc, _, msg = _compile_rc([[i + 1] for i in range(1025)], 1.0)
    assert rc != 0 and "1024" in msg
    assert _compile_rc([[i + 1] for i in range(1024)], 1.0)[0] == 0
    rc, _, msg = _compile_rc([list(range(1, 18))], 1.0)
    assert rc != 0 and "16" in msg
    assert _compile_rc([list(range(1, 17))], 1.0)[0] == 0
    rc, _, msg = _compile_rc([[5, EOT]], 1.0)
    assert rc != 0 and str(EOT) in msg
    assert _compile_rc([[5, -1]], 1.0)[0] != 0 and _compile_rc([[EOT - 1]], 1.0)[0] == 0
    for bad in (0.0, -1.0, float("nan"), float("inf"), -float("inf")):
        rc, _, msg = _compile_rc(ok, bad)
        assert rc != 0 and "boost" in msg, bad
    rc, _, msg = _compile_rc(ok, 1.0, eot=65537, v=65537)
    assert rc != 0 and "65536" in msg
    # the cap on table entries, 262144: 512 phrases [x, z_j] give node x 512 children, and each of 512 nodes [y_i, x] inherits them all through its failure link
    big = [[9, 1000 + j] for j in range(512)] + [[2000 + i, 9] for i in range(512)]
    rc, _, msg = _compile_rc(big, 1.0)
    assert rc != 0 and "262144" in msg
    assert _compile_rc(big[:-12], 1.0)[0] == 0                                     # 500 x 512 + 512 + the root's 1012
    # a buffer that is too small is refused, nothing is written past it
    tokens, lens = binding.pack_phrases(ok)
    buf = np.full(8, -7, np.int32)
    rc = binding.lib().wh_boost_compile(tokens.ctypes.data_as(C.c_void_p), lens.ctypes.data_as(C.c_void_p), 2, 2, EOT, V, 1.0, buf.ctypes.data_as(C.c_void_p), 4, C.byref(n))
    assert rc != 0 and (buf == -7).all()
    # the host step refuses tables that are not a compiler's and a state that is no node
    tables = binding.boost_compile(ok, EOT, V, 1.0)
    with pytest.raises(binding.WhisperHipError):
        binding.boost_step_host(tables[:-1], 0, 5, 0, np.zeros(V, np.float32), EOT)
    with pytest.raises(binding.WhisperHipError):
        binding.boost_step_host(tables, int(tables[0]), 5, 0, np.zeros(V, np.float32), EOT)


# ---------------------------------------------------------------------------------------------------------------------
# the scheduler over the test double
# ---------------------------------------------------------------------------------------------------------------------
import json  # noqa: E402
import os  # noqa: E402
import shutil  # noqa: E402
import subprocess  # noqa: E402

import test_hostloop_cpu as H  # noqa: E402
from test_batch_cpu import StreamDesc, recordings  # noqa: E402
from whisper_amd import ggml_format as gf  # noqa: E402

ROOT = H.ROOT
HOST = os.path.join(ROOT, "whisper_amd", "host")
LIB = os.path.join(H.BUILD, "libphrase_boost_cpu.so")
SOURCES = [os.path.join(ROOT, "tests", "phrase_boost_cpu", "batch_driver.cpp")] + [os.path.join(HOST, f) for f in ("batchScheduler.cpp", "support.cpp", "tokenTimestamps.cpp")]
DEPS = SOURCES + [os.path.join(HOST, f) for f in os.listdir(HOST) if f.endswith(".h")] + [os.path.join(ROOT, "include", h) for h in ("whisperApi.h", "whisper_hip.h")] + \
       [os.path.join(ROOT, "tests", "hostloop_cpu", f) for f in ("fake_device.cpp", "batch_driver.cpp")]
INCLUDES = ["-I" + os.path.join(ROOT, "include"), "-I" + HOST]
E_POINTER, E_INVALIDARG, E_NOTIMPL, E_BOUNDS = 0x80004003, 0x80070057, 0x80004001, 0x8000000B
SET_A, SET_B = dict(count=2, first=1000, boost=2.5), dict(count=1, first=1003, boost=4.0)
CLEARED = dict(count=0, first=-1, boost=0.0)


@pytest.fixture(scope="module")
def lib():
    """whisper_amd/host/batchScheduler.cpp compiled UNCHANGED next to the unchanged test double of the compute layer and tests/phrase_boost_cpu/batch_driver.cpp"""
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
    L.pb_run.argtypes = run_args + [C.POINTER(C.c_int32), C.c_int]
    L.bt_result.restype = C.c_char_p
    L.pb_result.restype = C.c_char_p
    L.pb_install_hook(1)
    return L


@pytest.fixture(scope="module")
def model_path(tmp_path_factory):
    model = gf.conditioned_model(gf.conditioned_layout(gf.hparams_for("test-d128-ml")), 4, kind="test-d128-ml", seed=10)
    path = str(tmp_path_factory.mktemp("boost") / "m.bin")
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
    hr = L.pb_run(*common, a, len(script))
    return hr, json.loads(L.pb_result().decode())


def transcripts(res):
    return [(st["hr"], [(s["t0"], s["t1"], s["text"], s["tokens"]) for s in st["segments"]]) for st in res["streams"]]


def told(c):
    return dict(count=c["count"], first=c["first"], boost=c["boost"])


@pytest.mark.parametrize("slots,groups", [(1, 1), (2, 1), (5, 1), (2, 2), (5, 2)])
def test_every_group_is_told_once_per_change(lib, model_path, slots, groups):
    """1 / 2 / 5 slots, 1 / 2 groups, five runs of one runner: set A before run 0, nothing before run 1, cleared before run 2, A twice before run 3, B before
    run 4. Every group's context hears each change exactly once -- the whole set and its boost -- before it started a window of that run; run 1 tells nobody.
    The recording hook boosts nothing: the transcripts are those of the unchanged harness."""
    hr0, plain = run(lib, model_path, slots, groups, plain=True)
    hr, res = run(lib, model_path, slots, groups, script=[1, -1, 0, 3, 4])
    assert hr0 == 0 and hr == 0 and transcripts(res) == transcripts(plain) and sum(len(s["segments"]) for s in plain["streams"]) >= 6
    calls = res["calls"]
    used = res["counters"][0] - 1                                                # the groups' contexts alive at the end, without the loader
    assert used == min(groups, len(STREAMS) // 2)
    by_run = {r: [c for c in calls if c["run"] == r] for r in range(5)}
    assert by_run[1] == [] and len(calls) == 4 * used
    starts = {}
    for r, want in ((0, SET_A), (2, CLEARED), (3, SET_A), (4, SET_B)):
        assert sorted(c["context"] for c in by_run[r]) == list(range(used)) and all(told(c) == want for c in by_run[r]), (r, by_run[r])
        for c in by_run[r]:
            # told before the context's first window of that run: its count of window starts is what the run before left
            assert c["starts"] >= starts.get(c["context"], 0) and (r > 0 or c["starts"] == 0), c
            starts[c["context"]] = c["starts"]
    assert all(c["starts"] > 0 for c in by_run[2])                               # ... and the earlier runs did start windows


def test_never_set_cleared_and_no_hook(lib, model_path):
    """Never set, only ever cleared (by nullptr or by a count of 0), or set and cleared again before a run: no context is given a set. Without the hook setting
    phrases is E_NOTIMPL and clearing S_OK. An id equal to eot is E_INVALIDARG. Results: the unchanged harness's, every time."""
    hr0, plain = run(lib, model_path, 2, 2, plain=True)
    assert hr0 == 0
    for script in ([-1], [0], [5], [0, 5]):
        hr, res = run(lib, model_path, 2, 2, script=script)
        assert hr == 0 and transcripts(res) == transcripts(plain) and res["calls"] == [], script
    for script in ([2], [0, 2]):
        # set and cleared again is two changes: a group hears the state it must be in, no set, once
        hr, res = run(lib, model_path, 2, 2, script=script)
        assert hr == 0 and transcripts(res) == transcripts(plain) and res["calls"] and all(told(c) == CLEARED for c in res["calls"]), script
    hr, res = run(lib, model_path, 2, 2, script=[6])
    assert hr & 0xFFFFFFFF == E_INVALIDARG and res == {}
    lib.pb_install_hook(0)
    try:
        for script in ([1], [-1, 1], [3], [4]):
            hr, res = run(lib, model_path, 2, 2, script=script)
            assert hr & 0xFFFFFFFF == E_NOTIMPL and res == {}, script
        for script in ([-1], [0], [0, 5]):
            hr, res = run(lib, model_path, 2, 2, script=script)
            assert hr == 0 and res["calls"] == [] and transcripts(res) == transcripts(plain), script
    finally:
        lib.pb_install_hook(1)


# ---------------------------------------------------------------------------------------------------------------------
# phraseSpellings, flat C, Python, tools: what needs no device
# ---------------------------------------------------------------------------------------------------------------------
def _spellings(path, text, cap=2):
    from whisper_amd import api
    tokens, lens, n = np.zeros((max(cap, 1), 16), np.int32), np.zeros(max(cap, 1), np.int32), C.c_uint32(0)
    hr = api.lib().whisperc_debug_phrase_spellings(path.encode(), text.encode("utf-8"), tokens.ctypes.data_as(C.c_void_p), lens.ctypes.data_as(C.c_void_p), cap, C.byref(n))
    return hr & 0xFFFFFFFF, [[int(t) for t in tokens[r, :lens[r]]] for r in range(min(n.value, cap))]


def test_phrase_spellings_on_a_synthetic_vocabulary(model_path, capfd):
    """Whisper::phraseSpellings on the vocabulary of a synthetic model file: the text as written and the text behind one space, each what the tokenizer gives;
    a text that begins with a space gives one row; spellings that come out equal collapse; an over-long phrase is refused, and the log names it."""
    from whisper_amd import api
    L = api.lib()

    def tokenize(text):
        buf = (C.c_int32 * 4096)()
        n = L.whisperc_debug_tokenize(model_path.encode(), text.encode("utf-8"), buf, 4096)
        assert n >= 0
        return list(buf[:n])

    word = next(w for w in ("hello", "the", "a", "Hello", "b") if tokenize(w) and tokenize(" " + w) and tokenize(w) != tokenize(" " + w))
    hr, rows = _spellings(model_path, word)
    assert hr == 0 and rows == [tokenize(word), tokenize(" " + word)]
    hr, rows = _spellings(model_path, " " + word)
    assert hr == 0 and rows == [tokenize(" " + word)]                            # the leading-space case gives no duplicate
    hr, rows = _spellings(model_path, word, cap=1)
    assert hr == E_BOUNDS
    long_text = " ".join([word] * 40)
    assert len(tokenize(long_text)) > 16
    capfd.readouterr()
    hr, rows = _spellings(model_path, long_text)
    log = capfd.readouterr().err
    assert hr == E_INVALIDARG and rows == []
    assert "phraseSpellings" in log and '"%s"' % long_text in log and "%d tokens" % len(tokenize(long_text)) in log, log
    hr, rows = _spellings(model_path, "")
    log = capfd.readouterr().err
    assert hr == E_INVALIDARG and rows == [] and "phraseSpellings" in log and 'the phrase ""' in log and "0 tokens" in log, log
    assert L.whisperc_phrase_spellings(None, b"x", None, None, 0, None) & 0xFFFFFFFF == E_POINTER


def test_flat_c_argument_checks_and_exports():
    from whisper_amd import api
    L = api.lib()
    assert L.whisperc_set_boost_phrases(None, None, None, 0, 0, 1.0) & 0xFFFFFFFF == E_POINTER
    assert L.whisperc_batch_set_boost_phrases(None, None, None, 0, 0, 1.0) & 0xFFFFFFFF == E_POINTER
    for name in ("wh_context_set_boost", "wh_boost_compile", "wh_boost_step_host", "wh_op_boost_logits"):
        assert name in binding.EXPORTS
    assert callable(api.Context.set_boost_phrases) and callable(api.BatchRunner.set_boost_phrases) and callable(api.Model.phrase_spellings)
    assert callable(binding.HipContext.set_boost)
    # the compute layer's own argument checks come before any device call
    H_ = binding.lib()
    assert H_.wh_context_set_boost(None, None, None, 0, 0, 1.0) != 0
    assert H_.wh_op_boost_logits(None, None, 1, 8, 2, None, 8, None, 1, None) != 0


def test_the_tools_take_the_options(tmp_path):
    """whisper-main: --boost-phrases FILE --boost N are parsed out before the reference's parser sees the line, so --dump-options and the usage text stay the
    reference's; either without the other is an error. whisper-mgpu: the pair parses (the line then fails for its missing -m and -f, not with the usage text
    an unknown option gets), one alone is refused."""
    from whisper_amd import build
    if not os.path.exists(build.CLI_BIN) or not os.path.exists(build.MGPU_BIN):
        build.build_all()
    phrases = str(tmp_path / "phrases.txt")
    with open(phrases, "w", encoding="utf-8") as f:
        f.write("hello\n\n world \n")
    run_main = lambda *a: subprocess.run([build.CLI_BIN] + list(a), stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=60)
    plain = run_main("--dump-options", "-f", "a.wav")
    with_it = run_main("--dump-options", "--boost-phrases", phrases, "--boost", "3.5", "-f", "a.wav")
    assert plain.returncode == 0 and with_it.returncode == 0 and with_it.stdout == plain.stdout and "a.wav" in plain.stdout
    for alone in (("--boost-phrases", phrases), ("--boost", "3.5")):
        r = run_main("--dump-options", *alone, "-f", "a.wav")
        assert r.returncode == 2 and "go together" in r.stderr, alone
    usage = run_main("-h")
    assert "boost" not in usage.stdout + usage.stderr
    run_mgpu = lambda *a: subprocess.run([build.MGPU_BIN] + list(a), stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=60)
    r = run_mgpu("-boost-phrases", phrases, "-boost", "3.5")
    assert r.returncode == 1 and "-m and -f are required" in r.stderr and "usage:" not in r.stderr
    for alone in (("-boost-phrases", phrases), ("-boost", "3.5")):
        r = run_mgpu(*alone, "-m", "m.bin", "-f", "a.wav")
        assert r.returncode == 1 and "go together" in r.stderr, alone
    usage = run_mgpu("-tsx")
    assert usage.returncode == 1 and "usage: whisper-mgpu" in usage.stderr and "boost" not in usage.stderr
