"""CPU tests of suppressed tokens ("Suppressed tokens"):

  * the non-speech set builder (whisper_amd/host/nonSpeechTokens.h) against a restatement of its rule written here, on synthetic vocabularies with planted
    strings, multilingual and .en; the header's stand-alone driver (tests/suppress_cpu/driver.cpp) compiled alone, plain and under
    -fsanitize=address,undefined; Whisper::getNonSpeechTokens on a model file's vocabulary, with its capacity rules;
  * the lock-step scheduler: whisper_amd/host/batchScheduler.cpp compiled UNCHANGED next to the unchanged test double of the compute layer and
    tests/suppress_cpu/batch_driver.cpp, whose injected hook (batchSuppress.h) records every call. The hook filters nothing, so the transcripts must be those
    of a runner on which nothing was set: what is tested is who is told what, and when;
  * argument checks of the flat C and Python layers that need no device, and the tools' option parsing.
The GPU twin: tests/test_gpu_suppress.py."""
import ctypes as C
import json
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import test_hostloop_cpu as H
from test_batch_cpu import StreamDesc, recordings
from whisper_amd import ggml_format as gf

ROOT = H.ROOT
HOST = os.path.join(ROOT, "whisper_amd", "host")
HEADER = os.path.join(HOST, "nonSpeechTokens.h")
DRIVER = os.path.join(ROOT, "tests", "suppress_cpu", "driver.cpp")
LIB = os.path.join(H.BUILD, "libsuppress_cpu.so")
SOURCES = [os.path.join(ROOT, "tests", "suppress_cpu", "batch_driver.cpp")] + [os.path.join(HOST, f) for f in ("batchScheduler.cpp", "support.cpp", "tokenTimestamps.cpp")]
DEPS = SOURCES + [os.path.join(HOST, f) for f in os.listdir(HOST) if f.endswith(".h")] + [os.path.join(ROOT, "include", h) for h in ("whisperApi.h", "whisper_hip.h")] + \
       [os.path.join(ROOT, "tests", "hostloop_cpu", f) for f in ("fake_device.cpp", "batch_driver.cpp")]
INCLUDES = ["-I" + os.path.join(ROOT, "include"), "-I" + HOST]
E_POINTER, E_INVALIDARG, E_NOTIMPL, E_BOUNDS = 0x80004003, 0x80070057, 0x80004001, 0x8000000B

# ---------------------------------------------------------------------------------------------------------------------
# the rule, restated: the 54 symbols of the issue, as UTF-8
# ---------------------------------------------------------------------------------------------------------------------
SYMBOLS = ('" # ( ) * + / : ; < = > @ [ \\ ] ^ _ ` { | } ~ 「 」 『 』 '
           '<< >> <<< >>> -- --- -( -[ (\' (" (( )) ((( ))) [[ ]] {{ }} ♪♪ ♪♪♪ '
           '♩ ♪ ♫ ♬ ♭ ♮ ♯').split()


def expected(words, eot):
    """Every id < eot whose stored text is a symbol or a blank and a symbol, or " -" or " '"; ascending."""
    wanted = {s.encode() for s in SYMBOLS} | {b" " + s.encode() for s in SYMBOLS} | {b" -", b" '"}
    return [i for i, w in enumerate(words[:eot]) if w in wanted]


def planted_vocabulary(kind):
    """default_vocab_words (its 256 single-byte words kept: '(' is id 40 ...) with strings planted among the " w<id>" words. Returns (hparams, words, eot, the
    planted ids that must be found)."""
    hp = gf.hparams_for(kind)
    words = list(gf.default_vocab_words(hp))
    eot = gf.special_tokens(hp)["eot"]
    assert len(SYMBOLS) == 54
    hits = {300: " (", 301: "[[", 777: " ♪", 1000: " -", 1001: " '", 20000: "♪♪♪", 20001: " ♪♪♪", 31000: "((", 31001: "((", eot - 1: " 『", 256: "}}", 40000: "\\"}
    misses = {302: "(a", 303: "  (", 304: "-", 305: "'", 306: " ' ", 307: "( ", 308: "♪♪♪♪", 309: " --- ", 310: " w(", 311: "a-", 312: " -'"}
    for i, w in {**hits, **misses}.items():
        words[i] = w.encode()
    assert len(words) == eot
    words.append(b"[[")                                                          # one more stored word, at eot itself: an id >= eot is never returned
    return hp, words, eot, sorted(hits)


def test_the_restatement_on_the_planted_vocabularies():
    for kind in ("test-d128-ml", "test-d128"):
        hp, words, eot, hits = planted_vocabulary(kind)
        want = expected(words, eot)
        assert eot == (50257 if kind.endswith("ml") else 50256)
        assert set(hits) <= set(want) and want == sorted(set(want)) and all(i < eot for i in want)
        # the single-byte words: 23 ASCII symbols; ids 302 .. 312 are near-misses
        assert [i for i in want if i < 256] == sorted(ord(s) for s in SYMBOLS if len(s) == 1 and ord(s) < 128) and len([i for i in want if i < 256]) == 23
        assert not set(range(302, 313)) & set(want) and len(want) == 23 + len(hits)
        assert 31000 in want and 31001 in want                                   # the same string at two ids


# ---------------------------------------------------------------------------------------------------------------------
# the header alone
# ---------------------------------------------------------------------------------------------------------------------
def _build_standalone(sanitize):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    os.makedirs(H.BUILD, exist_ok=True)
    out = os.path.join(H.BUILD, "non-speech-sanitized" if sanitize else "non-speech-plain")
    if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in (DRIVER, HEADER)):
        flags = ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"] if sanitize else []
        r = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror"] + flags + ["-I" + HOST, DRIVER, "-o", out], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        assert r.returncode == 0, r.stdout
    return out


def _write_words(path, words):
    with open(path, "wb") as f:
        f.write(struct.pack("<I", len(words)))
        for w in words:
            f.write(struct.pack("<I", len(w)) + w)


@pytest.mark.parametrize("sanitize", [False, True])
def test_the_header_alone_equals_the_restatement(tmp_path, sanitize):
    """The stand-alone program over nonSpeechTokens.h and nothing else, plain and under -fsanitize=address,undefined: the restatement's ids on both vocabularies,
    nothing at eot 0, a vocabulary shorter than eot, and an empty one."""
    exe = _build_standalone(sanitize)
    for kind in ("test-d128-ml", "test-d128"):
        hp, words, eot, hits = planted_vocabulary(kind)
        path = str(tmp_path / (kind + ".vocab"))
        _write_words(path, words)
        for e in (eot, 0, 1000, len(words) + 5):
            r = subprocess.run([exe, path, str(e)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
            assert r.returncode == 0 and "ERROR: AddressSanitizer" not in r.stdout and "runtime error" not in r.stdout, r.stdout[-3000:]
            lines = r.stdout.splitlines()
            got = [int(x) for x in lines[1].split()] if len(lines) > 1 else []
            assert lines[0] == "54" and got == expected(words, e), (kind, e)
    _write_words(str(tmp_path / "empty.vocab"), [])
    r = subprocess.run([exe, str(tmp_path / "empty.vocab"), "50257"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.splitlines() == ["54", ""]


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
    L.bs_run.argtypes = run_args + [C.c_int, C.POINTER(C.c_int32), C.c_uint32, C.c_int]
    L.bt_result.restype = C.c_char_p
    L.bs_result.restype = C.c_char_p
    L.bs_non_speech.argtypes = [C.c_char_p, C.POINTER(C.c_int32), C.POINTER(C.c_uint32)]
    L.bs_set_only.argtypes = [C.c_char_p, C.POINTER(C.c_int32), C.c_uint32]
    L.bs_install_hook(1)
    return L


@pytest.fixture(scope="module")
def model_path(tmp_path_factory):
    model = gf.conditioned_model(gf.conditioned_layout(gf.hparams_for("test-d128-ml")), 4, kind="test-d128-ml", seed=10)
    path = str(tmp_path_factory.mktemp("sup") / "m.bin")
    gf.write_model(path, model)
    return path


STREAMS = [(0, 0, 0), (1, 0, 0), (2, 0, 0), (3, 0, 0), (4, 0, 0), (4, 16000 * 5, 16000 * 9)]
SET = [91, 40, 300, 40, 50256, 0]                                                # unsorted, a duplicate, eot - 1 and 0: the runner hands them on as given


def run(L, path, slots, groups, mode=0, ids=SET, n_runs=1, plain=False):
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
    a = (C.c_int32 * max(1, len(ids)))(*ids)
    hr = L.bs_run(*common, mode, a, len(ids), n_runs)
    return hr, json.loads(L.bs_result().decode())


def transcripts(res):
    return [(st["hr"], [(s["t0"], s["t1"], s["text"], s["tokens"]) for s in st["segments"]]) for st in res["streams"]]


@pytest.mark.parametrize("slots,groups", [(1, 1), (2, 1), (5, 1), (2, 2), (5, 2)])
def test_every_group_is_told_once_before_its_first_round(lib, model_path, slots, groups):
    """1 / 2 / 5 slots, 1 / 2 groups, two runs of one runner: every group's context receives the set exactly once, in the first run, before it started any
    window; the second run tells nobody again. The recording hook filters nothing: the transcripts are those of the unchanged harness."""
    hr0, plain = run(lib, model_path, slots, groups, plain=True)
    hr, res = run(lib, model_path, slots, groups, mode=1, n_runs=2)
    assert hr0 == 0 and hr == 0 and transcripts(res) == transcripts(plain) and sum(len(s["segments"]) for s in plain["streams"]) >= 6
    calls = res["calls"]
    used = res["counters"][0] - 1                                                # the groups' contexts alive at the end, without the loader
    assert used == min(groups, len(STREAMS) // 2) and len(calls) == used and sorted(c["context"] for c in calls) == list(range(used))
    for c in calls:
        assert c["run"] == 0 and c["starts"] == 0 and c["ids"] == SET, c


def test_empty_sets_and_no_hook(lib, model_path):
    """Never set, or only ever an empty set: the hook is not called. The set and then an empty one: every group hears 0 ids, or nothing. Without the hook a
    non-empty set is E_NOTIMPL and an empty one S_OK. Results: the unchanged harness's, every time."""
    hr0, plain = run(lib, model_path, 2, 2, plain=True)
    assert hr0 == 0
    for mode in (0, 3):
        hr, res = run(lib, model_path, 2, 2, mode=mode)
        assert hr == 0 and res["calls"] == [] and transcripts(res) == transcripts(plain)
    hr, res = run(lib, model_path, 2, 2, mode=2)
    assert hr == 0 and transcripts(res) == transcripts(plain) and all(c["ids"] == [] and c["starts"] == 0 for c in res["calls"]) and len(res["calls"]) in (0, 2)
    lib.bs_install_hook(0)
    try:
        hr, res = run(lib, model_path, 2, 2, mode=1)
        assert hr & 0xFFFFFFFF == E_NOTIMPL and res == {}
        for mode in (0, 3):
            hr, res = run(lib, model_path, 2, 2, mode=mode)
            assert hr == 0 and res["calls"] == [] and transcripts(res) == transcripts(plain)
    finally:
        lib.bs_install_hook(1)


def test_runner_refuses_ids_outside_the_text_tokens(lib, model_path):
    eot = gf.special_tokens(gf.hparams_for("test-d128-ml"))["eot"]
    for ids, want in (([eot - 1, 0], 0), ([eot], E_INVALIDARG), ([5, -1], E_INVALIDARG), ([51864], E_INVALIDARG), ([], 0)):
        a = (C.c_int32 * max(1, len(ids)))(*ids)
        assert lib.bs_set_only(model_path.encode(), a if ids else None, len(ids)) & 0xFFFFFFFF == want, ids
    assert lib.bs_set_only(model_path.encode(), None, 3) & 0xFFFFFFFF == E_POINTER


@pytest.mark.parametrize("kind", ["test-d128-ml", "test-d128"])
def test_get_non_speech_tokens_on_a_model_file(lib, tmp_path, kind):
    """Whisper::getNonSpeechTokens over the vocabulary a model file stores (loadVocabulary), multilingual and .en: the restatement's ids; the size without a
    buffer, E_BOUNDS for a capacity one short (as whisperc_window_stats does it), a null count."""
    hp, words, eot, hits = planted_vocabulary(kind)
    model = gf.synth_model(kind, seed=5)
    model.vocab = words
    path = str(tmp_path / "planted.bin")
    gf.write_model(path, model)
    want = expected(words, eot)
    n = C.c_uint32(0)
    assert lib.bs_non_speech(path.encode(), None, C.byref(n)) == 0 and n.value == len(want)
    out = (C.c_int32 * (len(want) + 4))()
    n = C.c_uint32(len(want) - 1)
    assert lib.bs_non_speech(path.encode(), out, C.byref(n)) & 0xFFFFFFFF == E_BOUNDS and n.value == len(want)
    n = C.c_uint32(len(want) + 4)
    assert lib.bs_non_speech(path.encode(), out, C.byref(n)) == 0 and list(out[:n.value]) == want
    assert lib.bs_non_speech(path.encode(), out, None) & 0xFFFFFFFF == E_POINTER


# ---------------------------------------------------------------------------------------------------------------------
# flat C, Python, tools: what needs no device
# ---------------------------------------------------------------------------------------------------------------------
def test_flat_c_and_python_argument_checks():
    from whisper_amd import api
    L = api.lib()
    n = C.c_uint32(0)
    assert L.whisperc_non_speech_tokens(None, None, 0, C.byref(n)) & 0xFFFFFFFF == E_POINTER
    assert L.whisperc_set_suppress_tokens(None, None, 0) & 0xFFFFFFFF == E_POINTER
    assert L.whisperc_batch_set_suppress_tokens(None, None, 0) & 0xFFFFFFFF == E_POINTER
    assert len(api._suppress_ids(None, None)) == 0 and len(api._suppress_ids(None, [])) == 0
    a = api._suppress_ids(None, [5, 3, 5])
    assert a.dtype == np.int32 and a.tolist() == [5, 3, 5]
    with pytest.raises(ValueError):
        api._suppress_ids(None, "speech")


def test_the_tools_take_the_option():
    """whisper-main: -sns / --suppress-nst are parsed out before the reference's parser sees the line, so --dump-options and the usage text stay the
    reference's. whisper-mgpu: -sns parses (the line then fails for its missing -m and -f, not with the usage text an unknown option gets)."""
    from whisper_amd import build
    if not os.path.exists(build.CLI_BIN) or not os.path.exists(build.MGPU_BIN):
        build.build_all()
    run_main = lambda *a: subprocess.run([build.CLI_BIN] + list(a), stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=60)
    plain = run_main("--dump-options", "-f", "a.wav")
    for name in ("-sns", "--suppress-nst"):
        with_it = run_main("--dump-options", name, "-f", "a.wav")
        assert plain.returncode == 0 and with_it.returncode == 0 and with_it.stdout == plain.stdout and "a.wav" in plain.stdout
    usage = run_main("-h")
    assert "-sns" not in usage.stdout + usage.stderr and "suppress" not in usage.stdout + usage.stderr
    for name in ("-sns", "--suppress-nst"):
        r = subprocess.run([build.MGPU_BIN, name], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=60)
        assert r.returncode == 1 and "-m and -f are required" in r.stderr and "usage:" not in r.stderr
    r = subprocess.run([build.MGPU_BIN, "-snx"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=60)
    assert r.returncode == 1 and "usage: whisper-mgpu" in r.stderr
