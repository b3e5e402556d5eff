"""CPU tests of language detection (language "auto"): the host half of whisper_lang_auto_detect (whisper_amd/host/languageDetect.h) against the
reference's CPU model (oracle/_ref/libwhisper_ref.so), bit for bit, and the fixture tests/golden/ref_lang_detect.json against a live run of its
generator. No GPU: the device half (wh_lang_detect) is tests/test_gpu_lang_detect.py's."""
import ctypes
import json
import os
import sys
import tempfile

import numpy as np
import pytest

from whisper_amd import api, ggml_format as gf

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")
sys.path.insert(0, GOLDEN)
import make_golden_lang_detect as mk  # noqa: E402


@pytest.fixture(scope="module")
def fixture():
    with open(os.path.join(GOLDEN, "ref_lang_detect.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def host_lib():
    if not os.path.exists(api.HOST_LIB_PATH):
        pytest.skip("libWhisper.so not built")
    return api.lib()


def test_fixture_conditions(fixture):
    """What the generator asserts, once more on the committed file: enough cases, winners and language-sensitive transcripts, margins."""
    cases = fixture["cases"]
    assert len(cases) >= mk.MIN_KEPT
    assert len({c["winner"] for c in cases}) >= mk.MIN_WINNERS
    assert sum(1 for c in cases if c["transcript_differs_under"]) >= mk.MIN_SENSITIVE
    for c in cases:
        assert c["lang_logit_margin"] >= mk.MIN_MARGIN and c["min_logit_margin"] >= mk.MIN_MARGIN, c["name"]
        p = mk.from_bits(c["p_bits"])
        assert len(p) == 99 and int(np.argmax(p)) == c["winner_id"] and mk.LANG_CODES[c["winner_id"]] == c["winner"]


def test_host_half_reproduces_the_reference_bit_for_bit(fixture, host_lib):
    """finishLanguageProbs (sort descending, exp in double, the running sum in single precision, scatter) fed with the reference's own p gives the reference's
    lang_probs bit for bit and its winner, on every case of the fixture. This is what settles which exp() the reference's unqualified exp( float )
    is under its build flags: the double one (the single-precision overload fails this test)."""
    for c in fixture["cases"]:
        p, want = mk.from_bits(c["p_bits"]), mk.from_bits(c["lang_probs_bits"])
        best, got = api.finish_language_probs(p)
        assert best == c["winner_id"], c["name"]
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (c["name"], float(np.abs(got - want).max()))
        assert abs(float(got.sum()) - 1.0) < 1e-5


def test_host_half_against_a_live_reference_run(host_lib, ref_lib_available, tmp_path):
    """The same on a fresh run of the reference (a seed and recordings of its own, 1 and 3 threads, offsets 0 and 12 s), and the error codes of a
    bad offset."""
    if not ref_lib_available:
        pytest.skip("oracle/_ref/libwhisper_ref.so not present")
    from oracle import ref
    path = str(tmp_path / "m.bin")
    gf.write_model(path, mk.model_for(31))
    for rec, nt, off in (("jfk", 1, 0), ("mixed", 3, 0), ("mixed", 3, 12000)):
        w = ref.RefWhisper(path, n_threads=nt, log_level=0)
        w.pcm_to_mel(mk.pcm_for(rec))
        winner, p, want, _ = mk.detect(w, off)
        assert winner >= 0
        best, got = api.finish_language_probs(p)
        assert best == winner and np.array_equal(got.view(np.uint32), want.view(np.uint32)), (rec, nt, off)
        assert mk.detect(w, -10)[0] == -1 and mk.detect(w, 10 * w.L.ref_mel_len(w.ctx))[0] == -2
        w.close()


def test_auto_is_a_language_key(host_lib):
    """findLanguageKeyA( "auto" ) is makeLanguageKey( "auto" ) (it fits the uint32); the table of languages is unchanged."""
    f = getattr(ctypes.CDLL(api.HOST_LIB_PATH), "_ZN7Whisper16findLanguageKeyAEPKc")
    f.restype = ctypes.c_uint32
    f.argtypes = [ctypes.c_char_p]
    assert f(b"auto") == int.from_bytes(b"auto", "little") == 0x6F747561 and f(b"AUTO") == 0x6F747561
    assert f(b"en") == 0x6E65 and f(b"xx") == 0xFFFFFFFF and f(b"aut") == 0xFFFFFFFF
    codes = api.language_codes()
    assert len(codes) == 99 and codes[:7] == list(mk.LANG_CODES) and "auto" not in codes


def test_fixture_is_current(fixture, ref_lib_available):
    """Regenerating one case live gives the committed record (the model generator, the recordings and the reference have not moved)."""
    if not ref_lib_available:
        pytest.skip("oracle/_ref/libwhisper_ref.so not present")
    assert fixture["self_out_scale"] == mk.SELF_OUT_SCALE and fixture["kind"] == mk.KIND
    c = fixture["cases"][0]
    live, why = mk.make_case(c["seed"], c["pcm"], verbose=False)
    assert live is not None, why
    assert json.loads(json.dumps(live)) == c


# ---------------------------------------------------------------------------------------------------------------------
# the lock-step batch scheduler with language "auto": every stream its own language
# ---------------------------------------------------------------------------------------------------------------------
import ctypes as C  # noqa: E402
import shutil  # noqa: E402
import subprocess  # noqa: E402

ROOT = os.path.dirname(HERE)
BUILD = os.path.join(HERE, "_build")
REF_DIR = os.path.join(ROOT, "oracle", "_ref")
BATCH_LANG_LIB = os.path.join(BUILD, "libbatch_lang_cpu.so")
BATCH_LANG_SOURCES = [os.path.join(HERE, "hostloop_cpu", "batch_lang_driver.cpp")] + \
                     [os.path.join(ROOT, "whisper_amd", "host", f) for f in ("batchScheduler.cpp", "support.cpp", "tokenTimestamps.cpp")]
FLAG_NO_CONTEXT = 2


class StreamDesc(C.Structure):
    _fields_ = [("buffer", C.c_int32), ("firstSample", C.c_int64), ("countSamples", C.c_int64)]


@pytest.fixture(scope="module")
def batch_lang_lib():
    """batchScheduler.cpp + the test double of the compute layer (tests/hostloop_cpu/fake_device.cpp, unchanged, included by the new source) + a detector
    played by the double's per-slot reference models, injected the way libWhisper.so injects wh_lang_detect. Linked with --no-undefined like
    tests/test_batch_cpu.py's library: the scheduler holds no reference to the compute layer's detection entry."""
    if not os.path.exists(os.path.join(REF_DIR, "libwhisper_ref.so")):
        pytest.skip("oracle/_ref/libwhisper_ref.so not built (needs /root/reference)")
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    os.makedirs(BUILD, exist_ok=True)
    hdr = [os.path.join(ROOT, "whisper_amd", "host", f) for f in os.listdir(os.path.join(ROOT, "whisper_amd", "host")) if f.endswith(".h")]
    deps = BATCH_LANG_SOURCES + hdr + [os.path.join(HERE, "hostloop_cpu", f) for f in ("fake_device.cpp", "batch_driver.cpp")] + [os.path.join(REF_DIR, "libwhisper_ref.so")]
    if not os.path.exists(BATCH_LANG_LIB) or any(os.path.getmtime(d) > os.path.getmtime(BATCH_LANG_LIB) for d in deps):
        cmd = ["g++", "-std=c++17", "-O1", "-fPIC", "-shared", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "whisper_amd", "host"),
               "-I" + os.path.join(HERE, "hostloop_cpu")] + BATCH_LANG_SOURCES + \
              ["-o", BATCH_LANG_LIB, "-L" + REF_DIR, "-lwhisper_ref", "-Wl,-rpath," + REF_DIR, "-Wl,-Bsymbolic", "-Wl,--no-undefined", "-lpthread"]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        assert r.returncode == 0, r.stdout
    L = C.CDLL(BATCH_LANG_LIB)
    L.bl_run.argtypes = [C.c_char_p, C.c_int, C.c_uint32, C.c_uint32, C.c_int, C.POINTER(C.c_int32), C.c_int, C.POINTER(C.POINTER(C.c_float)), C.POINTER(C.c_int32),
                         C.c_int, C.POINTER(StreamDesc), C.c_int, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int]
    L.bl_result.restype = C.c_char_p
    return L


def _run_batch(L, path, buffers, streams, slots, groups, lang="auto"):
    bufs = [np.ascontiguousarray(b, np.float32) for b in buffers]
    ptrs = (C.POINTER(C.c_float) * len(bufs))(*[b.ctypes.data_as(C.POINTER(C.c_float)) for b in bufs])
    lens = (C.c_int32 * len(bufs))(*[len(b) for b in bufs])
    descs = (StreamDesc * len(streams))(*[StreamDesc(b, f, n) for (b, f, n) in streams])
    pt = (C.c_int32 * 1)(1000)
    key = int.from_bytes(lang.encode(), "little")
    hr = L.bl_run(path.encode(), 0, FLAG_NO_CONTEXT, key, 0, C.cast(pt, C.POINTER(C.c_int32)), 1, ptrs, lens, len(bufs), descs, len(streams), slots, groups, 4, 0, 4)
    return hr, json.loads(L.bl_result().decode())


def test_batch_scheduler_gives_every_stream_its_own_language(batch_lang_lib, tmp_path):
    """Streams of different winners in one lock-step batch -- whole recordings, two pieces of a buffer (firstSample > 0: a piece is detected on ITS OWN
    first frame) and one of half a second -- with language "auto" and with key 0: every stream's language and transcript are those of that stream run
    ALONE through the reference's whisper_full( "auto" ) at the double's thread count, whatever maxSlots (1, 2, 5, 64), the number of groups and the
    order of the streams. One detection pre-pass per admission wave, not per stream. Without an injected detector "auto" is E_NOTIMPL per stream."""
    from oracle import ref
    L = batch_lang_lib
    path = str(tmp_path / "m.bin")
    gf.write_model(path, mk.model_for(10))
    bufs = [mk.pcm_for("jfk"), mk.pcm_for("quiet"), mk.pcm_for("mixed")]
    streams = [(0, 0, 0), (1, 0, 0), (2, 0, 0), (2, 16000 * 12, 0), (1, 16000 * 9, 16000 * 14), (0, 0, 8000)]
    want = []
    w = ref.RefWhisper(path, n_threads=4, log_level=0)
    for b, first, count in streams:
        pcm = bufs[b][first:first + count] if count else bufs[b][first:]
        if len(pcm) < 16000:
            want.append((1, -1, []))                                               # S_FALSE, nothing detected, nothing transcribed
            continue
        w.pcm_to_mel(pcm)
        winner = mk.detect(w)[0]
        shift = first * 10000000 // 16000
        want.append((0, winner, [(s["t0"] * 100000 + shift, s["t1"] * 100000 + shift, s["tokens"]) for s in mk.full(w, pcm, "auto")]))
    w.close()
    assert len({x[1] for x in want if x[1] >= 0}) >= 2, "the streams of this test must differ in language"
    assert want[3][1] >= 0 and sum(len(x[2]) for x in want) >= 8
    counters = (C.c_int32 * 2)()
    for slots, groups, order, lang in ((1, 1, 1, "auto"), (2, 2, -1, "auto"), (5, 1, 1, ""), (64, 2, -1, "auto")):
        idx = list(range(len(streams)))[::order]
        L.bl_detect_counters(counters)
        calls0 = counters[0]
        hr, got = _run_batch(L, path, bufs, [streams[i] for i in idx], slots, groups, lang)
        assert hr == 0, (slots, groups, hr)
        for st, i in zip(got["streams"], idx):
            assert st["hr"] == want[i][0] and st["lang"] == want[i][1], (slots, groups, i, st["hr"], st["lang"], want[i][:2])
            assert [(s["t0"], s["t1"], s["tokens"]) for s in st["segments"]] == want[i][2], (slots, groups, i)
            assert (0.0 < st["p"] < 1.0) == (want[i][1] >= 0)
        L.bl_detect_counters(counters)
        if slots == 64:
            assert counters[0] - calls0 <= groups, "one pre-pass per group when every stream has a slot"
    # a named language in the same library: nothing detected
    hr, got = _run_batch(L, path, bufs, streams[:2], 2, 1, "en")
    assert hr == 0 and all(st["lang"] == -1 for st in got["streams"])
    # no detector injected: E_NOTIMPL for the streams that would need it, S_FALSE as ever for the one that is too short
    L.bl_install_detector(0)
    try:
        hr, got = _run_batch(L, path, bufs, [streams[0], streams[5]], 2, 1, "auto")
    finally:
        L.bl_install_detector(1)
    assert hr & 0xFFFFFFFF == 0x80004001 and got["streams"][0]["hr"] & 0xFFFFFFFF == 0x80004001 and got["streams"][1]["hr"] == 1
