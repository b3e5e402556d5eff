"""CPU test of stereo diarization in the lock-step batch scheduler (whisper_amd/host/batchScheduler.cpp over the test double of the compute layer,
tests/hostloop_cpu/fake_device.cpp): the speakers a stream's result carries, and what the stream's context answers iContext::detectSpeaker from the
new_segment callback, against the restatement of the reference's rule in tests/test_diarize_cpu.py. No GPU."""
import ctypes as C
import json
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

from whisper_amd import ggml_format as gf

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))
import make_golden_lang_detect as mk  # noqa: E402
from test_diarize_cpu import LEFT, NO_STEREO_DATA, RIGHT, speakers_of  # noqa: E402

BUILD = os.path.join(HERE, "_build")
REF_DIR = os.path.join(ROOT, "oracle", "_ref")
LIB = os.path.join(BUILD, "libbatch_diarize_cpu.so")
SOURCES = [os.path.join(HERE, "hostloop_cpu", "batch_diarize_driver.cpp")] + \
          [os.path.join(ROOT, "whisper_amd", "host", f) for f in ("batchScheduler.cpp", "support.cpp", "tokenTimestamps.cpp")]
FLAG_NO_CONTEXT = 2


class StreamDesc(C.Structure):
    _fields_ = [("buffer", C.c_int32), ("firstSample", C.c_int64), ("countSamples", C.c_int64)]


@pytest.fixture(scope="module")
def batch_lib():
    """Linked with --no-undefined like the scheduler's other CPU libraries: diarize.h refers to nothing of the compute layer."""
    if not os.path.exists(os.path.join(REF_DIR, "libwhisper_ref.so")):
        pytest.skip("oracle/_ref/libwhisper_ref.so not built")
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
    fpp = C.POINTER(C.POINTER(C.c_float))
    L.bd_run.argtypes = [C.c_char_p, C.c_uint32, C.c_uint32, fpp, fpp, C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.c_int, C.POINTER(StreamDesc), C.c_int,
                         C.c_uint32, C.c_uint32, C.c_int]
    L.bd_result.restype = C.c_char_p
    return L


def run_batch(L, path, buffers, stereo, times, streams, slots, groups):
    fp = C.POINTER(C.c_float)
    bufs = [np.ascontiguousarray(b, np.float32) for b in buffers]
    sts = [None if s is None else np.ascontiguousarray(s, np.float32) for s in stereo]
    ptrs = (fp * len(bufs))(*[b.ctypes.data_as(fp) for b in bufs])
    st_ptrs = (fp * len(bufs))(*[C.cast(None, fp) if s is None else s.ctypes.data_as(fp) for s in sts])
    lens = (C.c_int32 * len(bufs))(*[len(b) for b in bufs])
    tm = (C.c_int64 * len(bufs))(*times)
    descs = (StreamDesc * len(streams))(*[StreamDesc(b, f, n) for (b, f, n) in streams])
    hr = L.bd_run(path.encode(), FLAG_NO_CONTEXT, int.from_bytes(b"en", "little"), ptrs, st_ptrs, tm, lens, len(bufs), descs, len(streams), slots, groups, 4)
    return hr, json.loads(L.bd_result().decode())


def alternating(n, seed, period):
    """Stereo noise whose loud channel changes every `period` samples: left, right, both, left ..."""
    rng = np.random.default_rng(seed)
    st = (0.1 * rng.standard_normal((n, 2))).astype(np.float32)
    which = (np.arange(n) // period) % 3
    st[which == 0, 1] *= 0.25
    st[which == 1, 0] *= 0.25
    return st


def test_batch_streams_carry_their_speakers(batch_lib, tmp_path):
    """Four streams in one lock-step batch: a recording with stereo data whose left channel is louder; a piece of a larger stereo buffer (firstSample > 0,
    a media time of 3.6 s on the buffer) whose right channel is louder inside the piece and whose left channel is louder before it; a mono recording.
    The fourth, another stereo piece, has a loud channel that alternates every 1.7 s, so that its segments differ. The speakers of every stream's result are the
    restatement's on the stream's own segment times and its own piece of the stereo data; the mono stream reports 0xFF for every segment; the answers
    of iContext::detectSpeaker in the new_segment callbacks are the results' (speaker_faults). Whatever the number of slots and groups."""
    L = batch_lib
    path = str(tmp_path / "m.bin")
    gf.write_model(path, mk.model_for(10))
    bufs = [mk.pcm_for("jfk"), mk.pcm_for("mixed"), mk.pcm_for("quiet")]
    first, count = 16000 * 12, 16000 * 11
    rng = np.random.default_rng(5)
    st0 = (rng.standard_normal((len(bufs[0]), 2)) * np.array([0.2, 0.05])).astype(np.float32)
    st1 = (rng.standard_normal((len(bufs[1]), 2)) * np.array([0.2, 0.05])).astype(np.float32)
    st1[first:] = st1[first:, ::-1]
    st_alt = alternating(len(bufs[1]), 9, 27200)
    times = [0, 36_000_000, 0, 0]
    # buffer 3 = buffer 1's mono beside the alternating stereo
    buffers, stereo = bufs + [bufs[1]], [st0, st1, None, st_alt]
    streams = [(0, 0, 0), (1, first, count), (2, 0, 0), (3, 16000 * 3, 0)]
    seen = None
    for slots, groups in ((2, 2), (64, 1)):
        hr, got = run_batch(L, path, buffers, stereo, times, streams, slots, groups)
        assert hr == 0 and got["speaker_faults"] == 0, (slots, groups, hr, got["speaker_faults"])
        want = []
        for (b, f, n), st in zip(streams, got["streams"]):
            assert st["hr"] == 0 and len(st["segments"]) >= 2, (b, st["hr"], len(st["segments"]))
            piece = None if stereo[b] is None else (stereo[b][f:f + n] if n else stereo[b][f:])
            want.append(speakers_of(st["segments"], piece, times[b] + f * 10_000_000 // 16000))
            assert st["speakers"] == want[-1], (slots, groups, b, st["speakers"], want[-1])
        assert got["speaker_calls"] == sum(len(st["segments"]) for st in got["streams"])
        assert set(want[0]) == {LEFT} and set(want[1]) == {RIGHT} and set(want[2]) == {NO_STEREO_DATA} and len(set(want[3])) >= 2, want
        # the piece's speakers depend on where its stereo data starts: the buffer's first samples instead of the piece's give other answers
        s1 = got["streams"][1]["segments"]
        assert speakers_of(s1, stereo[1][:count], times[1] + first * 10_000_000 // 16000) != want[1]
        assert seen is None or seen == want, "the speakers do not depend on slots and groups"
        seen = want
