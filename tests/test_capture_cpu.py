"""CPU tests of live capture: the loop of iContext::runCapture (whisper_amd/host/captureLoop.h) and the resumable voice-activity detector (vad.h) through
a stand-alone driver (tests/capture_cpu/driver.cpp: the header alone with a main) built with the address and undefined-behaviour sanitizers, held against
the Python twin of tests/capture_ref.py AND against expectations derived by hand from the reference's text, one per branch of Capture::run
(Whisper/Whisper/ContextImpl.capture.cpp:212-288). The device half is tested in tests/test_gpu_capture.py.

Hand arithmetic used below, with the default parameters: minDuration 32000, maxDuration 48000, dropStartSilence 4000, pauseDuration 5328 samples; reads of
1600 samples; a scripted detector in which frame f of a buffer is speech when its first sample lies in a speech interval."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import capture_ref as R
import vad_ref as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = os.path.join(ROOT, "tests", "_build")
HOST = os.path.join(ROOT, "whisper_amd", "host")
REFERENCE_HEADER = "/root/reference/Whisper/API/MfStructs.h"
L, VO, T, S = R.LISTENING, R.VOICE, R.TRANSCRIBING, R.STALLED


def _compile(exe, src, extra=()):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    os.makedirs(BUILD, exist_ok=True)
    deps = [src, os.path.join(HOST, "captureLoop.h"), os.path.join(HOST, "vad.h"), os.path.join(ROOT, "include", "whisperApi.h")]
    if not os.path.exists(exe) or any(os.path.getmtime(d) > os.path.getmtime(exe) for d in deps):
        r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I" + HOST,
                            "-I" + os.path.join(ROOT, "include")] + list(extra) + [src, "-o", exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        assert r.returncode == 0, r.stdout
    return exe


@pytest.fixture(scope="module")
def driver():
    return _compile(os.path.join(BUILD, "capture-driver"), os.path.join(ROOT, "tests", "capture_cpu", "driver.cpp"))


def run_driver(exe, *args):
    r = subprocess.run([exe] + [str(a) for a in args], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    return r.stdout.splitlines()


def rle(chunks):
    """[1600, 1600, 255] -> "1600x2,255x1" """
    out = []
    for c in chunks:
        if out and out[-1][0] == c:
            out[-1][1] += 1
        else:
            out.append([c, 1])
    return ",".join("%dx%d" % (c, k) for c, k in out) or "-"


def spans(line):
    return [tuple(int(v) for v in s.split("-")) for s in line.split()[1:]]


def driver_loop(exe, chunks, params, intervals, jobs=None, cancel_at=None, worker=False):
    secs = [repr(float(np.float32(s))) for s in params.seconds]
    out = run_driver(exe, "loop", *secs, params.flags, -1 if cancel_at is None else cancel_at, rle(chunks),
                     ",".join("%d-%d" % iv for iv in intervals) or "-", ",".join(str(j) for j in jobs) if jobs else "-", *(["worker"] if worker else []))
    assert out[0].startswith("hr ") and out[1].startswith("status") and out[2].startswith("pieces") and out[3].startswith("discarded"), out
    return dict(hr=int(out[0].split()[1], 16), status=[int(v) for v in out[1].split()[1:]], pieces=spans(out[2]), discarded=spans(out[3]))


def both(exe, chunks, intervals, jobs=None, cancel_at=None, **params):
    """the driver and the twin on the same script: they must agree; returns the driver's answer"""
    p = R.Params(**params)
    got = driver_loop(exe, chunks, p, intervals, jobs, cancel_at)
    want = R.run(chunks, p, R.vad_from_intervals(intervals), jobs, cancel_at)
    assert got["hr"] == 0
    assert got["status"] == want["status"], (got["status"], want["status"])
    assert got["pieces"] == want["pieces"] and got["discarded"] == want["discarded"], (got, want)
    # status callbacks fire only on changes and carry the whole word: exactly one bit differs between neighbours, the first word is Listening
    words = [0] + got["status"]
    assert all(bin(a ^ b).count("1") == 1 for a, b in zip(words, words[1:])), got["status"]
    assert got["status"][0] == L
    return got


# ---- the branches of Capture::run, each against the twin and against hand arithmetic ---------------------------------------------------------------
def test_silence_is_dropped_and_the_start_time_moves(driver):
    """Silence only: the buffer is dropped at every read that brings it to 4000 samples or more -- 4800, after three reads -- and nothing else happens. That
    the start time moved shows when speech follows: with speech from 16000 on, three drops put the buffer's start at 14400."""
    got = both(driver, [1600] * 40, [])
    assert got["status"] == [L] and got["pieces"] == [] and got["discarded"] == []
    got = both(driver, [1600] * 60, [(16000, 200000)])
    assert got["pieces"][0] == (14400, 14400 + 48000)


def test_speech_then_a_pause_posts_at_the_first_read_that_qualifies(driver):
    """Speech in [0, 36000): the last speech frame is 140 (first sample 35840), lastVoice = 141 * 256 = 36096, and voice stops being recent when
    oldSamples > 36096 + 5328 = 41424: the read from 41600 to 43200, which is past minDuration, so it posts [0, 43200) -- and not at 32000, where the voice
    was still recent. Speech in [0, 20000): lastVoice 20224, recent until oldSamples > 25552; the read 27200 -> 28800 clears Voice but is short of
    minDuration; the read that reaches 32000 posts."""
    got = both(driver, [1600] * 40, [(0, 36000)])
    assert got["pieces"] == [(0, 43200)]
    got = both(driver, [1600] * 40, [(0, 20000)])
    assert got["pieces"] == [(0, 32000)]
    # Listening; Voice at the first read; Voice cleared at the read 27200 -> 28800; Transcribing at the post; cleared when the next pass finds the job ended
    assert got["status"] == [L, L | VO, L, L | T, L]


def test_continuous_speech_posts_at_max_duration(driver):
    got = both(driver, [1600] * 95, [(0, 10 ** 6)])
    assert got["pieces"][:3] == [(0, 48000), (48000, 96000), (96000, 144000)]
    # the tail, 8000 samples with voice, goes out at the end of the stream
    assert got["pieces"][3] == (144000, 152000) and got["discarded"] == []


def test_a_busy_job_stalls_the_loop_until_it_ends(driver):
    """Continuous speech, the first job posted in pass 29 (the 30th read) and found ended in pass 29 + 45 = 74. The second buffer is full in pass 59: the job is
    busy and the buffer is at maxDuration, so Stalled is set. Passes 60 .. 73 discard their reads -- 14 x 1600 samples from 96000 -- while the clock goes
    on. Pass 74 sees the job ended: Transcribing and Stalled fall, the waiting buffer [48000, 96000) is posted without a read, and the next piece begins
    at 96000 + 22400 = 118400."""
    got = both(driver, [1600] * 120, [(0, 10 ** 6)], jobs=[45])
    assert got["discarded"] == [(96000 + 1600 * i, 96000 + 1600 * (i + 1)) for i in range(14)]
    assert got["pieces"][:2] == [(0, 48000), (48000, 96000)] and got["pieces"][2][0] == 118400
    i = got["status"].index(L | VO | T | S)
    assert got["status"][i:i + 4] == [L | VO | T | S, L | VO | S, L | VO, L | VO | T]
    # a job that never ends by itself: everything after the stall is discarded; the end of the stream waits for it and posts the stalled buffer
    got = both(driver, [1600] * 80, [(0, 10 ** 6)], jobs=[10 ** 6])
    assert got["discarded"] == [(96000 + 1600 * i, 96000 + 1600 * (i + 1)) for i in range(20)] and got["pieces"] == [(0, 48000), (48000, 96000)]


def test_no_drop_never_discards_and_does_not_depend_on_the_job(driver):
    chunks = [1600] * 120
    base = both(driver, chunks, [(0, 10 ** 6)], flags=R.NO_DROP)
    assert base["discarded"] == [] and not any(w & S for w in base["status"])
    assert base["pieces"] == [(48000 * i, 48000 * (i + 1)) for i in range(4)]
    for jobs in ([45], [10 ** 6, 3, 10 ** 6], [1, 1, 1, 1]):
        got = both(driver, chunks, [(0, 10 ** 6)], jobs=jobs, flags=R.NO_DROP)
        assert got == base, jobs
    # the same script without the flag does stall
    assert both(driver, chunks, [(0, 10 ** 6)], jobs=[45])["discarded"]


SPEECH = [(3000, 30000), (41000, 100000), (130000, 131000), (160000, 161000)]


@pytest.mark.parametrize("chunk", [1, 255, 256, 257, 1600])
def test_chunk_sizes(driver, chunk):
    n = 170000
    chunks = [chunk] * (n // chunk) + ([n % chunk] if n % chunk else [])
    base = None
    for jobs in (None, [10 ** 6] * 8):
        got = both(driver, chunks, SPEECH, jobs=jobs, flags=R.NO_DROP)
        assert got["discarded"] == [] and len(got["pieces"]) >= 3
        edges = set(np.cumsum([0] + chunks).tolist())
        assert all(a in edges and b in edges and a < b for a, b in got["pieces"])
        assert all(p[1] <= q[0] for p, q in zip(got["pieces"], got["pieces"][1:]))
        assert base is None or got == base          # under NoDrop the pieces and the words depend on the audio and the reads only
        base = got
    # without the flag and with jobs that end at once nothing stalls either: the same pieces
    free = both(driver, chunks, SPEECH)
    assert free["pieces"] == base["pieces"] and free["discarded"] == []


def test_end_of_stream(driver):
    """With voice buffered -- speech in [0, 20000), the stream ends at 24000 -- the rest is posted and waited for; with silence buffered (3200 samples, below
    dropStartSilence, so still there) nothing is."""
    got = both(driver, [1600] * 15, [(0, 20000)])
    assert got["pieces"] == [(0, 24000)] and got["status"] == [L, L | VO, L | VO | T, L | VO]
    got = both(driver, [1600] * 2, [])
    assert got["pieces"] == [] and got["status"] == [L]
    assert both(driver, [], [])["status"] == [L]


def test_cancel_mid_stream(driver):
    got = both(driver, [1600] * 100, [(0, 10 ** 6)], cancel_at=10)
    assert got["pieces"] == [] and got["status"] == [L, L | VO]
    # cancelled while a job runs: the loop waits for it (the Transcribing bit falls) and returns S_OK
    got = both(driver, [1600] * 100, [(0, 10 ** 6)], jobs=[10 ** 6], cancel_at=35)
    assert got["pieces"] == [(0, 48000)] and got["status"][-2:] == [L | VO | T, L | VO] and got["hr"] == 0


def test_the_worker_may_clear_transcribing_itself(driver):
    """Without NoDrop the job's end is announced by whoever runs the job (Loop::workerEnded, the reference's workCallback): the bit falls then, the loop only
    collects the result -- the same words in the same order as when the loop finds the ended job itself, and no second call for the same bit. Under NoDrop
    the announcement changes nothing: the loop clears the bit where it waits."""
    for flags in (0, R.NO_DROP):
        for jobs in ([45], [3, 70, 1], None):
            p = R.Params(flags=flags)
            plain = driver_loop(driver, [1600] * 120, p, [(0, 10 ** 6)], jobs)
            announced = driver_loop(driver, [1600] * 120, p, [(0, 10 ** 6)], jobs, worker=True)
            assert announced == plain, (flags, jobs)
            assert plain["status"] == R.run([1600] * 120, p, R.vad_from_intervals([(0, 10 ** 6)]), jobs)["status"]


def test_out_of_range_silence_and_pause_durations(driver):
    """only minDuration and maxDuration are refused; the other two are converted: NaN and negative count as 0, the top is 2^30 samples"""
    got = [int(v) for v in run_driver(driver, "samples", "nan", "-1", "-inf", "1e30", "inf", "70000", "0")]
    assert got == [0, 0, 0, 2 ** 30, 2 ** 30, 2 ** 30, 0]
    # a pause duration of 0 and a silence that is dropped at once: the loop runs
    got = driver_loop(driver, [1600] * 40, R.Params(drop_start_silence=0.0, pause_duration=0.0), [(0, 20000)])
    assert got["hr"] == 0 and got["pieces"] == [(0, 32000)]


REFUSAL_SOURCES = [os.path.join(ROOT, "tests", "capture_cpu", "refusal_driver.cpp"), os.path.join(HOST, "capture.cpp"), os.path.join(HOST, "support.cpp"),
                   os.path.join(ROOT, "tests", "hostloop_cpu", "fake_device.cpp")]


def test_refusals_over_the_cpu_device_double(tmp_path):
    """iContext::runCapture's three refusals -- a null capture, a capture of another library, minDuration or maxDuration out of range -- through
    capture.cpp as it ships, over the CPU double of the compute layer and a context double: each comes with its HRESULT and its log line before any
    device entry point is called or any job is started. A stream that ends before its first chunk is S_OK, and a failure of the device layer is the call's."""
    ref_dir = os.path.join(ROOT, "oracle", "_ref")
    if not os.path.exists(os.path.join(ref_dir, "libwhisper_ref.so")):
        pytest.skip("oracle/_ref/libwhisper_ref.so not built (needs /root/reference): the CPU device double links against it")
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    os.makedirs(BUILD, exist_ok=True)
    exe = os.path.join(BUILD, "capture-refusals")
    deps = REFUSAL_SOURCES + [os.path.join(HOST, h) for h in ("captureLoop.h", "vad.h", "hostCommon.h")] + [os.path.join(ROOT, "include", "whisperApi.h")]
    if not os.path.exists(exe) or any(os.path.getmtime(d) > os.path.getmtime(exe) for d in deps):
        r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I" + HOST, "-I" + os.path.join(ROOT, "include")] +
                           REFUSAL_SOURCES + ["-o", exe, "-L" + ref_dir, "-lwhisper_ref", "-Wl,-rpath," + ref_dir, "-lpthread"], stdout=subprocess.PIPE,
                           stderr=subprocess.STDOUT, text=True)
        assert r.returncode == 0, r.stdout
    rows = {ln.split("\t")[0]: ln.split("\t")[1:] for ln in run_driver(exe)}
    E_POINTER, E_INVALIDARG, E_FAIL, S_OK = "0x80004003", "0x80070057", "0x80004005", "0x00000000"
    untouched = ["0", "0"]                       # device calls so far, runFull calls so far
    assert rows["null"][:3] == [E_POINTER] + untouched
    assert rows["foreign"][:3] == [E_INVALIDARG] + untouched and "not created by Whisper::createPcmCapture" in rows["foreign"][3]
    for name, which, value in (("min_low", "minDuration", "0.1"), ("min_high", "minDuration", "30.5"), ("max_low", "maxDuration", "0.1"),
                               ("max_high", "maxDuration", "31"), ("min_nan", "minDuration", "nan"), ("max_nan", "maxDuration", "nan")):
        assert rows[name][:3] == [E_INVALIDARG] + untouched, name
        assert "%s parameter %s is out of range" % (which, value) in rows[name][3], rows[name]
    assert rows["empty"][:3] == [S_OK] + untouched and rows["empty_again"][:3] == [S_OK] + untouched
    assert rows["device_failure"][:3] == [E_FAIL, "1", "0"] and "wh_capture_create" in rows["device_failure"][3]


def test_seconds_to_samples(driver):
    """0.333 s -> 5328, 0.03125 s -> 500; 2^-8 s is 62.5 samples and 3 * 2^-8 s is 187.5, both exact in float32: ties go to the even neighbour"""
    secs = [0.333, 0.03125, 2.0 ** -8, 3 * 2.0 ** -8, 2.0, 3.0, 0.25, 30.0, 0.125]
    got = [int(v) for v in run_driver(driver, "samples", *[repr(float(np.float32(s))) for s in secs])]
    assert got == [5328, 500, 62, 188, 32000, 48000, 4000, 480000, 2000]
    assert got == [R.samples_from_seconds(s) for s in secs]


def test_duration_ranges(driver):
    ok = lambda a, b: run_driver(driver, "validate", a, b)[0]
    assert ok(2, 3) == ok(0.125, 30) == "0x00000000"
    for a, b in ((0.1249, 3), (30.001, 3), (2, 0.1), (2, 31), ("nan", 3), (2, "nan"), (-1, 3)):
        assert ok(a, b) == "0x80070057", (a, b)
    assert R.Params(0.125, 30).valid() and not R.Params(0.1249, 3).valid() and not R.Params(2, 31).valid()
    # the loop is not entered with bad parameters
    p = R.Params(min_duration=0.1)
    assert driver_loop(driver, [1600] * 4, p, [])["hr"] == 0x80070057


# ---- the resumable detector ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["zeros_at_the_start", "zeros_in_the_middle", "speech_first", "fewer_than_30_frames"])
def test_resumable_detector_gives_decides_answer_on_any_split(driver, tmp_path, name):
    """vad::Detector fed any split of a feature array ends where vad::decide ends on the whole, frame for frame. zeros_at_the_start is the case vad.h
    describes: an all-zero first frame, whose SFM is NaN, is the minimum for ever."""
    feat = V.features(V.recordings()[name][:256 * 400])[0]
    if name == "zeros_at_the_start":
        assert np.isnan(feat[0, 2]) and feat[0, 0] == 0
    path = str(tmp_path / "feat.bin")
    feat.astype("<f4").tofile(path)
    n = len(feat)
    rng = np.random.default_rng(5)
    irregular = []
    while sum(irregular) < n:
        irregular.append(int(rng.integers(0, 40)))
    for split in ("%d" % n, "1x%d" % n, "29,1,1,%d" % n, "30,%d" % n, "7x%d" % (n // 7 + 1), ",".join(str(k) for k in irregular), "0,0,5,0,%d" % n):
        got, want, same = (int(v) for v in run_driver(driver, "vad", path, split)[0].split())
        assert got == want and same == 1, (name, split, got, want)
    assert want > 0


# ---- layouts against the reference's header -------------------------------------------------------------------------------------------------------
LAYOUT_MAIN = r"""
#include <cstdio>
#include <cstddef>
#include <cstdint>
%s
using namespace Whisper;
int main()
{
	printf( "%%zu %%zu %%zu %%zu %%zu %%zu\n", sizeof( sCaptureParams ), offsetof( sCaptureParams, minDuration ), offsetof( sCaptureParams, maxDuration ),
		offsetof( sCaptureParams, dropStartSilence ), offsetof( sCaptureParams, pauseDuration ), offsetof( sCaptureParams, flags ) );
	printf( "%%zu %%zu %%zu %%zu\n", sizeof( sCaptureCallbacks ), offsetof( sCaptureCallbacks, shouldCancel ), offsetof( sCaptureCallbacks, captureStatus ),
		offsetof( sCaptureCallbacks, pv ) );
	printf( "%%d %%d %%d %%d %%d %%zu %%zu\n", (int)eCaptureStatus::Listening, (int)eCaptureStatus::Voice, (int)eCaptureStatus::Transcribing, (int)eCaptureStatus::Stalled,
		(int)eCaptureFlags::Stereo, sizeof( eCaptureStatus ), sizeof( eCaptureFlags ) );
	const sCaptureParams d;
	printf( "%%g %%g %%g %%g %%u\n", d.minDuration, d.maxDuration, d.dropStartSilence, d.pauseDuration, d.flags );
	return 0;
}
"""


def _layout(tmp_path, name, include, flags):
    src = str(tmp_path / (name + ".cpp"))
    with open(src, "w") as f:
        f.write(LAYOUT_MAIN % include)
    exe = str(tmp_path / name)
    r = subprocess.run(["g++", "-std=c++17", "-Wno-invalid-offsetof"] + flags + [src, "-o", exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    return subprocess.run([exe], stdout=subprocess.PIPE, text=True, check=True).stdout


def test_structures_against_the_reference_header(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    ours = _layout(tmp_path, "ours", '#include "whisperApi.h"', ["-I" + os.path.join(ROOT, "include")])
    assert ours.splitlines()[0] == "20 0 4 8 12 16" and ours.splitlines()[2].startswith("1 2 4 128 1 1 4") and ours.splitlines()[3] == "2 3 0.25 0.333 0"
    if not os.path.exists(REFERENCE_HEADER):
        pytest.skip("the reference tree is not on this machine")
    ref = _layout(tmp_path, "ref", 'typedef int32_t HRESULT;\n#include "%s"' % REFERENCE_HEADER, ["-D__stdcall="])
    assert ours == ref


# ---- the faces ---------------------------------------------------------------------------------------------------------------------------------------------
def test_declarations_and_exports():
    from whisper_amd import api, binding, build
    if not os.path.exists(api.HOST_LIB_PATH):
        build.build_all()
    out = subprocess.run(["nm", "-D", "--defined-only", "-C", api.HOST_LIB_PATH], stdout=subprocess.PIPE, text=True, check=True).stdout
    assert "Whisper::createPcmCapture(" in out
    header = open(os.path.join(ROOT, "include", "whisper_c.h")).read()
    lib = ctypes.CDLL(api.HOST_LIB_PATH)
    for name in ("whisperc_capture_create", "whisperc_capture_write", "whisperc_capture_close", "whisperc_capture_destroy", "whisperc_run_capture"):
        assert re.search(r"\b%s\s*\(" % name, header) and hasattr(lib, name), name
    hip = open(os.path.join(ROOT, "include", "whisper_hip.h")).read()
    dev = subprocess.run(["nm", "-D", "--defined-only", binding.LIB_PATH], stdout=subprocess.PIPE, text=True, check=True).stdout
    for name in ("wh_capture_create", "wh_capture_append", "wh_capture_clear", "wh_capture_take", "wh_capture_destroy", "wh_op_capture_append"):
        assert re.search(r"\b%s\s*\(" % name, hip) and (" T " + name) in dev and name in binding.EXPORTS, name
    assert callable(api.Capture.write) and callable(api.Capture.close) and callable(api.Context.run_capture)
    assert (api.LISTENING, api.VOICE, api.TRANSCRIBING, api.STALLED, api.CAPTURE_STEREO, api.CAPTURE_NO_DROP) == (1, 2, 4, 0x80, 1, 2)
    text = open(os.path.join(ROOT, "include", "whisperApi.h")).read()
    for word in ("struct iPcmCapture : public iAudioCapture", "NoDrop = 2", "createPcmCapture( const sCaptureParams& params, iPcmCapture** pp )"):
        assert word in text, word


def test_capture_object_needs_no_device():
    """the source is host code: create, write, refuse, close -- no device is touched; run_capture's refusals that come before any device work"""
    from whisper_amd import api, build
    if not os.path.exists(api.HOST_LIB_PATH):
        build.build_all()
    cap = api.Capture()
    cap.write(np.zeros(100, np.int16))
    cap.write(np.zeros(40000, np.int16))            # more than a second: queued as several chunks
    with pytest.raises(api.WhisperError) as e:
        cap.write(np.zeros(100, np.float32))        # the format of a capture does not change
    assert e.value.hr == 0x80070057
    with pytest.raises(api.WhisperError):
        cap.write(np.zeros((100, 2), np.int16))
    with pytest.raises(ValueError):
        cap.write(np.zeros(100, np.float64))
    assert api.lib().whisperc_capture_write(cap.h, None, 2, 1, 10) == ctypes.c_int32(0x80070057).value        # s24 is not a capture format
    cap.close()
    with pytest.raises(api.WhisperError) as e:
        cap.write(np.zeros(100, np.int16))
    assert e.value.hr == 0x8000FFFF
    assert cap.dropped_chunks() == 0
    cap.release()
    # without NoDrop the oldest chunks go when more than maxDuration + 1 s is queued: 4 s + 1600
    cap = api.Capture()
    for _ in range(60):
        cap.write(np.zeros(1600, np.float32))
    assert cap.dropped_chunks() == 60 - (64000 // 1600 + 1)        # the queue holds 41 chunks before a write finds more than 64000 queued
    cap.release()
    assert api.lib().whisperc_run_capture(None, None, b"en", 0, None, None, None, None) == ctypes.c_int32(0x80004003).value


def test_cli_parses_the_capture_options():
    """whisper-main --dump-options prints the capture options on a second line, and only with --capture: the first line, which the reference's parser is
    compared with, and the usage text are what they were"""
    import json
    from whisper_amd import build
    if not os.path.exists(build.CLI_BIN):
        build.build_all()
    run = lambda *a: subprocess.run([build.CLI_BIN] + list(a), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=30)
    r = run("--dump-options", "--capture", "-", "--capture-format", "f32", "--capture-channels", "2", "--capture-min-duration", "1.5", "--capture-max-duration", "4",
            "--capture-drop-start-silence", "0.5", "--capture-pause-duration", "0.25", "--capture-no-drop", "-di", "-l", "de")
    assert r.returncode == 0
    first, second = (json.loads(ln) for ln in r.stdout.decode().splitlines())
    assert first["language"] == "de" and first["inputs"] == [] and "capture" not in first
    assert second == dict(capture="-", format="f32", channels=2, min_duration=1.5, max_duration=4, drop_start_silence=0.5, pause_duration=0.25, flags=3)
    r = run("--dump-options", "--capture", "x.raw")
    assert json.loads(r.stdout.decode().splitlines()[1]) == dict(capture="x.raw", format="s16", channels=1, min_duration=2, max_duration=3, drop_start_silence=0.25,
                                                                  pause_duration=0.333, flags=0)
    plain = run("--dump-options", "a.wav")
    assert len(plain.stdout.decode().splitlines()) == 1
    for bad in (["--capture-format", "s24"], ["--capture-channels", "3"], ["--capture"], ["--capture", "x.raw", "a.wav"]):
        r = run(*bad)
        assert r.returncode == 2 and b"error:" in r.stderr, bad
    usage = run("-h").stderr
    assert b"capture" not in usage
