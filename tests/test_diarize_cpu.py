"""CPU tests of stereo diarization (iContext::detectSpeaker): whisper_amd/host/diarize.h, compiled alone into a program under the address and
undefined-behaviour sanitizers (tests/diarize_cpu/driver.cpp), against a numpy float32 restatement of the reference's rule
(Whisper/Whisper/ContextImpl.diarize.cpp with Spectrogram::copyStereoPcm, Whisper/Whisper/Spectrogram.cpp:142-168). The oracle's harness of ContextImpl stubs
detectSpeaker, so the reference itself cannot be run for this; the restatement below carries its line references. No GPU."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = os.path.join(ROOT, "tests", "_build")

S_OK, E_BOUNDS, OLE_E_BLANK = 0, 0x8000000B, 0x80040007
UNSURE, LEFT, RIGHT, NO_STEREO_DATA = 0, 1, 2, 0xFF
FFT_STEP = 160
NOT_WRITTEN = 0x7E                    # what the driver presets the verdict to: a failed call leaves it


# ---------------------------------------------------------------------------------------------------------------------
# the yardstick
# ---------------------------------------------------------------------------------------------------------------------
def chunk_offset(ticks: int, media_time_offset: int) -> int:
    """diarize.cpp:9-13: `time -= mediaTimeOffset; return ( time * 100 ) / 10'000'000;` on int64 -- C++ division truncates towards zero."""
    v = (ticks - media_time_offset) * 100
    q = abs(v) // 10_000_000
    return q if v >= 0 else -q


def channels_energy(buf: np.ndarray, f64: bool = False):
    """diarize.cpp:17-52 on an [n, 2] float32 array: the SSE accumulator's lanes are ( left, right ) of the even frames and ( left, right ) of the odd frames,
    each lane added to one frame after the other (lines 36-41); a trailing odd frame is loaded into the low two lanes (42-47: the even pair); then
    acc.xy + acc.zw (50). np.cumsum over a float32 array is that sequential single-precision chain. f64 = True sums the same numbers in double precision
    instead: what the comparison would see if the order and the precision of the sums did not matter."""
    a = np.abs(buf.astype(np.float32))                      # _mm_and_ps with 0x7FFFFFFF (29-39): clears the sign, -0.0 -> +0.0, a NaN stays one
    if f64:
        s = a.astype(np.float64).sum(0)
        return np.float32(s[0]), np.float32(s[1])
    lanes = []
    for rows in (a[0::2], a[1::2]):                          # an odd n: the last frame has an even index, it is in the first slice
        for c in range(2):
            col = np.ascontiguousarray(rows[:, c], np.float32)
            with np.errstate(over="ignore"):                 # a sum past FLT_MAX is inf, as it is in the lane
                lanes.append(np.cumsum(col, dtype=np.float32)[-1] if len(col) else np.float32(0))
    with np.errstate(over="ignore"):
        return np.float32(lanes[0] + lanes[2]), np.float32(lanes[1] + lanes[3])


def produce_result(left, right) -> int:
    """diarize.cpp:54-70: lanes flipped, times 1.1f in single precision, `ev > tmp` per lane, the low two bits of the mask: bit 0 = left > 1.1f * right
    (eSpeakerChannel::Left = 1), bit 1 = right > 1.1f * left (Right = 2), neither = Unsure = 0. A NaN compares false both ways."""
    k = np.float32(1.1)
    with np.errstate(invalid="ignore", over="ignore"):
        mask = (1 if left > np.float32(k * right) else 0) | (2 if right > np.float32(k * left) else 0)
    assert mask != 3
    return mask


def detect_speaker(stereo, media_time_offset: int, t0: int, t1: int, f64: bool = False):
    """ContextImpl::detectSpeaker, diarize.cpp:73-108, while a run's spectrogram is current. stereo: [n, 2] float32 or None (the spectrogram has no stereo
    data). t0 / t1: 100 ns ticks. Returns (HRESULT, eSpeakerChannel or None when the call fails)."""
    begin = chunk_offset(t0, media_time_offset)              # 83-87
    end = chunk_offset(t1, media_time_offset)
    length = end - begin                                     # 89
    if length <= 0:                                          # 90-94
        return S_OK, UNSURE
    # Spectrogram::copyStereoPcm( (size_t)begin, (size_t)len, buffer ), Spectrogram.cpp:142-168
    if stereo is None or len(stereo) == 0:                   # 144-145: OLE_E_BLANK, which diarize.cpp:98-102 turns into NoStereoData / S_OK
        return S_OK, NO_STEREO_DATA
    offset = (begin % 2 ** 64) * FFT_STEP % 2 ** 64          # 147-148, on size_t: a negative begin is a huge offset
    if offset >= len(stereo):                                # 149-150
        return E_BOUNDS, None
    buf = np.zeros((length * FFT_STEP, 2), np.float32)       # 154, 166: what is not copied is zero
    n = min(length * FFT_STEP, len(stereo) - offset)         # 161-162
    buf[:n] = stereo[offset:offset + n]
    return S_OK, produce_result(*channels_energy(buf, f64))  # diarize.cpp:105-107


def speakers_of(segments, stereo, media_time_offset: int = 0):
    """What results carry: detect_speaker on the times of every segment {t0, t1 in ticks}; a run without stereo data 0xFF for every segment."""
    out = []
    for s in segments:
        if stereo is None:
            out.append(NO_STEREO_DATA)
            continue
        hr, ch = detect_speaker(stereo, media_time_offset, s["t0"], s["t1"])
        out.append(ch if hr == S_OK else NO_STEREO_DATA)
    return out


# ---------------------------------------------------------------------------------------------------------------------
# diarize.h through its driver
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def driver():
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    os.makedirs(BUILD, exist_ok=True)
    exe = os.path.join(BUILD, "diarize-driver")
    src = os.path.join(ROOT, "tests", "diarize_cpu", "driver.cpp")
    hdrs = [os.path.join(ROOT, "whisper_amd", "host", "diarize.h"), os.path.join(ROOT, "include", "whisperApi.h")]
    if not os.path.exists(exe) or any(os.path.getmtime(d) > os.path.getmtime(exe) for d in [src] + hdrs):
        r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I" + os.path.dirname(hdrs[0]),
                            "-I" + os.path.dirname(hdrs[1]), src, "-o", exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        assert r.returncode == 0, r.stdout
    return exe


def run_cases(exe, tmp_path, cases):
    """cases: (stereo [n, 2] or None, mediaTimeOffset, t0, t1) -> [(HRESULT, verdict)] from the driver."""
    path = str(tmp_path / "cases.bin")
    with open(path, "wb") as f:
        for stereo, off, t0, t1 in cases:
            f.write(struct.pack("<qqQQ", -1 if stereo is None else len(stereo), off, t0 % 2 ** 64, t1 % 2 ** 64))
            if stereo is not None:
                f.write(np.ascontiguousarray(stereo, "<f4").tobytes())
    r = subprocess.run([exe, path], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    out = [(int(a, 16), int(b)) for a, b in (ln.split() for ln in r.stdout.splitlines())]
    assert len(out) == len(cases)
    return out


def check(exe, tmp_path, cases):
    got = run_cases(exe, tmp_path, cases)
    want = [detect_speaker(*c) for c in cases]
    for i, ((hr, ch), (whr, wch)) in enumerate(zip(got, want)):
        assert hr == whr and ch == (NOT_WRITTEN if wch is None else wch), (i, cases[i][1:], hex(hr), ch, hex(whr), wch)
    return want


def noise(frames, seed, left=0.1, right=0.1):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((frames, 2)) * np.array([left, right])).astype(np.float32)


TICKS_PER_CHUNK = 100_000            # 10 ms


def test_chunk_offset_truncates(driver):
    """chunkOffset on ticks where truncation and floor differ (a time before the media time offset that is no whole number of chunks), around zero and
    around a non-zero offset."""
    for off in (0, 12_345_678, -987_654_321):
        for d in (-250_001, -250_000, -100_001, -100_000, -99_999, -50_000, -1, 0, 1, 99_999, 100_000, 100_001, 36_000_000, 3_599_999_999):
            r = subprocess.run([driver, "chunk", str(off + d), str(off)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=60)
            assert r.returncode == 0 and "runtime error" not in r.stderr, r.stderr
            assert int(r.stdout) == chunk_offset(off + d, off), (off, d)
    assert chunk_offset(-50_000, 0) == 0 and (-50_000 * 100) // 10_000_000 == -1          # the two roundings are apart on these ticks
    assert chunk_offset(-150_000, 0) == -1 and (-150_000 * 100) // 10_000_000 == -2


def test_frame_counts(driver, tmp_path):
    """Buffers of 0, 1, 2, 3, 159, 160, 161 and 16001 frames, judged over the chunks they reach into, one chunk fewer and one chunk more: the odd tail, both
    accumulator pairs, zero fill of a last incomplete chunk. An empty buffer has no stereo data."""
    cases = []
    for n in (0, 1, 2, 3, 159, 160, 161, 16001):
        chunks = max(1, -(-n // FFT_STEP))
        for k, (l, r) in enumerate(((0.3, 0.1), (0.1, 0.3), (0.2, 0.2))):
            st = noise(n, 100 + n + k, l, r)
            for c in {max(1, chunks - 1), chunks, chunks + 1}:
                cases.append((st, 0, 0, c * TICKS_PER_CHUNK))
    want = check(driver, tmp_path, cases)
    assert {w[1] for w in want} == {UNSURE, LEFT, RIGHT, NO_STEREO_DATA}
    # one frame: the louder channel of that frame alone
    one = np.array([[0.5, -0.25]], np.float32)
    assert check(driver, tmp_path, [(one, 0, 0, TICKS_PER_CHUNK), (one[:, ::-1], 0, 0, TICKS_PER_CHUNK)]) == [(S_OK, LEFT), (S_OK, RIGHT)]


def test_slices(driver, tmp_path):
    """Where the slice lies in the buffer. The left channel is louder in the first half of the buffer and the right in the second, so a slice that is
    taken from the wrong place gives the wrong verdict."""
    n = 10 * FFT_STEP
    st = noise(n, 7)
    st[:n // 2, 1] *= 0.2
    st[n // 2:, 0] *= 0.2
    t = TICKS_PER_CHUNK
    cases = [(st, 0, 0, 5 * t), (st, 0, 5 * t, 10 * t),                   # ends exactly at the end of the buffer
             (st, 0, 5 * t, 11 * t), (st, 0, 0, 11 * t),                  # ends one chunk past it: zero fill
             (st, 0, 9 * t, 10 * t), (st, 0, 9 * t, 400 * t),             # the last chunk; far past the end
             (st[:9 * FFT_STEP + 1], 0, 9 * t, 10 * t),                   # starts at the last frame
             (st[:9 * FFT_STEP], 0, 9 * t, 10 * t),                       # starts one frame past the end: E_BOUNDS
             (st, 0, 10 * t, 11 * t), (st, 0, 1000 * t, 1001 * t),        # at / far past the end: E_BOUNDS
             (st, 0, 3 * t, 3 * t), (st, 0, 3 * t + 5, 3 * t + 99_000),   # len 0
             (st, 0, 5 * t, 2 * t), (st, 0, 1000 * t, 2 * t),             # len negative -- before the bounds are looked at
             (None, 0, 5 * t, 2 * t), (None, 0, 0, 5 * t),                # no stereo data: len <= 0 is still Unsure
             (st, 0, -t, 3 * t), (st, 0, -7 * t, -2 * t), (st, 0, -50 * t, 50 * t),   # a negative begin: E_BOUNDS
             (st, 0, -50_000, 5 * t)]                                     # ... but -0.5 chunks truncate to chunk 0
    want = check(driver, tmp_path, cases)
    assert want[0] == (S_OK, LEFT) and want[1] == (S_OK, RIGHT) and want[2] == (S_OK, RIGHT) and want[4] == (S_OK, RIGHT)
    assert want[7] == want[8] == want[9] == (E_BOUNDS, None)
    assert want[10] == want[11] == want[12] == want[13] == want[14] == (S_OK, UNSURE) and want[15] == (S_OK, NO_STEREO_DATA)
    assert want[16] == want[17] == want[18] == (E_BOUNDS, None) and want[19] == (S_OK, LEFT)


def test_media_time_offset(driver, tmp_path):
    """A buffer whose first sample is at a media time other than zero: the interval is offset before it is scaled, and ticks that are no whole chunk from
    the offset truncate towards zero on both sides of it."""
    n = 20 * FFT_STEP
    st = noise(n, 11)
    st[:n // 2, 1] *= 0.2
    st[n // 2:, 0] *= 0.2
    t = TICKS_PER_CHUNK
    cases = []
    for off in (36_000_000, 12_345_678, -5_000_001):
        cases += [(st, off, off, off + 10 * t), (st, off, off + 10 * t, off + 20 * t), (st, off, off + 10 * t - 1, off + 20 * t - 1),
                  (st, off, off - 50_000, off + 10 * t), (st, off, off - 99_999, off + 3 * t + 99_999), (st, off, off - t, off + 3 * t),
                  (st, off, 0, off + 3 * t) if off > 0 else (st, off, off + 19 * t + 7, off + 25 * t + 7), (st, off, off + 20 * t, off + 21 * t)]
    want = check(driver, tmp_path, cases)
    assert want[0] == (S_OK, LEFT) and want[1] == (S_OK, RIGHT) and want[3] == (S_OK, LEFT) and want[5] == (E_BOUNDS, None) and want[7] == (E_BOUNDS, None)


SWEEP_FRAMES, SWEEP_SEED, SWEEP_AMPLITUDE = 100 * FFT_STEP, 2024, 0.25


def sweep_cases():
    """The left channel is seeded noise, the right the same noise scaled so that L / R steps through 1.1 * ( 1 +- k * 2^-20 ), k = 0 .. 8; then the mirror
    image for R / L. 34 steps (k = 0 once per side)."""
    rng = np.random.default_rng(SWEEP_SEED)
    left = (SWEEP_AMPLITUDE * rng.standard_normal(SWEEP_FRAMES)).astype(np.float32)
    cases = []
    for mirror in (False, True):
        for k in range(-8, 9):
            ratio = 1.1 * (1.0 + k * 2.0 ** -20)
            right = (left.astype(np.float64) / ratio).astype(np.float32)
            st = np.stack([right, left] if mirror else [left, right], 1)
            cases.append((st, 0, 0, SWEEP_FRAMES // FFT_STEP * TICKS_PER_CHUNK))
    return cases


def test_threshold_sweep(driver, tmp_path):
    """34 recordings whose channel energies are within 8 * 2^-20 of the 1.1 threshold, either way round: the driver's verdict is the restatement's on every
    step. At these distances the verdict depends on the order and the precision of the sums, which is what this case is for: with the same numbers summed
    in double precision the restatement gives another verdict on some of the steps, so a diarize.h that summed in another order would be caught here.

    Measured (seed 2024, 16000 frames, amplitude 0.25; the same on every run): Unsure 12, Left 11, Right 11; the double-precision sums disagree with the
    reference's order on 4 of the 34 steps."""
    cases = sweep_cases()
    want = check(driver, tmp_path, cases)
    again = [detect_speaker(*c) for c in sweep_cases()]
    assert again == want, "the restatement must give the same answers on a repeated run"
    counts = {v: sum(1 for w in want if w == (S_OK, v)) for v in (UNSURE, LEFT, RIGHT)}
    f64 = [detect_speaker(*c, f64=True) for c in cases]
    differ = sum(1 for a, b in zip(want, f64) if a != b)
    print("threshold sweep: Unsure %d, Left %d, Right %d; float64 sums disagree on %d of %d steps" % (counts[UNSURE], counts[LEFT], counts[RIGHT], differ, len(cases)))
    assert all(counts[v] > 0 for v in counts) and sum(counts.values()) == len(cases)
    assert differ >= 1, "the sweep must hold a step on which the summation order decides"


def test_extreme_samples(driver, tmp_path):
    """Full scale either way, denormals, -0.0 and zeros. (A NaN sample needs no case: the reference's comparison is then false both ways round, so the
    verdict is Unsure, and diarize.h compares the same two numbers.)"""
    n = 2 * FFT_STEP
    t = 2 * TICKS_PER_CHUNK
    full = np.ones((n, 2), np.float32)
    full[::2] = -1.0
    tiny = np.full((n, 2), 1e-42, np.float32)                  # denormal
    tiny_left = tiny.copy()
    tiny_left[:, 0] = 3e-42
    neg_zero = np.full((n, 2), -0.0, np.float32)
    half = full.copy()
    half[:, 1] *= 0.5
    edge = full.copy()
    edge[:, 0] = np.float32(1.1)                               # 320 adds of 1.1f in two chains against 1.1f * 320: the sums round, the product rounds once
    big = np.full((n, 2), 3e38, np.float32)                    # the sums overflow to inf: inf > 1.1f * inf is false
    one_den = np.zeros((n, 2), np.float32)
    one_den[n - 1, 1] = 1e-45                                  # the smallest denormal, in the last (odd) frame
    cases = [(x, 0, 0, t) for x in (full, tiny, tiny_left, neg_zero, half, half[:, ::-1], edge, big, one_den, np.zeros((n, 2), np.float32))]
    want = check(driver, tmp_path, cases)
    assert want[0] == (S_OK, UNSURE) and want[2] == (S_OK, LEFT) and want[3] == (S_OK, UNSURE) and want[4] == (S_OK, LEFT) and want[5] == (S_OK, RIGHT)
    assert want[7] == (S_OK, UNSURE) and want[8] == (S_OK, RIGHT) and want[9] == (S_OK, UNSURE)
