"""CPU tests of the resampler (whisper_amd/csrc/resample.hip, whisper_amd/host/wavFormat.h): the filter's design as a numpy restatement with the
properties a 16 kHz front end needs, the library's tap tables against that restatement (host code: no device), and the WAV header parser through a
stand-alone driver built with the address and undefined-behaviour sanitizers. The kernel itself is tested in tests/test_gpu_resample.py."""
import ctypes as C
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import resample_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = os.path.join(ROOT, "tests", "_build")
RATES = (8000, 11025, 12345, 22050, 24000, 32000, 44100, 48000, 96000)
MARGIN = 400            # outputs left out at both ends of a 0.5 s tone: the filter's run-in (half <= 203 input samples at these rates)


@pytest.fixture(scope="module")
def designs():
    return {fin: R.design(fin) for fin in RATES}


def tone(fin, f, d):
    L, M, half, K, h = d
    t = np.arange(int(fin * 0.5)) / fin
    return R.resample(np.sin(2 * np.pi * f * t).astype(np.float32), L, M, half, K, h)


def test_design_integers():
    got = {fin: R.design(fin)[:4] for fin in (8000, 44100, 48000, 96000, 12345)}
    assert {k: (v[0], v[1], v[3]) for k, v in got.items()} == {8000: (2, 1, 70), 44100: (160, 441, 190), 48000: (1, 3, 206), 96000: (1, 6, 408), 12345: (3200, 2469, 70)}
    for fin, (L, M, half, K) in got.items():
        assert K == 2 * half + 2 and L * fin == M * 16000


@pytest.mark.parametrize("fin", RATES)
def test_filter_properties(fin, designs):
    """DC gain of every phase, tones in the pass band against the analytic tone at 16 kHz, residue of tones beyond 8 kHz."""
    d = designs[fin]
    h = d[4]
    dc = np.abs(h.astype(np.float64).sum(1) - 1.0).max()
    print("%6d Hz  L %d M %d half %d K %d  dc %.2e" % ((fin,) + d[:4] + (dc,)))
    assert dc <= 2e-7
    for f in (100.0, 1000.0, 3000.0):
        if f >= 0.45 * min(fin, 16000):
            continue
        y = tone(fin, f, d)
        want = np.sin(2 * np.pi * f * np.arange(len(y)) / 16000.0)
        err = np.abs(y - want)[MARGIN:-MARGIN].max()
        print("   pass %6.0f Hz  %.2e" % (f, err))
        assert err <= 3e-7
    # the edge of the flat band: the cutoff is 0.9476 * 8 kHz = 7.58 kHz and the transition band reaches down to about 6.5 kHz (2e-5 at 6.6 kHz)
    if 6400.0 < 0.45 * min(fin, 16000):
        y = tone(fin, 6400.0, d)
        err = np.abs(y - np.sin(2 * np.pi * 6400.0 * np.arange(len(y)) / 16000.0))[MARGIN:-MARGIN].max()
        print("   pass   6400 Hz  %.2e" % err)
        assert err <= 3e-7
    for f, bound in ((8500.0, 5e-4), (9000.0, 3e-7), (12000.0, 3e-7), (20000.0, 3e-7)):
        if f >= fin / 2:
            continue
        res = np.abs(tone(fin, f, d))[MARGIN:-MARGIN].max()
        print("   stop %6.0f Hz  %.2e" % (f, res))
        assert res <= bound


@pytest.mark.parametrize("fin", RATES + (1000, 384000))
def test_library_taps_match_the_restatement(fin):
    """wh_resample_taps is host code: the integers are identical, every tap within one float32 ulp of the larger magnitude (the two evaluate I0 and
    sinc with different code, so a double one ulp apart may round to the neighbouring float), exact zeros where the window is zero."""
    from whisper_amd import binding
    lib = binding.lib()
    ints = [C.c_int32() for _ in range(4)]
    binding.check(lib.wh_resample_taps(fin, *[C.byref(i) for i in ints], None, 0))
    L, M, half, K, want = R.design(fin)
    assert tuple(i.value for i in ints) == (L, M, half, K)
    got = np.full((L, K), np.nan, np.float32)
    binding.check(lib.wh_resample_taps(fin, None, None, None, None, got.ctypes.data_as(C.c_void_p), got.size))
    ulp = np.spacing(np.maximum(np.abs(got), np.abs(want)))
    assert (np.abs(got.astype(np.float64) - want.astype(np.float64)) <= ulp).all()
    assert np.array_equal(got == 0, want == 0) and (got[:, K - 1][:1] == 0).all()
    assert lib.wh_resample_taps(fin, None, None, None, None, got.ctypes.data_as(C.c_void_p), got.size - 1) == -1      # WH_E_INVALIDARG: too small
    assert lib.wh_resample_taps(999, None, None, None, None, None, 0) == -1 and lib.wh_resample_taps(384001, None, None, None, None, None, 0) == -1


def test_out_len_without_a_device():
    from whisper_amd import binding
    lib = binding.lib()
    n = C.c_int64(-1)
    for fin in RATES + (16000,):
        L, M = R.design(fin)[:2]
        for frames in (0, 1, 2, 44100, 2 ** 33 + 1):
            binding.check(lib.wh_resample_out_len(fin, frames, C.byref(n)))
            assert n.value == (frames * L + M - 1) // M
    assert lib.wh_resample_out_len(48000, -1, C.byref(n)) == -1 and lib.wh_resample_out_len(500, 1, C.byref(n)) == -1


# ---------------------------------------------------------------------------------------------------------------------
# wavFormat.h through tests/wav_cpu/driver.cpp, a program of its own under the sanitizers
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def driver():
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    os.makedirs(BUILD, exist_ok=True)
    exe = os.path.join(BUILD, "wav-driver")
    src = os.path.join(ROOT, "tests", "wav_cpu", "driver.cpp")
    hdr = os.path.join(ROOT, "whisper_amd", "host", "wavFormat.h")
    if not os.path.exists(exe) or any(os.path.getmtime(d) > os.path.getmtime(exe) for d in (src, hdr)):
        r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I" + os.path.dirname(hdr), src, "-o", exe],
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        assert r.returncode == 0, r.stdout
    return exe


def run_driver(exe, tmp_path, data):
    path = str(tmp_path / "case.wav")
    with open(path, "wb") as f:
        f.write(data)
    r = subprocess.run([exe, path], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=60)
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    assert r.returncode in (0, 2), (r.returncode, r.stderr[-2000:])
    return r.returncode, r.stdout.strip()


def chunk(tag, body):
    return tag + struct.pack("<I", len(body)) + body + (b"\0" if len(body) & 1 else b"")


def fmt_chunk(fmt, channels, rate, extensible=False, block=None, tag=None):
    bits = 8 * R.BYTES[fmt]
    block = channels * R.BYTES[fmt] if block is None else block
    plain = (3 if fmt == R.F32 else 1) if tag is None else tag
    if not extensible:
        return chunk(b"fmt ", struct.pack("<HHIIHH", plain, channels, rate, rate * block, block, bits))
    guid = struct.pack("<H", plain) + bytes([0x00, 0x00, 0x00, 0x00, 0x10, 0x00, 0x80, 0x00, 0x00, 0xAA, 0x00, 0x38, 0x9B, 0x71])
    return chunk(b"fmt ", struct.pack("<HHIIHHHHI", 0xFFFE, channels, rate, rate * block, block, bits, 22, bits, (1 << channels) - 1) + guid)


def riff(*chunks):
    body = b"WAVE" + b"".join(chunks)
    return b"RIFF" + struct.pack("<I", len(body)) + body


def samples(fmt, channels, frames, seed):
    rng = np.random.default_rng(seed)
    if fmt == R.F32:
        raw = rng.uniform(-1, 1, (frames, channels)).astype(np.float32)
    elif fmt == R.U8:
        raw = rng.integers(0, 256, (frames, channels)).astype(np.uint8)
    else:
        bits = 8 * R.BYTES[fmt]
        raw = rng.integers(-2 ** (bits - 1), 2 ** (bits - 1), (frames, channels)).astype(np.int32 if fmt != R.S16 else np.int16)
    return raw, R.pack(raw, fmt).tobytes()


@pytest.mark.parametrize("extensible", [False, True])
@pytest.mark.parametrize("fmt", [R.U8, R.S16, R.S24, R.S32, R.F32])
def test_wav_parser_accepts(driver, tmp_path, fmt, extensible):
    """Every accepted format x 1, 2, 3 and 8 channels, plain and extensible headers, a LIST chunk of odd length before `data` (padded to even), a
    `data` chunk of odd length followed by another chunk: format, channels, rate, first byte, frames and the sum of every converted sample."""
    for channels in (1, 2, 3, 8):
        frames = 11 if (fmt == R.U8 and channels in (1, 3)) or (fmt == R.S24 and channels in (1, 3)) else 10       # odd byte counts where the format allows
        raw, data = samples(fmt, channels, frames, 100 * fmt + channels)
        head = fmt_chunk(fmt, channels, 44100, extensible)
        lst = chunk(b"LIST", b"INFOISFT\x05\0\0\0abcd\0")                     # 17 bytes: odd, so a pad byte follows
        want_sum = float(R.to_float(raw, fmt).astype(np.float64).sum())
        for image, first in ((riff(head, chunk(b"data", data)), 12 + len(head) + 8),
                             (riff(head, lst, chunk(b"data", data), chunk(b"cue ", b"\1\2\3")), 12 + len(head) + len(lst) + 8)):
            rc, out = run_driver(driver, tmp_path, image)
            assert rc == 0, out
            f = out.split()
            assert f[0] == "ok" and [int(v) for v in f[1:6]] == [fmt, channels, 44100, first, frames], out
            assert abs(float(f[6]) - want_sum) <= 1e-6 * max(1.0, abs(want_sum)), (out, want_sum)


def test_wav_parser_clips_a_data_length_past_the_end_of_the_file(driver, tmp_path):
    """A `data` length past the end of the file (a writer that never went back to patch it, a cut download) is handled without a read outside the file:
    the chunk is clipped to what the file holds, whole frames only -- what the loader always did with such files."""
    raw, data = samples(R.S16, 2, 100, 7)
    head = fmt_chunk(R.S16, 2, 48000)
    for claimed in (len(data) + 1, 0x7FFFFFFF, 0xFFFFFFFF):
        rc, out = run_driver(driver, tmp_path, b"RIFF" + struct.pack("<I", 0xFFFFFFFF) + b"WAVE" + head + b"data" + struct.pack("<I", claimed) + data[:-3])
        assert rc == 0 and [int(v) for v in out.split()[1:6]] == [R.S16, 2, 48000, 12 + len(head) + 8, (len(data) - 3) // 4], out


def test_wav_parser_rejects_cleanly(driver, tmp_path):
    """Broken files end in a message, never in a read outside the file (the driver holds the file in a heap block of exactly its size)."""
    raw, data = samples(R.S16, 2, 100, 7)
    good = riff(fmt_chunk(R.S16, 2, 48000), chunk(b"data", data))
    assert run_driver(driver, tmp_path, good)[0] == 0
    rejected = {
        "empty file": b"",
        "RIFF alone": b"RIFF",
        "not WAVE": b"RIFF\x04\0\0\0AVI ",
        "truncated inside fmt": good[:12 + 8 + 10],
        "fmt header only": good[:12 + 8],
        "fmt shorter than 16": riff(chunk(b"fmt ", b"\1\0\2\0"), chunk(b"data", data)),
        "no data chunk": riff(fmt_chunk(R.S16, 2, 48000)),
        "no fmt chunk": riff(chunk(b"data", data)),
        "zero channels": riff(fmt_chunk(R.S16, 0, 48000, block=2), chunk(b"data", data)),
        "nine channels": riff(fmt_chunk(R.S16, 9, 48000), chunk(b"data", data)),
        "block size that is not channels x bytes": riff(fmt_chunk(R.S16, 2, 48000, block=3), chunk(b"data", data)),
        "block size zero": riff(fmt_chunk(R.S16, 2, 48000, block=0), chunk(b"data", data)),
        "compressed format": riff(fmt_chunk(R.S16, 2, 48000, tag=0x55), chunk(b"data", data)),
        "rate too low": riff(fmt_chunk(R.S16, 2, 999), chunk(b"data", data)),
        "rate too high": riff(fmt_chunk(R.S16, 2, 384001), chunk(b"data", data)),
        "float of 16 bits": riff(fmt_chunk(R.S16, 2, 48000, tag=3), chunk(b"data", data)),
        "extensible cut short": riff(fmt_chunk(R.S16, 2, 48000, extensible=True))[:12 + 8 + 30],
        "extensible with a foreign sub-format": riff(fmt_chunk(R.S16, 2, 48000, extensible=True)[:-1] + b"\x00", chunk(b"data", data)),
    }
    for name, image in rejected.items():
        rc, out = run_driver(driver, tmp_path, image)
        assert rc == 2 and out.startswith("rejected: "), (name, rc, out)
    # the message names what is accepted
    assert "8, 16, 24 or 32 bits or float32, 1 to 8 channels, 1000 to 384000 Hz" in run_driver(driver, tmp_path, rejected["nine channels"])[1]
