"""GPU tests of the resampler (whisper_amd/csrc/resample.hip; wh_resample* of include/whisper_hip.h) and of what sits on top of it: the WAV loader,
whisper-main and the Python API on files that are not at 16 kHz.

The kernel's sums are FP64 over float taps, one rounding to float at the end, so the reference is the float64 sum over the LIBRARY's own taps
(tests/resample_ref.py) and the bound is one float32 ulp of the reference (the two may round a near-tie differently) plus 1e-12. Sources sit inside
larger tensors whose surroundings are NaN (float) or full-scale samples (integers), destinations are surrounded by and -- at stride 2 -- interleaved
with NaN: a read outside the source or a write outside the destination shows as a wrong or missing value."""
import ctypes as C
import json
import os
import subprocess
import wave

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import resample_ref as R  # noqa: E402
from whisper_amd import api, binding, build, ggml_format as gf  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RATES = (8000, 11025, 12345, 22050, 24000, 32000, 44100, 48000, 96000)
FORMATS = (R.U8, R.S16, R.S24, R.S32, R.F32)
GUARD = 64                  # floats of NaN on both sides of a destination
INVALID = -1                # WH_E_INVALIDARG


def library_design(fin):
    lib = binding.lib()
    ints = [C.c_int32() for _ in range(4)]
    binding.check(lib.wh_resample_taps(fin, *[C.byref(i) for i in ints], None, 0))
    L, M, half, K = (i.value for i in ints)
    taps = np.full((L, K), np.nan, np.float32)
    binding.check(lib.wh_resample_taps(fin, None, None, None, None, taps.ctypes.data_as(C.c_void_p), taps.size))
    return L, M, half, K, taps


def make_input(fmt, channels, frames, seed):
    """uniform in [-1, 1] (integers: the whole range) plus a unit (full-scale) impulse at the first and at the last frame"""
    rng = np.random.default_rng(seed)
    if fmt == R.F32:
        raw = rng.uniform(-1, 1, (frames, channels)).astype(np.float32)
        raw[0] += 1
        raw[-1] += 1
    elif fmt == R.U8:
        raw = rng.integers(0, 256, (frames, channels)).astype(np.uint8)
        raw[0] = raw[-1] = 255
    else:
        bits = 8 * R.BYTES[fmt]
        raw = rng.integers(-2 ** (bits - 1), 2 ** (bits - 1), (frames, channels)).astype(np.int16 if fmt == R.S16 else np.int32)
        raw[0] = raw[-1] = 2 ** (bits - 1) - 1
    return raw


class Source:
    """The bytes of `raw` on the device inside a larger buffer: NaN (float) or full-scale samples (integers) in front and behind; the sample type's
    alignment and no more (an s16 source starts at an address that is 2 mod 4)."""

    def __init__(self, raw, fmt):
        body = R.pack(raw, fmt)
        front = {R.U8: 37, R.S16: 38, R.S24: 37, R.S32: 36, R.F32: 36}[fmt]
        fill = 0xFF if fmt in (R.F32, R.U8) else 0x7F
        buf = np.full(front + len(body) + 64, fill, np.uint8)
        buf[front:front + len(body)] = body
        self.t = torch.from_numpy(buf).cuda()
        self.ptr = C.c_void_p(self.t.data_ptr() + front)


def device_resample(src, fmt, channels, channel, fin, frames, stride, n_out, check=True):
    """wh_resample into a guarded destination: the nOut values, after the guards and the gaps have been found untouched"""
    dst = torch.full((2 * GUARD + n_out * stride,), float("nan"), dtype=torch.float32, device="cuda")
    rc = binding.lib().wh_resample(None, src.ptr, fmt, channels, channel, fin, frames, C.c_void_p(dst.data_ptr() + 4 * GUARD), stride, n_out)
    if not check:
        return rc
    binding.check(rc)
    out = dst.cpu().numpy()
    assert np.isnan(out[:GUARD]).all() and np.isnan(out[GUARD + n_out * stride:]).all(), "write outside the destination"
    body = out[GUARD:GUARD + n_out * stride].reshape(n_out, stride)
    assert np.isnan(body[:, 1:]).all(), "write between the strided outputs"
    return body[:, 0].copy()


# ---- 3. taps -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fin", RATES)
def test_taps(fin):
    """wh_resample_taps against the restatement: identical integers, every tap within one float32 ulp of the larger magnitude, exact zeros where the window
    is zero. And the table the KERNEL reads is that table: the response to a unit impulse is the taps themselves, bit for bit (a product with 1.0 and
    sums with zeros are exact)."""
    L, M, half, K, taps = library_design(fin)
    rl, rm, rhalf, rk, want = R.design(fin)
    assert (L, M, half, K) == (rl, rm, rhalf, rk)
    ulp = np.spacing(np.maximum(np.abs(taps), np.abs(want)))
    d = np.abs(taps.astype(np.float64) - want.astype(np.float64))
    print("%6d Hz: %d of %d taps differ from the restatement, at most %.2f ulp" % (fin, int((taps != want).sum()), taps.size, float((d / ulp).max())))
    assert (d <= ulp).all()
    assert np.array_equal(taps == 0, want == 0) and taps[0, K - 1] == 0
    frames = 2 * K + 3 * M
    x = np.zeros((frames, 1), np.float32)
    at = K + M
    x[at] = 1.0
    n_out = R.out_len(frames, L, M)
    got = device_resample(Source(x, R.F32), R.F32, 1, -1, fin, frames, 1, n_out)
    n = np.arange(n_out, dtype=np.int64)
    k = at - ((n * M) // L - half)
    ok = (k >= 0) & (k < K)
    expect = np.where(ok, taps[(n * M) % L, np.clip(k, 0, K - 1)], np.float32(0))
    assert ok.sum() >= K * L // M - 1 and np.array_equal(got, expect)


# ---- 4. kernel ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fin", [8000, 48000, 44100, 12345, 96000])
def test_kernel_against_float64_sum(fin):
    """Every format x channels 1, 2, 3, 8 x channel -1, 0, C - 1 x dstStride 1, 2 at the frame counts where the kernel's blocks begin and end."""
    L, M, half, K, taps = library_design(fin)
    block = R.block_outputs(L, M, K)
    span = block * M // L                   # input frames one block of outputs spans
    sizes = sorted({1, 2, K - 1, K, K + 1, span - 1, span, span + 1, 3 * span + 17})
    worst = 0.0
    calls = 0
    for frames in sizes:
        n_out = R.out_len(frames, L, M)
        assert n_out > (160 if frames >= span else 0)           # the phases wrap within a block (L <= 160 at the rates with a table in LDS)
        for fmt in FORMATS:
            for channels in (1, 2, 3, 8):
                raw = make_input(fmt, channels, frames, frames * 131 + fmt * 17 + channels)
                src = Source(raw, fmt)
                x = R.to_float(raw, fmt)
                for channel in sorted({-1, 0, channels - 1}):
                    ref = R.resample(R.downmix(x, channel), L, M, half, K, taps)
                    bound = R.ulp32(ref) + 1e-12
                    for stride in (1, 2):
                        got = device_resample(src, fmt, channels, channel, fin, frames, stride, n_out)
                        assert np.isfinite(got).all(), (fin, frames, fmt, channels, channel, stride)
                        err = np.abs(got.astype(np.float64) - ref)
                        worst = max(worst, float((err / bound).max()))
                        assert (err <= bound).all(), (fin, frames, fmt, channels, channel, stride, float(err.max()), int(np.argmax(err - bound)))
                        calls += 1
    print("%6d Hz  L %d M %d K %d  block %d  sizes %s  %d calls  worst error / bound %.3f" % (fin, L, M, K, block, sizes, calls, worst))


@pytest.mark.parametrize("fin", [384000, 192000, 11025, 383984])
def test_kernel_block_rule_and_chunked_table(fin):
    """The rates at which a workgroup owns fewer than 1024 outputs (256 at 384 kHz, 576 at 192 kHz), the table staged in chunks of few taps (L = 640 at
    11025 Hz) and a steep ratio with the table read from global memory (L = 1000, M = 23999), on a reduced format / channel matrix."""
    L, M, half, K, taps = library_design(fin)
    block = R.block_outputs(L, M, K)
    assert block == {384000: 256, 192000: 576, 11025: 1024, 383984: 256}[fin]
    span = block * M // L
    worst = 0.0
    for frames in sorted({1, K - 1, K + 1, span - 1, span, span + 1, 3 * span + 17}):
        n_out = R.out_len(frames, L, M)
        for fmt, channels, channel, stride in ((R.S16, 2, -1, 1), (R.F32, 1, -1, 2), (R.S24, 3, 2, 1), (R.U8, 8, -1, 2), (R.S32, 2, 0, 1)):
            raw = make_input(fmt, channels, frames, frames * 7 + fmt)
            ref = R.resample(R.downmix(R.to_float(raw, fmt), channel), L, M, half, K, taps)
            bound = R.ulp32(ref) + 1e-12
            got = device_resample(Source(raw, fmt), fmt, channels, channel, fin, frames, stride, n_out)
            err = np.abs(got.astype(np.float64) - ref)
            worst = max(worst, float((err / bound).max()))
            assert np.isfinite(got).all() and (err <= bound).all(), (fin, frames, fmt, channels, channel, stride, float(err.max()))
    print("%6d Hz  L %d M %d K %d  block %d  worst error / bound %.3f" % (fin, L, M, K, block, worst))


def test_taps_through_lds_and_from_global_memory_give_the_same_bits():
    """The option "resample_lds_phases" only moves the taps' way to the lanes: the same sums in the same order."""
    frames, fin = 9000, 44100
    raw = make_input(R.S16, 2, frames, 3)
    src = Source(raw, R.S16)
    n_out = R.out_len(frames, 160, 441)
    try:
        binding.set_option("resample_lds_phases", 0)
        a = device_resample(src, R.S16, 2, -1, fin, frames, 1, n_out)
    finally:
        binding.set_option("resample_lds_phases", binding.get_option_default("resample_lds_phases"))
    b = device_resample(src, R.S16, 2, -1, fin, frames, 1, n_out)
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


# ---- 5. bypass, lengths, arguments -------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", FORMATS)
def test_bypass_at_16000_is_bit_exact(fmt):
    """Nothing is filtered at 16 kHz: the conversion formulas and the FP32 downmix, bit for bit (two channels: the bits of 0.5f * ( l + r ))."""
    for channels in (1, 2, 3, 8):
        frames = 1000 + channels
        raw = make_input(fmt, channels, frames, 5 * fmt + channels)
        src = Source(raw, fmt)
        x = R.to_float(raw, fmt)
        for channel in sorted({-1, 0, channels - 1}):
            for stride in (1, 2):
                got = device_resample(src, fmt, channels, channel, 16000, frames, stride, frames)
                want = R.downmix(x, channel)
                assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (fmt, channels, channel, stride)
        if channels == 2:
            assert np.array_equal(R.downmix(x, -1), np.float32(0.5) * (x[:, 0] + x[:, 1]))


def test_out_len_and_invalid_arguments():
    lib = binding.lib()
    n = C.c_int64(-1)
    for fin in RATES:
        L, M = R.design(fin)[:2]
        for frames in (0, 1, 2 ** 33 + 1):
            binding.check(lib.wh_resample_out_len(fin, frames, C.byref(n)))
            assert n.value == (frames * L + M - 1) // M
    frames, fin = 500, 44100
    raw = make_input(R.S16, 2, frames, 1)
    src = Source(raw, R.S16)
    n_out = R.out_len(frames, 160, 441)
    assert len(device_resample(src, R.S16, 2, -1, fin, frames, 1, n_out)) == n_out
    assert device_resample(src, R.S16, 2, -1, fin, 0, 1, 0, check=False) == 0                  # nothing in, nothing out
    bad = [dict(fin=999), dict(fin=384001), dict(fin=0), dict(fmt=-1), dict(fmt=5), dict(channels=0), dict(channels=9), dict(channel=-2), dict(channel=2),
           dict(stride=0), dict(stride=3), dict(n_out=n_out - 1), dict(n_out=n_out + 1), dict(frames=-1)]
    for b in bad:
        a = dict(fmt=R.S16, channels=2, channel=-1, fin=fin, frames=frames, stride=1, n_out=n_out)
        a.update(b)
        assert device_resample(src, a["fmt"], a["channels"], a["channel"], a["fin"], a["frames"], a["stride"], a["n_out"], check=False) == INVALID, b
    host = np.zeros(n_out, np.float32)
    hp = host.ctypes.data_as(C.c_void_p)
    rp = np.ascontiguousarray(raw).ctypes.data_as(C.c_void_p)
    assert lib.wh_resample_host(rp, R.S16, 2, -1, 999, frames, hp, 1, n_out) == INVALID
    assert lib.wh_resample_host(rp, R.S16, 2, 2, fin, frames, hp, 1, n_out) == INVALID
    assert lib.wh_resample_host(rp, R.S16, 2, -1, fin, frames, hp, 3, n_out) == INVALID
    assert lib.wh_resample_host(rp, R.S16, 2, -1, fin, frames, hp, 1, n_out + 1) == INVALID
    assert lib.wh_resample_host(None, R.S16, 2, -1, fin, 0, None, 1, 0) == 0


# ---- 6. host entry and Python API --------------------------------------------------------------------------------------
@pytest.mark.parametrize("fin,fmt,channels", [(44100, R.S16, 2), (48000, R.F32, 1), (8000, R.U8, 3), (96000, R.S24, 2), (22050, R.S32, 8), (16000, R.S16, 2)])
def test_host_entry_and_python_api_match_the_device_call(fin, fmt, channels):
    lib = binding.lib()
    frames = 3 * fin // 10 + 7
    raw = make_input(fmt, channels, frames, fin + fmt)
    packed = R.pack(raw, fmt)
    L, M = R.design(fin)[:2] if fin != 16000 else (1, 1)
    n_out = R.out_len(frames, L, M)
    src = Source(raw, fmt)
    for channel in (-1, channels - 1):
        want = device_resample(src, fmt, channels, channel, fin, frames, 1, n_out)
        for stride in (1, 2):
            host = np.full(n_out * stride, np.nan, np.float32)
            binding.check(lib.wh_resample_host(packed.ctypes.data_as(C.c_void_p), fmt, channels, channel, fin, frames, host.ctypes.data_as(C.c_void_p), stride, n_out))
            assert np.array_equal(host[::stride].view(np.uint32), want.view(np.uint32)) and np.isnan(host.reshape(n_out, stride)[:, 1:]).all()
        if fmt != R.S24:
            got = api.resample(raw if channels > 1 else raw[:, 0], fin, channel)
            assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), want.view(np.uint32))
    with pytest.raises(ValueError):
        api.resample(np.zeros(10, np.float64), 44100)
    with pytest.raises(api.WhisperError):
        api.resample(np.zeros(10, np.float32), 500)


# ---- 7. end to end -----------------------------------------------------------------------------------------------------
def voice(t, ch):
    """three amplitude-modulated sines below 3 kHz; |.| <= 0.675"""
    parts = [(220.0, 3.0, 0.20, 0.1), (1310.0, 5.0, 0.15, 0.7), (2870.0, 7.0, 0.10, 1.9)] if ch == 0 else \
            [(330.0, 2.0, 0.20, 0.4), (990.0, 4.0, 0.15, 1.1), (2500.0, 6.0, 0.10, 2.3)]
    return sum(a * (1 + 0.5 * np.sin(2 * np.pi * m * t)) * np.sin(2 * np.pi * f * t + ph) for f, m, a, ph in parts)


SECONDS = 3
FILES = {"44k_stereo_s16": (44100, 2, 2), "48k_mono_s24": (48000, 1, 3), "8k_mono_u8": (8000, 1, 1)}        # rate, channels, bytes per sample


@pytest.fixture(scope="module")
def clips(tmp_path_factory):
    d = tmp_path_factory.mktemp("resample_e2e")
    t16 = np.arange(SECONDS * 16000) / 16000.0
    out = {"analytic": [voice(t16, 0), voice(t16, 1)], "paths": {}, "float": {}}
    path = str(d / "16k.wav")
    with wave.open(path, "wb") as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(16000)
        w.writeframes(np.clip(np.round(voice(t16, 0) * 32768.0), -32768, 32767).astype("<i2").tobytes())
    out["paths"]["16k"] = path
    for name, (rate, channels, width) in FILES.items():
        t = np.arange(SECONDS * rate) / rate
        x = np.stack([voice(t, c) for c in range(channels)], 1)
        scale = 2.0 ** (8 * width - 1)
        q = np.clip(np.round(x * scale), -scale, scale - 1).astype(np.int32)
        if width == 1:
            data = (q + 128).astype(np.uint8).tobytes()
        elif width == 2:
            data = q.astype("<i2").tobytes()
        else:
            data = R.pack(q, R.S24).tobytes()
        path = str(d / (name + ".wav"))
        with wave.open(path, "wb") as w:
            w.setnchannels(channels)
            w.setsampwidth(width)
            w.setframerate(rate)
            w.writeframes(data)
        out["paths"][name] = path
        out["float"][name] = x.mean(1).astype(np.float32)
    case = [c for c in json.load(open(os.path.join(ROOT, "tests", "golden", "ref_hostloop.json")))["cases"] if c["name"] == "first_window_no_prompt"][0]
    out["model"] = str(d / "m.bin")
    gf.write_model(out["model"], gf.scripted_model(case["script"], case["prompt_len"]))
    out["lang"] = case["lang"]
    return out


@pytest.mark.parametrize("name", list(FILES))
def test_load_audio_is_the_analytic_signal(clips, name):
    """The file at its own rate against the same signal evaluated at 16 kHz: within the format's quantisation step 2^-b (b = bits - 1) plus the filter's
    3e-7, away from the first and last `half` outputs. Whole seconds keep the sample count."""
    rate, channels, width = FILES[name]
    half = R.design(rate)[2]
    got = api.load_audio(clips["paths"][name])
    assert got.dtype == np.float32 and got.shape == (SECONDS * 16000,)
    want = sum(clips["analytic"][:channels]) / channels
    bound = 2.0 ** -(8 * width - 1) + 3e-7
    err = np.abs(got.astype(np.float64) - want)[half:-half].max()
    print("%s: max error %.3e, bound %.3e" % (name, err, bound))
    assert err <= bound
    st = api.load_audio(clips["paths"][name], stereo=True)
    assert st.shape == (SECONDS * 16000, 2)
    for c in range(2):
        e = np.abs(st[:, c].astype(np.float64) - clips["analytic"][c if channels == 2 else 0])[half:-half].max()
        assert e <= bound, (name, c, e)
    if channels == 2:           # the two channels are apart
        assert np.abs(st[:, 0] - st[:, 1]).max() > 0.3
    else:
        assert np.array_equal(st[:, 0], got) and np.array_equal(st[:, 1], got)


def test_load_audio_at_16k_keeps_todays_samples(clips):
    got = api.load_audio(clips["paths"]["16k"])
    t16 = np.arange(SECONDS * 16000) / 16000.0
    q = np.clip(np.round(voice(t16, 0) * 32768.0), -32768, 32767).astype(np.int16)
    assert np.array_equal(got, q.astype(np.float32) / np.float32(32768.0))


def test_transcripts_do_not_depend_on_the_files_rate(clips):
    """whisper-main and Context.run_streamed on each file: the transcript and the times of the 16 kHz file (the scripted model's tokens do not depend on the
    audio; the windows, seeks and times depend on the number of 16 kHz samples, which whole seconds keep)."""
    if not os.path.exists(build.CLI_BIN):
        build.build_all()

    def cli(path):
        r = subprocess.run([build.CLI_BIN, "-m", clips["model"], "-f", path, "-l", clips["lang"], "-nc"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
        assert r.returncode == 0, r.stderr.decode()[-2000:]
        return r.stdout.decode()

    want_cli = cli(clips["paths"]["16k"])
    assert "-->" in want_cli
    m = api.Model(clips["model"])
    ctx = m.create_context()
    t16 = np.arange(SECONDS * 16000) / 16000.0
    hr, _ = ctx.run_streamed(voice(t16, 0).astype(np.float32), language=clips["lang"], flags=api.NO_CONTEXT)
    want = [(s["t0"], s["t1"], s["text"], [t["id"] for t in s["tokens"]]) for s in ctx.results()]
    assert hr == 0 and want
    hr = ctx.run_full(voice(t16, 0).astype(np.float32), language=clips["lang"], flags=api.NO_CONTEXT)
    want_full = [(s["t0"], s["t1"], s["text"], [t["id"] for t in s["tokens"]]) for s in ctx.results()]
    assert hr == 0 and want_full
    for name, (rate, channels, width) in FILES.items():
        assert cli(clips["paths"][name]) == want_cli, name
        hr, _ = ctx.run_streamed(clips["float"][name], language=clips["lang"], flags=api.NO_CONTEXT, sample_rate=rate)
        assert hr == 0 and [(s["t0"], s["t1"], s["text"], [t["id"] for t in s["tokens"]]) for s in ctx.results()] == want, name
        hr = ctx.run_full(clips["float"][name], language=clips["lang"], flags=api.NO_CONTEXT, sample_rate=rate)
        assert hr == 0 and [(s["t0"], s["t1"], s["text"], [t["id"] for t in s["tokens"]]) for s in ctx.results()] == want_full, name
    # what the loader refuses stays E_INVALIDARG and the tool says so
    bad = clips["paths"]["16k"] + ".9ch.wav"
    with wave.open(bad, "wb") as w:
        w.setnchannels(9)
        w.setsampwidth(2)
        w.setframerate(44100)
        w.writeframes(b"\0" * 18 * 100)
    with pytest.raises(api.WhisperError) as e:
        api.load_audio(bad)
    assert e.value.hr == 0x80070057
