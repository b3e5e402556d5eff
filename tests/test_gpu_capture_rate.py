"""GPU tests of live capture at another rate than 16 kHz: the per-chunk kernel with the resumable resampler (whisper_amd/csrc/capture.hip:
wh_op_capture_append_rate, wh_capture_create_rate / _flush / _skip of include/whisper_hip.h) and iContext::runCapture on top of it through
api.Capture( sample_rate = ), the flat C face and whisper-main --capture-rate.

Everything is compared as uint32; no tolerance appears anywhere. The contract: the 16 kHz samples a capture at rate R ever puts into its buffer are, in order,
the samples wh_resample gives for the whole stream at once, whatever the chunk sizes. So the mono samples are wh_resample_host( channel = -1 ) of the whole
source, the kept stereo its channels 0 and 1, and the features of the frames the appends completed, concatenated, are wh_vad_features_host of that mono
buffer. Which outputs appear on which call is tests/capture_rate_ref.py's (the index rule; no sample values). Device outputs sit between NaN guards that
must stay NaN."""
import ctypes as C
import importlib.util
import os
import subprocess

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import capture_rate_ref as CR  # noqa: E402
import capture_ref as R  # noqa: E402
import vad_ref as V  # noqa: E402
from whisper_amd import api, binding, build, ggml_format as gf  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 64
S16, F32 = 1, 4             # wh_pcm_format
INVALID, NOT_READY, BOUNDS = -1, -4, -6
RATES = [48000, 44100, 11025, 8000, 16001]      # L = 1; L = 160, taps in LDS; L = 640; more outputs than inputs; L = 16000, taps from global memory
vp = C.c_void_p


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


DESIGNS = {}


def design(rate):
    """(L, M, half, K) of wh_resample_taps"""
    if rate not in DESIGNS:
        v = [C.c_int32() for _ in range(4)]
        binding.check(binding.lib().wh_resample_taps(rate, *[C.byref(x) for x in v], None, 0))
        DESIGNS[rate] = tuple(x.value for x in v)
    return DESIGNS[rate]


def frames_of(rate):
    return (4 * rate + 4) // 5          # 0.8 s


def resample_host(src, fmt, channels, channel, rate):
    n = len(src)
    n_out = C.c_int64()
    binding.check(binding.lib().wh_resample_out_len(rate, n, C.byref(n_out)))
    dst = np.full(n_out.value, np.nan, np.float32)
    binding.check(binding.lib().wh_resample_host(src.ctypes.data_as(vp), fmt, channels, channel, rate, n, dst.ctypes.data_as(vp), 1, n_out.value))
    return dst


def features_host(mono):
    feat = np.full((len(mono) // 256, 3), np.nan, np.float32)
    if len(feat):
        binding.check(binding.lib().wh_vad_features_host(np.ascontiguousarray(mono).ctypes.data_as(vp), len(mono), feat.ctypes.data_as(vp)))
    return feat


# ---- the 0.8 s source and its references: computed once per (rate, format, channels), shared, left unchanged ------------------------------------------
SOURCES = {}


def source(rate, fmt, channels):
    """(interleaved source at `rate` in its own format, mono, stereo [n][2], features of mono): speech, faint noise, an all-zero stretch (NaN SFM frames),
    full scale, speech again -- laid out at 16 kHz as tests/test_gpu_capture.py does and held at `rate` (frame i is sample i * 16000 // rate), which keeps the
    exact zeros and the full-scale values"""
    key = (rate, fmt, channels)
    if key not in SOURCES:
        j = V.jfk_pcm()[8000:]
        rng = np.random.default_rng(3)
        full = rng.choice(np.array([-1.0, 32767.0 / 32768.0], np.float32), 600)
        n16 = 12801
        left = np.concatenate([j[:4000], V.gap(0.1, 5), np.zeros(2000, np.float32), full, j[20000:]])[:n16].astype(np.float32)
        right = np.concatenate([0.5 * j[40000:45600], np.zeros(2000, np.float32), full, V.gap(0.1, 6), j[::-1]])[:n16].astype(np.float32)
        n = frames_of(rate)
        hold = (np.arange(n, dtype=np.int64) * 16000) // rate
        chans = [left[hold], right[hold]][:channels]
        if fmt == S16:
            src = np.stack([np.clip(np.round(c * 32768.0), -32768, 32767).astype(np.int16) for c in chans], axis=1)
        else:
            src = np.stack([(c * np.float32(0.8137)).astype(np.float32) for c in chans], axis=1)
        src = np.ascontiguousarray(src)
        mono = resample_host(src, fmt, channels, -1, rate)
        stereo = np.ascontiguousarray(np.stack([resample_host(src, fmt, channels, 0, rate), resample_host(src, fmt, channels, channels - 1, rate)], axis=1))
        feat = features_host(mono)
        assert abs(len(mono) - 12800) <= 1 and len(mono) > 3 * 4096
        assert np.isnan(feat[:, 2]).sum() >= 3 and (feat[:, 0] == 0).sum() >= 3         # the all-zero stretch
        assert np.abs(mono).max() >= 0.5 and (fmt != S16 or src.min() == -32768)
        for a in (src, mono, stereo, feat):
            a.setflags(write=False)
        SOURCES[key] = (src, mono, stereo, feat)
    return SOURCES[key]


def frames_for_outputs(d, target):
    """the smallest number of input frames that makes `target` outputs ready"""
    L, M, half, K = d
    n_in = (target * M) // L + half
    s = CR.Stream(*d)
    while s.ready(n_in) < target:
        n_in += 1
    return n_in


def chunkings(rate):
    d = design(rate)
    L, M, half, K = d
    n = frames_of(rate)
    fixed = lambda c: [c] * (n // c) + ([n % c] if n % c else [])
    out = {"whole": [n], "ones_then_rest": [1] * (2 * K) + [n - 2 * K]}
    for c in (half, half + 1, K - 1, K, K + 1):
        out[str(c)] = fixed(c)
    # appends whose outputs end one short of, on and one past a multiple of 256 and of 4096 (where the rate makes two outputs per frame: the nearest above)
    edges = sorted({frames_for_outputs(d, t + e) for t in (256, 4096, 8192, 12288) for e in (-1, 0, 1)})
    edges = [e for e in edges if e < n]
    out["edges"] = [b - a for a, b in zip([0] + edges, edges + [n]) if b > a]
    rng = np.random.default_rng(11)
    irregular = []
    while sum(irregular) < n:
        irregular.append(int(rng.choice([1, 3, half, K - 1, K + 1, 255, 256, 257, 1000, 3 * M, 4096 * M // L, 4097 * M // L + 1, 5000])))
    irregular[-1] -= sum(irregular) - n
    out["irregular"] = [c for c in irregular if c > 0]
    return out


# ---- 1. the op ------------------------------------------------------------------------------------------------------------------------------------------
class OpStream:
    """wh_op_capture_append_rate with the state of a stream held here: every buffer between NaN guards"""

    def __init__(self, rate, fmt, channels, keep, src, cap):
        self.lib = binding.lib()
        self.rate, self.fmt, self.channels, self.keep, self.cap = rate, fmt, channels, keep, cap
        self.d = design(rate)
        self.twin = CR.Stream(*self.d)
        K = self.d[3]
        self.nf = 3 if channels == 2 and keep else 1
        g = lambda n: torch.full((2 * GUARD + n,), float("nan"), dtype=torch.float32, device="cuda")
        self.mono, self.stereo, self.feat = g(cap), g(2 * cap) if keep else None, g(3 * (cap // 256))
        self.hist = [g(self.nf * (K - 1)), g(self.nf * (K - 1))]
        self.cur = 0
        self.src = torch.from_numpy(np.array(src)).cuda()
        self.frame_bytes = src.itemsize * channels
        self.pos = 0            # input frames of src consumed
        self.n = 0              # buffer position
        self.n_in = self.z = 0

    def body(self, t, offset=0):
        return vp(t.data_ptr() + 4 * (GUARD + offset))

    def call(self, count, flush=0, **over):
        n_out = C.c_int64(-1)
        frames = over.pop("frames", count)
        a = dict(src=vp(self.src.data_ptr() + self.pos * self.frame_bytes), fmt=self.fmt, channels=self.channels, rate=self.rate, frames=frames, n_in=self.n_in,
                 z=self.z, flush=flush, hr=self.body(self.hist[self.cur]), hw=self.body(self.hist[self.cur ^ 1]), n=self.n, cap=self.cap, mono=self.body(self.mono),
                 stereo=self.body(self.stereo) if self.keep else None, feat=self.body(self.feat, 3 * (self.n // 256)))
        a.update(over)
        rc = self.lib.wh_op_capture_append_rate(None, a["src"], a["fmt"], a["channels"], a["rate"], a["frames"], a["n_in"], a["z"], a["flush"], a["hr"], a["hw"],
                                                a["n"], a["cap"], a["mono"], a["stereo"], a["feat"], C.byref(n_out))
        return rc, n_out.value

    def append(self, frames):
        rc, n_out = self.call(frames)
        first, last = self.twin.append(frames)
        assert rc == 0 and n_out == last - first, (rc, n_out, first, last)
        self.pos += frames
        self.n_in += frames
        self.n += n_out
        self.cur ^= 1

    def flush(self):
        rc, n_out = self.call(0, flush=1)
        first, last = self.twin.flush()
        assert rc == 0 and n_out == last - first, (rc, n_out, first, last)
        self.n += n_out

    def skip(self, frames):
        # host arithmetic only: nothing is uploaded or launched
        self.twin.skip(frames)
        self.pos += frames
        self.n_in += frames
        self.z = self.n_in

    def check(self, mono, stereo, feat, note):
        torch.cuda.synchronize()
        assert self.n == len(mono), (note, self.n, len(mono))
        pairs = [(self.mono, mono), (self.feat, feat.reshape(-1))] + ([(self.stereo, stereo.reshape(-1))] if self.keep else [])
        for buf, want in pairs:
            out = buf.cpu().numpy()
            assert np.isnan(out[:GUARD]).all() and np.isnan(out[GUARD + want.size:]).all(), ("write outside the destination", note)
            got = out[GUARD:GUARD + want.size]
            assert np.array_equal(bits(got), bits(want)), (note, np.flatnonzero(bits(got) != bits(want))[:5])
        for h in self.hist:
            out = h.cpu().numpy()
            assert np.isnan(out[:GUARD]).all() and np.isnan(out[-GUARD:]).all(), ("write outside the history", note)


CONFIGS = [(S16, 1, False), (S16, 2, True), (F32, 1, True), (F32, 2, False)]


@pytest.mark.parametrize("fmt,channels,keep", CONFIGS)
@pytest.mark.parametrize("rate", RATES)
def test_op_any_chunking_gives_the_whole_streams_bits(rate, fmt, channels, keep):
    src, mono, stereo, feat = source(rate, fmt, channels)
    for name, chunks in chunkings(rate).items():
        assert sum(chunks) == len(src)
        s = OpStream(rate, fmt, channels, keep, src, len(mono))
        for c in chunks:
            s.append(c)
        s.flush()
        s.check(mono, stereo, feat, (rate, name))


@pytest.mark.parametrize("rate", [48000, 8000])
def test_op_a_skip_in_the_middle_gives_the_zeroed_streams_tail(rate):
    fmt, channels, keep = S16, 2, True
    src, mono, stereo, _ = source(rate, fmt, channels)
    d = design(rate)
    L, M, half, K = d
    for before, skipped, chunk in ((3 * K + 11, 2 * K + 5, K - 1), (frames_for_outputs(d, 4096) + 1, half, 1000), (0, 700, K + 1)):
        s = OpStream(rate, fmt, channels, keep, src, len(mono))
        if before:
            s.append(before)
        head = s.n
        s.skip(skipped)
        z = before + skipped
        first = CR.ceil_div(z * L, M)
        rest = len(src) - z
        for c in [chunk] * min(5, rest // chunk):
            s.append(c)
        s.append(len(src) - s.pos)
        s.flush()
        zeroed = np.array(src)
        zeroed[:z] = 0
        want_mono = np.concatenate([mono[:head], resample_host(zeroed, fmt, channels, -1, rate)[first:]])
        want_stereo = np.concatenate([stereo[:head], np.stack([resample_host(zeroed, fmt, channels, c, rate)[first:] for c in (0, 1)], axis=1)])
        s.check(want_mono, want_stereo, features_host(want_mono), (rate, before, skipped, chunk))


def test_op_refusals_launch_nothing():
    rate, fmt, channels = 44100, S16, 2
    src, mono, _, _ = source(rate, fmt, channels)
    s = OpStream(rate, fmt, channels, True, src, len(mono))
    K = s.d[3]
    for over in (dict(rate=999), dict(rate=384001), dict(rate=16000), dict(fmt=2), dict(channels=3), dict(frames=-1), dict(n=-1), dict(n_in=-1), dict(z=1),
                 dict(src=None), dict(mono=None), dict(hr=None), dict(hw=None), dict(hw=s.body(s.hist[s.cur])), dict(feat=None),
                 dict(src=vp(s.src.data_ptr() + 1)), dict(mono=vp(s.mono.data_ptr() + 4 * GUARD + 2)), dict(stereo=vp(s.stereo.data_ptr() + 4 * GUARD + 1)),
                 dict(hr=vp(s.hist[0].data_ptr() + 4 * GUARD + 2)), dict(hw=vp(s.hist[1].data_ptr() + 4 * GUARD + 2)), dict(feat=vp(s.feat.data_ptr() + 4 * GUARD + 1))):
        assert s.call(5000, **over)[0] == INVALID, over
    assert s.call(5000, flush=1)[0] == INVALID                                     # a flush brings no frames
    # outputs that do not fit: 5000 frames make 1726 outputs ready
    ready = CR.Stream(*s.d).ready(5000)
    assert s.call(5000, cap=ready - 1)[0] == BOUNDS and s.call(5000, n=len(mono) - ready + 1)[0] == BOUNDS and s.call(0, n=len(mono) + 1)[0] == BOUNDS
    assert s.call(0) == (0, 0) and s.call(0, src=None, mono=None, hr=None, hw=None, feat=None) == (0, 0)        # nothing to do
    torch.cuda.synchronize()
    for t in (s.mono, s.stereo, s.feat, s.hist[0], s.hist[1]):
        assert torch.isnan(t).all()
    # a chunk below the look-ahead launches for the history alone and appends nothing
    rc, n_out = s.call(s.d[2] + 1, feat=None)
    torch.cuda.synchronize()
    assert (rc, n_out) == (0, 0) and torch.isnan(s.mono).all() and not torch.isnan(s.hist[1][GUARD:-GUARD]).any()


# ---- 2. wh_capture at a rate ----------------------------------------------------------------------------------------------------------------------------
def _generator():
    spec = importlib.util.spec_from_file_location("make_golden_runfull", os.path.join(ROOT, "tests", "golden", "make_golden_runfull.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def model(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("capture_rate") / "cond.bin")
    gf.write_model(path, _generator().model_for(10))
    m = api.Model(path)
    yield m, path
    m.close()


class DeviceCapture:
    def __init__(self, ctx, channels, keep_stereo, cap, rate):
        self.lib = binding.lib()
        self.h = C.c_void_p()
        self.rc = self.lib.wh_capture_create_rate(ctx.handle, channels, 1 if keep_stereo else 0, cap, rate, C.byref(self.h))

    def append(self, chunk, fmt):
        feat = np.full((len(chunk) * 16 // 256 + 3, 3), np.nan, np.float32)
        n_new = C.c_int64(-1)
        rc = self.lib.wh_capture_append(self.h, chunk.ctypes.data_as(vp), fmt, len(chunk), feat.ctypes.data_as(vp), len(feat), C.byref(n_new))
        return rc, n_new.value, feat

    def flush(self):
        feat = np.full((8, 3), np.nan, np.float32)
        n_new = C.c_int64(-1)
        rc = self.lib.wh_capture_flush(self.h, feat.ctypes.data_as(vp), len(feat), C.byref(n_new))
        return rc, n_new.value, feat

    def skip(self, frames):
        n = C.c_int64(-1)
        return self.lib.wh_capture_skip(self.h, frames, C.byref(n)), n.value

    def size(self):
        n = C.c_int64()
        binding.check(self.lib.wh_capture_size(self.h, C.byref(n)))
        return n.value

    def take(self):
        pm, ps, n = C.c_void_p(), C.c_void_p(), C.c_int64()
        binding.check(self.lib.wh_capture_take(self.h, C.byref(pm), C.byref(ps), C.byref(n)))
        mono = np.ctypeslib.as_array(C.cast(pm, C.POINTER(C.c_float)), (n.value,)).copy() if n.value else np.zeros(0, np.float32)
        stereo = np.ctypeslib.as_array(C.cast(ps, C.POINTER(C.c_float)), (n.value, 2)).copy() if ps.value and n.value else None
        return mono, stereo

    def close(self):
        assert self.lib.wh_capture_destroy(self.h) == 0


@pytest.fixture(scope="module")
def device(model):
    hm = binding.HipModel.from_file(model[1])
    ctx = binding.HipContext(hm, 1)
    yield ctx
    ctx.close()
    hm.close()


@pytest.mark.parametrize("rate,fmt,channels,keep", [(48000, S16, 2, True), (44100, F32, 1, True), (11025, F32, 2, False), (8000, S16, 1, False), (16001, S16, 2, True)])
def test_capture_at_a_rate_takes_and_clears_between_chunks(device, rate, fmt, channels, keep):
    src, mono, stereo, feat = source(rate, fmt, channels)
    for name in ("irregular", "edges", str(design(rate)[3] - 1)):
        chunks = chunkings(rate)[name]
        cap = DeviceCapture(device, channels, keep, len(mono) + 300, rate)
        assert cap.rc == 0
        twin = CR.Stream(*design(rate))
        pos, start, feats, since = 0, 0, [], 0
        for i, c in enumerate(chunks + ["flush"]):
            if c == "flush":
                rc, n_new, f = cap.flush()
                first, last = twin.flush()
            else:
                rc, n_new, f = cap.append(np.ascontiguousarray(src[pos:pos + c]), fmt)
                first, last = twin.append(c)
                pos += c
            n = cap.size()
            assert rc == 0 and n - since == last - first and n_new == n // 256 - since // 256, (name, i, c, n, since, first, last, n_new)
            assert np.isnan(f[n_new:]).all()
            # the features of the frames of the BUFFER: the buffer began at output `start` of the stream
            want = features_host(mono[start:start + n])[since // 256:]
            assert np.array_equal(bits(f[:n_new]), bits(want)), (name, i)
            since = n
            # a take or a clear between chunks resets the position only: the stream goes on
            if i % 7 == 3 or c == "flush":
                got_mono, got_stereo = cap.take()
                assert cap.size() == 0
                assert np.array_equal(bits(got_mono), bits(mono[start:start + n])), (name, i)
                if keep:
                    assert np.array_equal(bits(got_stereo), bits(stereo[start:start + n])), (name, i)
                else:
                    assert got_stereo is None
                start, since = start + n, 0
            elif i % 7 == 5:
                binding.check(cap.lib.wh_capture_clear(cap.h))
                assert cap.size() == 0
                start, since = start + n, 0
        # everything taken plus everything cleared, in order, is the whole stream
        assert start == len(mono) and pos == len(src)
        # the stream has ended
        assert cap.append(np.ascontiguousarray(src[:100]), fmt)[0] == NOT_READY and cap.flush()[0] == NOT_READY and cap.skip(5)[0] == NOT_READY
        cap.close()


def test_capture_skip_refusals_and_16_khz(device):
    rate, fmt = 48000, S16
    src, mono, _, _ = source(rate, fmt, 1)
    L, M, half, K = design(rate)
    cap = DeviceCapture(device, 1, False, 4096, rate)
    assert cap.rc == 0
    rc, n_new, _ = cap.append(np.ascontiguousarray(src[:3000]), fmt)
    n0 = cap.size()
    assert rc == 0 and n0 == CR.Stream(L, M, half, K).ready(3000)
    # the skip answers by how much the output clock grew, and appends nothing
    assert cap.skip(700) == (0, CR.ceil_div(3700 * L, M) - n0) and cap.size() == n0 and cap.skip(-1)[0] == INVALID
    assert cap.append(np.ascontiguousarray(src[3700:8000]), fmt)[0] == 0
    zeroed = np.array(src)
    zeroed[:3700] = 0
    tail = resample_host(zeroed, fmt, 1, -1, rate)
    first = CR.ceil_div(3700 * L, M)
    got, _ = cap.take()
    assert np.array_equal(bits(got[:n0]), bits(mono[:n0])) and np.array_equal(bits(got[n0:]), bits(tail[first:first + len(got) - n0]))
    # a chunk whose outputs do not fit, another format, too small a feature buffer: nothing is appended and the stream has not moved
    assert cap.append(np.ascontiguousarray(src[:13000]), fmt)[0] == BOUNDS and cap.append(np.ascontiguousarray(src[:100]), 2)[0] == INVALID
    n_new = C.c_int64()
    assert cap.lib.wh_capture_append(cap.h, src.ctypes.data_as(vp), fmt, 3000, None, 0, C.byref(n_new)) == INVALID and cap.size() == 0
    assert cap.append(np.ascontiguousarray(src[8000:9000]), fmt)[0] == 0
    got, _ = cap.take()
    ready = CR.Stream(L, M, half, K).ready
    assert np.array_equal(bits(got), bits(tail[ready(8000):ready(9000)]))
    cap.close()
    out = C.c_void_p()
    for bad in (999, 384001, 0):
        assert binding.lib().wh_capture_create_rate(device.handle, 1, 0, 4096, bad, C.byref(out)) == INVALID
    # 16000 gives the object wh_capture_create gives: one output per frame at once, nothing to flush, a skip counts frames
    cap = DeviceCapture(device, 1, False, 4096, 16000)
    src16 = source(48000, S16, 1)[0][:1000]
    rc, n_new, _ = cap.append(np.ascontiguousarray(src16), S16)
    assert rc == 0 and cap.size() == 1000 and n_new == 3 and cap.flush()[:2] == (0, 0) and cap.skip(77) == (0, 77) and cap.size() == 1000
    got, _ = cap.take()
    assert np.array_equal(bits(got), bits(src16[:, 0].astype(np.float32) / np.float32(32768.0)))
    cap.close()


# ---- 3. the library: a 48 kHz stream end to end --------------------------------------------------------------------------------------------------------
RECORDING = {}


def recording48():
    """(12.5 s at 48 kHz s16, its 16 kHz mono by the library's whole-buffer resampler): pieces of the host-loop tests' recording between gaps of faint noise,
    brought to 48 kHz by linear interpolation of the 16 kHz samples -- a fixed numpy rule; the library never sees the 16 kHz original"""
    if not RECORDING:
        j = _generator().pcm_for("jfk")
        pcm, _ = V.composite([j, j[20000:100000], (0.6 * j[::-1])[:64000]], [0.8, 0.6, 1.0], 40, lead=0.5)
        pcm = pcm[:200000]
        x = np.interp(np.arange(3 * len(pcm)) / 3.0, np.arange(len(pcm)), pcm.astype(np.float64))
        q = np.clip(np.round(x * 32768.0), -32768, 32767).astype(np.int16)
        mono = api.resample(q, 48000)
        assert len(mono) == len(pcm)
        q.setflags(write=False)
        mono.setflags(write=False)
        RECORDING["q"], RECORDING["mono"] = q, mono
    return RECORDING["q"], RECORDING["mono"]


def twin(mono, n_frames, write):
    """tests/capture_ref.py's loop over the reads the index rule gives for writes of `write` frames and the flush, fed the library's own voice-activity answers"""
    s = CR.Stream(*design(48000))
    reads = []
    for i in range(0, n_frames, write):
        first, last = s.append(min(write, n_frames - i))
        reads.append(last - first)
    first, last = s.flush()
    reads.append(last - first)
    assert sum(reads) == len(mono)
    vad = lambda start, count: api.vad(np.ascontiguousarray(mono[start:start + count]))[1] if count >= 256 else 0
    return R.run(reads, R.Params(flags=R.NO_DROP), vad)


def strip(segs, offset=0):
    return [(s["t0"] - offset, s["t1"] - offset, s["text"], [t["id"] for t in s["tokens"]], [t["p"] for t in s["tokens"]]) for s in segs]


def feed(cap, data, write):
    for i in range(0, len(data), write):
        cap.write(data[i:i + write])
    cap.close()


def check_pieces(m, pieces, mono):
    """every piece's results are run_full of its samples on a fresh context, the times moved by the piece's start"""
    fresh = m.create_context()
    texts = 0
    for start, count, res in pieces:
        fresh.run_full(np.ascontiguousarray(mono[start:start + count]), flags=api.NO_CONTEXT)
        want = fresh.results()
        assert strip(res, start * 625) == strip(want), (start, count)
        texts += len(want)
    fresh.close()
    assert texts >= 1


@pytest.mark.parametrize("write", [480, 4800])          # 10 ms and 100 ms
def test_run_capture_at_48_khz_is_the_twin_and_run_full_piece_by_piece(model, write):
    m, _ = model
    q, mono = recording48()
    want = twin(mono, len(q), write)
    print("twin: pieces %s, status %s" % (want["pieces"], want["status"]))
    assert len(want["pieces"]) >= 3 and want["discarded"] == []
    ctx = m.create_context()
    cap = api.Capture(sample_rate=48000, no_drop=True)
    feed(cap, q, write)
    status = []
    pieces = ctx.run_capture(cap, on_status=status.append, flags=api.NO_CONTEXT)
    ctx.close()
    assert [(s, s + n) for s, n, _ in pieces] == want["pieces"]
    assert status == want["status"]
    check_pieces(m, pieces, mono)


def test_flat_c_and_whisper_main_at_48_khz(model, tmp_path):
    m, path = model
    q, mono = recording48()
    write = 4800
    ctx = m.create_context()
    cap = api.Capture(sample_rate=48000, no_drop=True)
    feed(cap, q, write)
    want = ctx.run_capture(cap, flags=api.NO_CONTEXT)
    assert len(want) >= 3
    lib = api.lib()
    h = C.c_void_p()
    assert lib.whisperc_capture_create_rate(2.0, 3.0, 0.25, 0.333, api.CAPTURE_NO_DROP, 384001, C.byref(h)) == C.c_int32(0x80070057).value
    assert lib.whisperc_capture_create_rate(2.0, 3.0, 0.25, 0.333, api.CAPTURE_NO_DROP, 48000, C.byref(h)) == 0
    for i in range(0, len(q), write):
        part = np.ascontiguousarray(q[i:i + write])
        assert lib.whisperc_capture_write(h, part.ctypes.data_as(C.c_void_p), S16, 1, len(part)) == 0
    assert lib.whisperc_capture_close(h) == 0
    got, words = [], []
    piece_t = C.CFUNCTYPE(None, C.c_void_p, C.c_int64, C.c_int64)
    status_t = C.CFUNCTYPE(C.c_int32, C.c_void_p, C.c_uint8)
    on_piece = piece_t(lambda pv, s, n: got.append((s, n, ctx.results())))
    on_status = status_t(lambda pv, w: words.append(w) or 0)
    assert lib.whisperc_run_capture(ctx.h, h, b"en", api.NO_CONTEXT, None, C.cast(on_status, C.c_void_p), C.cast(on_piece, C.c_void_p), None) == 0
    lib.whisperc_capture_destroy(h)
    ctx.close()
    assert [(s, n, strip(r)) for s, n, r in got] == [(s, n, strip(r)) for s, n, r in want]
    assert words == twin(mono, len(q), write)["status"]
    # whisper-main reads standard input and writes 100 ms at a time: identical text, media times
    r = subprocess.run([build.CLI_BIN, "-m", path, "--capture", "-", "--capture-rate", "48000", "--capture-no-drop", "-nc"], input=q.astype("<i2").tobytes(),
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=240)
    print(r.stdout.decode()[-2000:], r.stderr.decode()[-1500:])
    assert r.returncode == 0
    lines = [ln for ln in r.stdout.decode().splitlines() if ln.startswith("[")]
    segs = [(s["t0"], s["t1"], s["text"].decode()) for _, _, res in want for s in res]
    assert len(lines) == len(segs) >= 3
    seconds = lambda hms: int(hms[0:2]) * 3600 + int(hms[3:5]) * 60 + float(hms[6:12])
    for ln, (t0, t1, text) in zip(lines, segs):
        assert ln[0] == "[" and ln[13:18] == " --> " and ln[30] == "]", ln
        assert ln.endswith("]  " + text), (ln, text)
        assert abs(seconds(ln[1:13]) - t0 / 1e7) < 0.0011 and abs(seconds(ln[18:30]) - t1 / 1e7) < 0.0011, (ln, t0, t1)
    # a rate out of range is refused before anything runs
    r = subprocess.run([build.CLI_BIN, "-m", path, "--capture", "-", "--capture-rate", "500"], input=b"", stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=30)
    assert r.returncode == 2 and b"error:" in r.stderr
