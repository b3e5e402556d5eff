"""GPU tests of live capture: the per-chunk kernel (whisper_amd/csrc/capture.hip: wh_op_capture_append, wh_capture_* of include/whisper_hip.h) and
iContext::runCapture on top of it (whisper_amd/host/capture.cpp, captureLoop.h) through api.Capture / Context.run_capture, the flat C face and whisper-main.

The kernel has exact references, all of this library and all bit for bit: the mono samples are wh_resample_host( inRate = 16000, channel = -1 ) of the
same source, the kept stereo its two channel extractions, and the features of the frames the chunks completed, concatenated, are wh_vad_features_host of
the mono buffer (compared as uint32, so NaN patterns count) -- whatever the chunking. Device outputs sit between NaN guards that must stay NaN.
The library has the twin of tests/capture_ref.py, fed the library's own voice-activity answers (api.vad) for every buffered span: under NoDrop the pieces
and the status words must be the twin's exactly, and every piece's results those of run_full on the same samples."""
import ctypes as C
import importlib.util
import os
import subprocess
import threading

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import capture_ref as R  # noqa: E402
import vad_ref as V  # noqa: E402
from whisper_amd import api, binding, build, ggml_format as gf  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 64
N = 48000                   # 3 s
S16, F32 = 1, 4             # wh_pcm_format
INVALID, BOUNDS = -1, -6


# ---- the 3 s buffer and its references: computed once, shared, left unchanged --------------------------------------------------------------------------
def chunkings():
    rng = np.random.default_rng(11)
    irregular = []
    while sum(irregular) < N:
        irregular.append(int(rng.choice([1, 3, 100, 255, 256, 257, 511, 1000, 4095, 4096, 4097, 5000])))
    irregular[-1] -= sum(irregular) - N
    fixed = lambda c: [c] * (N // c) + ([N % c] if N % c else [])
    out = {"whole": [N], "ones_then_rest": [1] * 600 + [N - 600], "irregular": [c for c in irregular if c > 0]}
    for c in (255, 256, 257, 4095, 4096, 4097):
        out[str(c)] = fixed(c)
    return out


CHUNKINGS = chunkings()
SOURCES = {}


def source(fmt, channels):
    """(interleaved source in its own format, mono, stereo [N][2], features of mono): speech, a gap of faint noise, an all-zero stretch (NaN SFM frames),
    full scale, speech again"""
    key = (fmt, channels)
    if key not in SOURCES:
        j = V.jfk_pcm()[8000:]
        rng = np.random.default_rng(3)
        full = rng.choice(np.array([-1.0, 32767.0 / 32768.0], np.float32), 2000)
        left = np.concatenate([j[:20000], V.gap(0.3, 5), np.zeros(3000, np.float32), full, j[20000:]])[:N].astype(np.float32)
        # the second channel: another recording, silent and at full scale where the first is, so that the mix has both
        right = np.concatenate([0.5 * j[40000:64800], np.zeros(3000, np.float32), full, V.gap(0.4, 6), j[::-1]])[:N].astype(np.float32)
        chans = [left, right][:channels]
        if fmt == S16:
            src = np.stack([np.clip(np.round(c * 32768.0), -32768, 32767).astype(np.int16) for c in chans], axis=1)
        else:
            # not representable in 16 bits: the f32 path takes the samples as they are
            src = np.stack([(c * np.float32(0.8137)).astype(np.float32) for c in chans], axis=1)
        src = np.ascontiguousarray(src)
        lib = binding.lib()
        outs = []
        for channel in (-1, 0, channels - 1):
            dst = np.full(N, np.nan, np.float32)
            binding.check(lib.wh_resample_host(src.ctypes.data_as(C.c_void_p), fmt, channels, channel, 16000, N, dst.ctypes.data_as(C.c_void_p), 1, N))
            outs.append(dst)
        mono = outs[0]
        stereo = np.ascontiguousarray(np.stack([outs[1], outs[2]], axis=1))
        feat = np.full((N // 256, 3), np.nan, np.float32)
        binding.check(lib.wh_vad_features_host(mono.ctypes.data_as(C.c_void_p), N, feat.ctypes.data_as(C.c_void_p)))
        assert np.isnan(feat[:, 2]).sum() >= 5 and (feat[:, 0] == 0).sum() >= 5        # the all-zero stretch
        assert np.abs(mono).max() >= 0.8 and (fmt != S16 or src.min() == -32768)
        for a in (src, mono, stereo, feat):
            a.setflags(write=False)
        SOURCES[key] = (src, mono, stereo, feat)
    return SOURCES[key]


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---- 1. the op ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt,channels", [(S16, 1), (S16, 2), (F32, 1), (F32, 2)])
@pytest.mark.parametrize("name", list(CHUNKINGS))
def test_op_any_chunking_gives_the_whole_buffers_bits(fmt, channels, name):
    src, mono, stereo, feat = source(fmt, channels)
    lib = binding.lib()
    dev_src = torch.from_numpy(np.array(src)).cuda()
    g = lambda n: torch.full((2 * GUARD + n,), float("nan"), dtype=torch.float32, device="cuda")
    d_mono, d_stereo, d_feat = g(N), g(2 * N), g(3 * (N // 256))
    frame_bytes = src.itemsize * channels
    pos = 0
    for c in CHUNKINGS[name]:
        done = pos // 256
        binding.check(lib.wh_op_capture_append(None, C.c_void_p(dev_src.data_ptr() + pos * frame_bytes), fmt, channels, pos, c, N,
                                               C.c_void_p(d_mono.data_ptr() + 4 * GUARD), C.c_void_p(d_stereo.data_ptr() + 4 * GUARD),
                                               C.c_void_p(d_feat.data_ptr() + 4 * (GUARD + 3 * done))))
        pos += c
    assert pos == N
    torch.cuda.synchronize()
    for buf, want in ((d_mono, mono), (d_stereo, stereo.reshape(-1)), (d_feat, feat.reshape(-1))):
        out = buf.cpu().numpy()
        assert np.isnan(out[:GUARD]).all() and np.isnan(out[GUARD + want.size:]).all(), "write outside the destination"
        got = out[GUARD:GUARD + want.size]
        assert np.array_equal(bits(got), bits(want)), (name, np.flatnonzero(bits(got) != bits(want))[:5])


def test_op_without_stereo_and_refusals():
    src, mono, _, feat = source(S16, 2)
    lib = binding.lib()
    dev_src = torch.from_numpy(np.array(src)).cuda()
    d_mono = torch.full((2 * GUARD + N,), float("nan"), dtype=torch.float32, device="cuda")
    d_feat = torch.full((2 * GUARD + 3 * (N // 256),), float("nan"), dtype=torch.float32, device="cuda")
    pm, pf, ps = d_mono.data_ptr() + 4 * GUARD, d_feat.data_ptr() + 4 * GUARD, dev_src.data_ptr()
    vp = C.c_void_p
    # refusals launch nothing: the destinations stay NaN
    assert lib.wh_op_capture_append(None, vp(ps), S16, 2, N - 100, 101, N, vp(pm), None, vp(pf)) == BOUNDS
    assert lib.wh_op_capture_append(None, vp(ps), S16, 2, N + 1, 0, N, vp(pm), None, vp(pf)) == BOUNDS
    assert lib.wh_op_capture_append(None, vp(ps), 2, 2, 0, 256, N, vp(pm), None, vp(pf)) == INVALID           # s24
    assert lib.wh_op_capture_append(None, vp(ps), S16, 3, 0, 256, N, vp(pm), None, vp(pf)) == INVALID
    assert lib.wh_op_capture_append(None, None, S16, 2, 0, 256, N, vp(pm), None, vp(pf)) == INVALID
    assert lib.wh_op_capture_append(None, vp(ps), S16, 2, 0, 256, N, None, None, vp(pf)) == INVALID
    assert lib.wh_op_capture_append(None, vp(ps), S16, 2, 0, 256, N, vp(pm), None, None) == INVALID
    assert lib.wh_op_capture_append(None, vp(ps + 1), S16, 2, 0, 256, N, vp(pm), None, vp(pf)) == INVALID
    assert lib.wh_op_capture_append(None, vp(ps), F32, 2, 0, 256, N, vp(pm + 2), None, vp(pf)) == INVALID
    assert lib.wh_op_capture_append(None, vp(ps), S16, 2, -1, 256, N, vp(pm), None, vp(pf)) == INVALID
    assert lib.wh_op_capture_append(None, vp(ps), S16, 2, 0, -1, N, vp(pm), None, vp(pf)) == INVALID
    assert lib.wh_op_capture_append(None, None, S16, 2, 7, 0, N, None, None, None) == 0                        # nothing to do
    torch.cuda.synchronize()
    assert torch.isnan(d_mono).all() and torch.isnan(d_feat).all()
    # stereo not kept, a chunk that completes no frame, then the rest
    binding.check(lib.wh_op_capture_append(None, vp(ps), S16, 2, 0, 255, N, vp(pm), None, None))
    binding.check(lib.wh_op_capture_append(None, vp(ps + 255 * 4), S16, 2, 255, N - 255, N, vp(pm), None, vp(pf)))
    torch.cuda.synchronize()
    assert np.array_equal(bits(d_mono.cpu().numpy()[GUARD:GUARD + N]), bits(mono))
    assert np.array_equal(bits(d_feat.cpu().numpy()[GUARD:-GUARD]), bits(feat.reshape(-1)))


# ---- 2. wh_capture --------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def model(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("capture") / "cond.bin")
    gf.write_model(path, _generator().model_for(10))
    m = api.Model(path)
    yield m, path
    m.close()


def _generator():
    spec = importlib.util.spec_from_file_location("make_golden_runfull", os.path.join(ROOT, "tests", "golden", "make_golden_runfull.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


class DeviceCapture:
    """wh_capture_* over a device context of its own (wh_capture_create only takes the device from it)"""

    def __init__(self, model_path, channels, keep_stereo, cap):
        self.lib = binding.lib()
        self.model = binding.HipModel.from_file(model_path)
        self.ctx = binding.HipContext(self.model, 1)
        self.h = C.c_void_p()
        binding.check(self.lib.wh_capture_create(self.ctx.handle, channels, 1 if keep_stereo else 0, cap, C.byref(self.h)))

    def append(self, chunk, fmt, feat_cap=None):
        frames = len(chunk)
        feat = np.full((frames // 256 + 2, 3), np.nan, np.float32)
        n_new = C.c_int64(-1)
        rc = self.lib.wh_capture_append(self.h, chunk.ctypes.data_as(C.c_void_p), fmt, frames, feat.ctypes.data_as(C.c_void_p),
                                        len(feat) if feat_cap is None else feat_cap, C.byref(n_new))
        return rc, n_new.value, feat

    def size(self):
        n = C.c_int64()
        binding.check(self.lib.wh_capture_size(self.h, C.byref(n)))
        return n.value

    def take(self):
        pm, ps, n = C.c_void_p(), C.c_void_p(), C.c_int64()
        binding.check(self.lib.wh_capture_take(self.h, C.byref(pm), C.byref(ps), C.byref(n)))
        mono = np.ctypeslib.as_array(C.cast(pm, C.POINTER(C.c_float)), (n.value,)) if n.value else np.zeros(0, np.float32)
        stereo = np.ctypeslib.as_array(C.cast(ps, C.POINTER(C.c_float)), (n.value, 2)) if ps.value and n.value else None
        return mono, stereo

    def close(self):
        assert self.lib.wh_capture_destroy(self.h) == 0
        self.ctx.close()
        self.model.close()


@pytest.fixture(scope="module")
def captures(model):
    made = {}

    def get(channels, keep):
        if (channels, keep) not in made:
            made[(channels, keep)] = DeviceCapture(model[1], channels, keep, N + 4097)
        return made[(channels, keep)]
    yield get
    for c in made.values():
        c.close()


@pytest.mark.parametrize("fmt,channels,keep", [(S16, 2, True), (F32, 1, True), (F32, 2, False), (S16, 1, False)])
def test_capture_append_take_clear(captures, fmt, channels, keep):
    src, mono, stereo, feat = source(fmt, channels)
    cap = captures(channels, keep)
    binding.check(cap.lib.wh_capture_clear(cap.h))
    first = None
    for name, chunks in CHUNKINGS.items():
        pos, feats = 0, []
        for c in chunks:
            rc, n_new, f = cap.append(np.ascontiguousarray(src[pos:pos + c]), fmt)
            assert rc == 0 and n_new == (pos + c) // 256 - pos // 256, (name, pos, c, n_new)
            assert np.isnan(f[n_new:]).all()            # nothing behind the completed frames is written
            feats.append(f[:n_new])
            pos += c
        assert cap.size() == N
        assert np.array_equal(bits(np.concatenate(feats)), bits(feat)), name
        if name == "whole":
            # clear, then the same appends, gives the same bytes
            binding.check(cap.lib.wh_capture_clear(cap.h))
            assert cap.size() == 0
            rc, n_new, f = cap.append(np.ascontiguousarray(src), fmt)
            assert rc == 0 and np.array_equal(bits(f[:n_new]), bits(feat))
        # take hands out the mirror and the next append starts at 0
        got_mono, got_stereo = cap.take()
        assert cap.size() == 0
        assert np.array_equal(bits(got_mono), bits(mono)), name
        if keep:
            assert np.array_equal(bits(got_stereo), bits(stereo)), name
        else:
            assert got_stereo is None
        if first is None:
            first = got_mono
    # the two mirrors swap: what a take handed out stays valid while the next piece fills
    rc, _, _ = cap.append(np.ascontiguousarray(src[:5000]), fmt)
    assert rc == 0
    a, _ = cap.take()
    keep_a = a.copy()
    rc, _, _ = cap.append(np.ascontiguousarray(src[7000:16000]), fmt)
    assert rc == 0 and np.array_equal(bits(a), bits(keep_a)) and np.array_equal(bits(a), bits(mono[:5000]))
    b, _ = cap.take()
    assert np.array_equal(bits(b), bits(mono[7000:16000]))


def test_capture_refusals_launch_nothing(captures):
    src, mono, _, _ = source(S16, 1)
    cap = captures(1, False)
    binding.check(cap.lib.wh_capture_clear(cap.h))
    rc, _, _ = cap.append(np.ascontiguousarray(src[:1000]), S16)
    assert rc == 0
    big = np.zeros((N + 4097, 1), np.int16)
    assert cap.append(big, S16)[0] == BOUNDS                                    # 1000 + cap > cap
    assert cap.append(np.ascontiguousarray(src[:256]), 2)[0] == INVALID          # s24
    assert cap.append(np.ascontiguousarray(src[:2000]), S16, feat_cap=1)[0] == INVALID
    n_new = C.c_int64()
    assert cap.lib.wh_capture_append(cap.h, None, S16, 10, None, 0, C.byref(n_new)) == INVALID
    assert cap.lib.wh_capture_append(cap.h, None, S16, 0, None, 0, C.byref(n_new)) == 0 and n_new.value == 0
    assert cap.size() == 1000
    got, _ = cap.take()
    assert np.array_equal(bits(got), bits(mono[:1000]))
    out = C.c_void_p()
    assert cap.lib.wh_capture_create(cap.ctx.handle, 3, 0, N, C.byref(out)) == INVALID and cap.lib.wh_capture_create(cap.ctx.handle, 1, 0, 100, C.byref(out)) == INVALID


# ---- 3. the library, deterministic --------------------------------------------------------------------------------------------------------------------
CHUNK = 1600
RECORDING = {}


def recording():
    """23 s: three pieces of the host-loop tests' recording between gaps of faint noise. On the CPU, with the numpy features of tests/vad_ref.py, the twin
    gives eight pieces of which four end at maxDuration (48000 samples) and three at a pause (32000, 43200, 41600)."""
    if not RECORDING:
        j = _generator().pcm_for("jfk")
        pcm, _ = V.composite([j, j[20000:100000], (0.6 * j[::-1])[:64000]], [0.8, 0.6, 1.0], 40, lead=0.5)
        pcm.setflags(write=False)
        RECORDING["pcm"] = pcm
    return RECORDING["pcm"]


def chunks_of(n):
    return [CHUNK] * (n // CHUNK) + ([n % CHUNK] if n % CHUNK else [])


def twin(mono, flags=R.NO_DROP):
    vad = lambda start, count: api.vad(np.ascontiguousarray(mono[start:start + count]))[1] if count >= 256 else 0
    return R.run(chunks_of(len(mono)), R.Params(flags=flags), vad)


def strip(segs, offset=0):
    return [(s["t0"] - offset, s["t1"] - offset, s["text"], [t["id"] for t in s["tokens"]], [t["p"] for t in s["tokens"]]) for s in segs]


def feed(cap, data):
    for i in range(0, len(data), CHUNK):
        cap.write(data[i:i + CHUNK])
    cap.close()


def check_pieces(m, pieces, mono, need_text=True, **kw):
    """every piece's results are run_full of its samples on a fresh context, the times moved by the piece's start"""
    fresh = m.create_context()
    for key, value in kw.pop("setup", {}).items():
        getattr(fresh, key)(value)
    texts = 0
    for start, count, res in pieces:
        fresh.run_full(np.ascontiguousarray(mono[start:start + count]), flags=api.NO_CONTEXT, **kw)
        want = fresh.results()
        assert strip(res, start * 625) == strip(want), (start, count)
        texts += len(want)
    fresh.close()
    assert texts >= 1 or not need_text
    return texts


def test_run_capture_is_the_twin_and_run_full_piece_by_piece(model):
    m, _ = model
    pcm = recording()
    want = twin(pcm)
    kinds = [b - a for a, b in want["pieces"]]
    print("twin: pieces %s, status %s" % (want["pieces"], want["status"]))
    assert len(kinds) >= 3 and 48000 in kinds and any(32000 <= k < 48000 for k in kinds[:-1]) and want["discarded"] == []
    ctx = m.create_context()
    cap = api.Capture(no_drop=True)
    feed(cap, pcm)
    status = []
    pieces = ctx.run_capture(cap, on_status=status.append, flags=api.NO_CONTEXT)
    assert [(s, s + n) for s, n, _ in pieces] == want["pieces"]
    assert status == want["status"]
    check_pieces(m, pieces, pcm)
    # a second run on the same context, int16 this time: the pieces are the twin's for what 16 bits keep of the samples
    q = np.clip(np.round(pcm * 32768.0), -32768, 32767).astype(np.int16)
    mono16 = q.astype(np.float32) / np.float32(32768.0)
    cap2 = api.Capture(no_drop=True)
    feed(cap2, q)
    pieces2 = ctx.run_capture(cap2, flags=api.NO_CONTEXT)
    assert [(s, s + n) for s, n, _ in pieces2] == twin(mono16)["pieces"]
    check_pieces(m, pieces2, mono16)
    ctx.close()


def test_run_capture_stereo_auto_language_and_suppress(model):
    m, _ = model
    pcm = recording()[:200000]
    # stereo: the left channel carries the speech
    st = np.ascontiguousarray(np.stack([pcm, np.float32(0.25) * pcm[::-1]], axis=1))
    mono = (st[:, 0] + st[:, 1]) * np.float32(0.5)
    ctx = m.create_context()
    cap = api.Capture(no_drop=True, stereo=True)
    feed(cap, st)
    speakers = []
    pieces = ctx.run_capture(cap, on_piece=lambda s, n, res: speakers.append(ctx.speakers()), flags=api.NO_CONTEXT)
    assert [(s, s + n) for s, n, _ in pieces] == twin(mono)["pieces"] and len(pieces) >= 3
    fresh = m.create_context()
    for (start, count, res), sp in zip(pieces, speakers):
        fresh.run_full(np.ascontiguousarray(mono[start:start + count]), flags=api.NO_CONTEXT, stereo=np.ascontiguousarray(st[start:start + count]))
        assert strip(res, start * 625) == strip(fresh.results()) and sp == fresh.speakers() and len(sp) == len(res)
    assert any(s not in (api.NO_STEREO_DATA,) for sp in speakers for s in sp)
    fresh.close()
    # language "auto" and a suppress set hold for every piece
    cap = api.Capture(no_drop=True)
    feed(cap, pcm)
    pieces = ctx.run_capture(cap, language="auto", flags=api.NO_CONTEXT)
    check_pieces(m, pieces, pcm, language="auto")
    plain = [t["id"] for _, _, res in pieces for s in res for t in s["tokens"]]
    eot = m.special_tokens()["eot"]
    text = [t for t in plain if t < eot]
    ban = sorted(set(text))[: max(1, len(set(text)) // 2)]
    ctx.set_suppress_tokens(ban)
    cap = api.Capture(no_drop=True)
    feed(cap, pcm)
    pieces = ctx.run_capture(cap, flags=api.NO_CONTEXT)
    got = [t["id"] for _, _, res in pieces for s in res for t in s["tokens"]]
    assert not set(got) & set(ban)
    check_pieces(m, pieces, pcm, setup={"set_suppress_tokens": ban})
    ctx.close()


# ---- 4. the library, timing-dependent mode ---------------------------------------------------------------------------------------------------------------
def test_run_capture_without_no_drop_properties_and_cancel(model):
    m, _ = model
    pcm = recording()
    ctx = m.create_context()
    # max_duration 30 s: the queue's limit (max_duration + 1 s) is above the recording's length, so the writer, which is much faster than real time, never
    # makes it drop a chunk -- a dropped chunk is not part of the stream's clock -- and the spans below are spans of pcm. Which pieces form depends on when
    # the jobs end.
    cap = api.Capture(max_duration=30.0)
    writer = threading.Thread(target=feed, args=(cap, pcm))
    status = []
    writer.start()
    pieces = ctx.run_capture(cap, on_status=status.append, flags=api.NO_CONTEXT)
    writer.join()
    assert cap.dropped_chunks() == 0 and len(pieces) >= 1
    assert status[0] == api.LISTENING and not status[-1] & api.TRANSCRIBING
    spans = [(s, s + n) for s, n, _ in pieces]
    assert all(0 <= a < b <= len(pcm) for a, b in spans) and all(p[1] <= q[0] for p, q in zip(spans, spans[1:]))
    check_pieces(m, pieces, pcm)
    # should_cancel after the first piece: success; the loop joins its worker before it returns, which the next run on the same context depends on (a job
    # still running would share the context's device state with it and the piece-by-piece comparison below would not hold)
    cap = api.Capture(no_drop=True)
    feed(cap, pcm)
    done = []
    pieces = ctx.run_capture(cap, on_piece=lambda s, n, res: done.append(s), should_cancel=lambda: bool(done), flags=api.NO_CONTEXT)
    assert 1 <= len(pieces) <= 2
    check_pieces(m, pieces, pcm)
    cap = api.Capture(no_drop=True)
    feed(cap, pcm[:100000])
    again = ctx.run_capture(cap, flags=api.NO_CONTEXT)
    assert [(s, s + n) for s, n, _ in again] == twin(pcm[:100000])["pieces"]
    # the keywords of run_full hold for every piece
    prompt = [t["id"] for t in again[0][2][0]["tokens"] if t["id"] < m.special_tokens()["eot"]][:3]
    for kw in (dict(max_tokens=2), dict(prompt=prompt, n_max_text_ctx=8), dict(audio_ctx=512)):
        cap = api.Capture(no_drop=True)
        feed(cap, pcm[:100000])
        got = ctx.run_capture(cap, flags=api.NO_CONTEXT, **kw)
        assert [(s, s + n) for s, n, _ in got] == [(s, s + n) for s, n, _ in again]
        check_pieces(m, got, pcm, need_text=False, **kw)        # two tokens per segment leave this model no segment at all: on both sides
        if "prompt" not in kw:
            assert [strip(r) for _, _, r in got] != [strip(r) for _, _, r in again], kw       # the keyword reached the pieces
    ctx.close()


def test_run_capture_refusals(model):
    m, _ = model
    ctx = m.create_context()
    with pytest.raises(api.WhisperError) as e:
        ctx.run_capture(None)
    assert e.value.hr == 0x80004003
    for kw in (dict(min_duration=0.1), dict(max_duration=30.5), dict(min_duration=float("nan"))):
        with pytest.raises(api.WhisperError) as e:
            ctx.run_capture(api.Capture(**kw))
        assert e.value.hr == 0x80070057, kw
    # an empty stream is no error
    cap = api.Capture()
    cap.close()
    assert ctx.run_capture(cap) == []
    ctx.close()


# ---- 5. flat C and the command-line tool ----------------------------------------------------------------------------------------------------------------
def test_flat_c_equals_the_python_face(model):
    m, _ = model
    pcm = recording()[:200000]
    ctx = m.create_context()
    cap = api.Capture(no_drop=True)
    feed(cap, pcm)
    want = ctx.run_capture(cap, flags=api.NO_CONTEXT)
    lib = api.lib()
    h = C.c_void_p()
    assert lib.whisperc_capture_create(2.0, 3.0, 0.25, 0.333, api.CAPTURE_NO_DROP, C.byref(h)) == 0
    for i in range(0, len(pcm), CHUNK):
        part = np.ascontiguousarray(pcm[i:i + CHUNK])
        assert lib.whisperc_capture_write(h, part.ctypes.data_as(C.c_void_p), F32, 1, len(part)) == 0
    assert lib.whisperc_capture_close(h) == 0
    got, words = [], []
    piece_t = C.CFUNCTYPE(None, C.c_void_p, C.c_int64, C.c_int64)
    status_t = C.CFUNCTYPE(C.c_int32, C.c_void_p, C.c_uint8)
    on_piece = piece_t(lambda pv, s, n: got.append((s, n, ctx.results())))
    on_status = status_t(lambda pv, w: words.append(w) or 0)
    assert lib.whisperc_run_capture(ctx.h, h, b"en", api.NO_CONTEXT, None, C.cast(on_status, C.c_void_p), C.cast(on_piece, C.c_void_p), None) == 0
    lib.whisperc_capture_destroy(h)
    assert [(s, n, strip(r)) for s, n, r in got] == [(s, n, strip(r)) for s, n, r in want] and len(got) >= 3
    assert words == twin(pcm)["status"]
    ctx.close()


def test_whisper_main_capture(model, tmp_path):
    m, path = model
    pcm = recording()[:200000]
    q = np.clip(np.round(pcm * 32768.0), -32768, 32767).astype("<i2")
    mono16 = q.astype(np.float32) / np.float32(32768.0)
    raw = str(tmp_path / "stream.s16")
    q.tofile(raw)
    r = subprocess.run([build.CLI_BIN, "-m", path, "--capture", raw, "--capture-no-drop", "-nc"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=240)
    print(r.stdout.decode()[-2000:], r.stderr.decode()[-1500:])
    assert r.returncode == 0
    lines = [ln for ln in r.stdout.decode().splitlines() if ln.startswith("[")]
    ctx = m.create_context()
    want = []
    for a, b in twin(mono16)["pieces"]:
        ctx.run_full(np.ascontiguousarray(mono16[a:b]), flags=api.NO_CONTEXT)
        want += [(s["t0"] + a * 625, s["t1"] + a * 625, s["text"].decode()) for s in ctx.results()]
    ctx.close()
    assert len(lines) == len(want) >= 3
    seconds = lambda hms: int(hms[0:2]) * 3600 + int(hms[3:5]) * 60 + float(hms[6:12])
    for ln, (t0, t1, text) in zip(lines, want):
        # "[hh:mm:ss.mmm --> hh:mm:ss.mmm]  text": media times, i.e. the piece's start added, in the existing console format
        assert ln[0] == "[" and ln[13:18] == " --> " and ln[30] == "]", ln
        assert ln.endswith("]  " + text), (ln, text)
        assert abs(seconds(ln[1:13]) - t0 / 1e7) < 0.0011 and abs(seconds(ln[18:30]) - t1 / 1e7) < 0.0011, (ln, t0, t1)
    assert any(t0 >= 30000000 for t0, _, _ in want)         # pieces that begin well into the stream
