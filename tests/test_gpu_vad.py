"""GPU tests of the voice-activity features (whisper_amd/csrc/vad.hip; wh_vad_features of include/whisper_hip.h) and of what sits on top of them:
api.vad, api.plan_chunks, BatchRunner.run_split and whisper-mgpu -split silence.

The features are defined as those of the exact DFT, evaluated in FP64 and rounded once to float, so the reference is the numpy restatement of
tests/vad_ref.py (np.fft.fft in float64). Bounds: energy within one float32 ulp, F equal, SFM within two float32 ulps plus four times the float64 floor
-- the largest difference between the restatement fed np.fft.fft and the same formulas fed a direct float64 DFT matrix product on the same input,
measured here and printed --, NaN where the restatement has NaN. Frames whose two largest |X|^2 of bins 0 .. 127 differ by less than 1e-9 relative, or that
hold a non-zero bin below 1e-7 of the frame's norm, are left out of the F and SFM comparisons (never of the energy's); they may be at most 1 % of a case.
Sources sit inside larger device buffers whose surroundings are NaN, destinations between 64 NaN floats that must stay NaN."""
import ctypes as C
import importlib.util
import json
import os
import subprocess
import wave

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import vad_ref as V  # noqa: E402
from whisper_amd import api, binding, build, ggml_format as gf  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 64                  # floats of NaN on both sides of a destination
T = 16                      # frames per workgroup of vadFeaturesKernel
FRAME_COUNTS = (0, 1, T - 1, T, T + 1, 2 * T + 1, 1000)
MARGIN_ULPS = 64
INVALID = -1                # WH_E_INVALIDARG


def device_features(pcm, n_samples, front=37):
    """wh_vad_features on pcm[:n_samples] placed `front` floats into a buffer of NaN, into a guarded destination"""
    n_frames = n_samples // 256
    buf = np.full(front + n_samples + 300, np.nan, np.float32)
    buf[front:front + n_samples] = pcm[:n_samples]
    src = torch.from_numpy(buf).cuda()
    dst = torch.full((2 * GUARD + 3 * n_frames,), float("nan"), dtype=torch.float32, device="cuda")
    binding.check(binding.lib().wh_vad_features(None, C.c_void_p(src.data_ptr() + 4 * front), n_samples, C.c_void_p(dst.data_ptr() + 4 * GUARD)))
    torch.cuda.synchronize()
    out = dst.cpu().numpy()
    assert np.isnan(out[:GUARD]).all() and np.isnan(out[GUARD + 3 * n_frames:]).all(), "write outside the destination"
    return out[GUARD:GUARD + 3 * n_frames].reshape(n_frames, 3).copy()


def make_input(kind):
    """1000 frames and 255 samples of tail"""
    n = 1000 * 256 + 255
    rng = np.random.default_rng({"noise": 1, "tones": 2, "jfk": 3, "zeros": 4, "full_scale": 5}[kind])
    if kind == "noise":
        return rng.uniform(-1, 1, n).astype(np.float32)
    if kind == "tones":         # two tones off the bin centres (bins 7.3 and 41.6) in noise
        t = np.arange(n)
        return (0.4 * np.sin(2 * np.pi * 7.3 * t / 256 + 0.3) + 0.25 * np.sin(2 * np.pi * 41.6 * t / 256 + 1.1) + 0.01 * rng.standard_normal(n)).astype(np.float32)
    if kind == "jfk":           # begins with frames of exact zeros; integer-valued samples
        j = V.jfk_pcm()
        return np.concatenate([j, 0.7 * j[::-1]])[:n].astype(np.float32)
    if kind == "zeros":         # frames of exact zeros between live frames, and frames that are zero in part
        x = (0.1 * rng.standard_normal(n)).astype(np.float32).reshape(-1)
        for f in (0, 3, 4, 15, 16, 17, 40, 998, 999):
            x[f * 256:(f + 1) * 256] = 0
        x[20 * 256:20 * 256 + 100] = 0
        x[33 * 256 + 200:34 * 256] = 0
        return x
    if kind == "full_scale":    # +-1: x = +-32768, the largest sums
        return rng.choice(np.array([-1.0, 1.0], np.float32), n)
    raise KeyError(kind)


REFERENCE = {}


def reference(kind):
    """pcm, the restatement's features and fragile frames, and the float64 floor of SFM: computed once per input, shared by the tests, left unchanged"""
    if kind not in REFERENCE:
        pcm = make_input(kind)
        feat, power = V.features(pcm)
        direct, _ = V.features(pcm, dft=V.dft_direct)
        both = np.isfinite(feat[:, 2]) & np.isfinite(direct[:, 2])
        sfm64 = []
        for dft in (V.dft_fft, V.dft_direct):
            mag = np.abs(dft(V.frames_of(pcm)[both]))
            sfm64.append(-10.0 * np.log10(np.exp(np.log(mag).sum(1) / 256) / (mag.sum(1) / 256)))
        fragile = V.fragile_frames(power)
        floor = float(np.abs(sfm64[0] - sfm64[1])[~fragile[both]].max())
        for a in (pcm, feat, fragile):
            a.setflags(write=False)
        REFERENCE[kind] = (pcm, feat, fragile, floor)
    return REFERENCE[kind]


def compare(got, want, fragile, floor, what):
    assert got.shape == want.shape, what
    if len(want) == 0:
        return 0.0, 0.0
    ulp = lambda a: np.spacing(np.abs(a).astype(np.float32)).astype(np.float64)
    # energy: every frame
    e_err = np.abs(got[:, 0].astype(np.float64) - want[:, 0]) / ulp(want[:, 0])
    assert (e_err <= 1).all(), (what, "energy", int(np.argmax(e_err)), float(e_err.max()))
    keep = ~fragile
    assert np.array_equal(got[keep, 1], want[keep, 1]), (what, "F", np.flatnonzero(got[:, 1] != want[:, 1])[:5])
    g, w = got[keep, 2], want[keep, 2]
    assert np.array_equal(np.isnan(g), np.isnan(w)), (what, "NaN", np.flatnonzero(np.isnan(g) != np.isnan(w))[:5])
    assert np.array_equal(np.isinf(g), np.isinf(w)) and (g[np.isinf(w)] == w[np.isinf(w)]).all(), (what, "inf")
    fin = np.isfinite(w)
    s_err = np.abs(g[fin].astype(np.float64) - w[fin])
    bound = 2 * ulp(w[fin]) + 4 * floor
    assert (s_err <= bound).all(), (what, "SFM", int(np.argmax(s_err - bound)), float((s_err / bound).max()))
    return float(e_err.max()), float((s_err / bound).max()) if fin.any() else 0.0


# ---- 5. features against the restatement ----------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["noise", "tones", "jfk", "zeros", "full_scale"])
def test_features_against_the_restatement(kind):
    pcm, want, fragile, floor = reference(kind)
    print("%s: float64 floor of SFM %.3g dB, %d fragile frames of %d, %d NaN, %d infinite" %
          (kind, floor, int(fragile.sum()), len(want), int(np.isnan(want[:, 2]).sum()), int(np.isinf(want[:, 2]).sum())))
    assert floor <= 1e-9
    if kind in ("jfk", "zeros"):
        zero = want[:, 0] == 0
        assert zero.sum() >= 2 and np.isnan(want[zero, 2]).all() and (want[zero, 1] == 0).all()
    # the frames left out of the F and SFM comparisons: at most 1 % of the case
    assert fragile.mean() <= 0.01, int(fragile.sum())
    worst = (0.0, 0.0)
    for frames in FRAME_COUNTS:
        for tail in (0, 255):
            got = device_features(pcm, 256 * frames + tail)
            e, s = compare(got, want[:frames], fragile[:frames], floor, (kind, frames, tail))
            worst = (max(worst[0], e), max(worst[1], s))
    print("   worst energy error %.2f ulp, worst SFM error %.2f of its bound" % worst)


def test_features_refuses_bad_calls():
    lib = binding.lib()
    n = C.c_int64(-7)
    for samples, frames in ((0, 0), (255, 0), (256, 1), (2 ** 33 + 511, 2 ** 25 + 1)):
        binding.check(lib.wh_vad_frame_count(samples, C.byref(n)))
        assert n.value == frames
    assert lib.wh_vad_frame_count(-1, C.byref(n)) == INVALID and lib.wh_vad_frame_count(2 ** 40 + 1, C.byref(n)) == INVALID
    buf = torch.zeros(1024, dtype=torch.float32, device="cuda")
    p = buf.data_ptr()
    assert lib.wh_vad_features(None, None, 255, None) == 0                               # no frames: nothing is touched
    assert lib.wh_vad_features(None, None, 256, C.c_void_p(p)) == INVALID
    assert lib.wh_vad_features(None, C.c_void_p(p), 256, None) == INVALID
    assert lib.wh_vad_features(None, C.c_void_p(p + 2), 256, C.c_void_p(p + 2048)) == INVALID
    assert lib.wh_vad_features(None, C.c_void_p(p), -1, C.c_void_p(p + 2048)) == INVALID
    assert lib.wh_vad_features_host(None, 256, None) == INVALID
    assert lib.wh_vad_features_host(None, 100, None) == 0
    # the host entry point is the device's
    pcm, want, _, _ = reference("noise")
    got = np.full((40, 3), np.nan, np.float32)
    binding.check(lib.wh_vad_features_host(pcm[:256 * 40 + 17].ctypes.data_as(C.c_void_p), 256 * 40 + 17, got.ctypes.data_as(C.c_void_p)))
    assert np.array_equal(got, device_features(pcm, 256 * 40 + 17))


# ---- 6. the sums do not depend on the block shape -------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["noise", "jfk"])
def test_features_are_bit_identical_wherever_the_frame_sits(kind):
    """The same frames at two buffer offsets, in calls of two lengths, and as other rows of other workgroups (the call that starts 5 frames later sees
    frame 5 as its frame 0): the same bits."""
    pcm = reference(kind)[0]
    whole = device_features(pcm, 256 * 1000 + 255, front=37)
    assert np.array_equal(whole.view(np.uint32), device_features(pcm, 256 * 1000 + 255, front=64).view(np.uint32))
    short = device_features(pcm, 256 * 40, front=41)
    assert np.array_equal(short.view(np.uint32), whole[:40].view(np.uint32))
    for shift in (5, 16, 27):
        moved = device_features(pcm[256 * shift:], 256 * (T + 2), front=33)
        assert np.array_equal(moved.view(np.uint32), whole[shift:shift + T + 2].view(np.uint32)), shift


# ---- 7. api.vad -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["composite", "zeros_in_the_middle"])
def test_api_vad_against_the_restatement(name):
    pcm = V.recordings()[name]
    feat, _ = V.features(pcm)
    want, want_last, margin = V.decide(feat)
    print("%s: %d frames, %d speech, smallest margin %.1f ulps" % (name, len(want), int(want.sum()), margin))
    assert margin > MARGIN_ULPS
    got, last = api.vad(pcm)
    assert got.dtype == np.uint8 and np.array_equal(got, want) and last == want_last


def test_api_vad_resamples_first():
    pcm8k = np.ascontiguousarray(V.recordings()["speech_first"][::2][:80000])
    a, a_last = api.vad(pcm8k, 8000)
    b, b_last = api.vad(api.resample(pcm8k, 8000))
    assert len(a) == 2 * len(pcm8k) // 256 and np.array_equal(a, b) and a_last == b_last and 0 < a.sum() < len(a)
    none, none_last = api.vad(np.zeros(100, np.float32))
    assert len(none) == 0 and none_last == 0


# ---- 8. end to end ----------------------------------------------------------------------------------------------------------
def _generator():
    spec = importlib.util.spec_from_file_location("make_golden_runfull", os.path.join(ROOT, "tests", "golden", "make_golden_runfull.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def strip(segs):
    return [(s["t0"], s["t1"], s["text"], [t["id"] for t in s["tokens"]], [t["p"] for t in s["tokens"]]) for s in segs]


def test_split_at_pauses_end_to_end(tmp_path):
    """A 70 s recording of pcm_for pieces and 0.8 s gaps of faint noise: a piece straddles 30 s and another 60 s, a gap lies in (15 s, 30 s] and another
    in (cut1 + 15 s, cut1 + 30 s], each followed by a piece that does not pause before the window's end. plan_chunks is the restatement's plan and cuts
    inside the gaps; run_split is run over those pieces, segment for segment, and not what the fixed 30 s split gives; whisper-mgpu -split silence prints
    it, whisper-mgpu without the option prints the fixed split's transcript."""
    mg = _generator()
    S = 16000
    pieces = [mg.pcm_for("quiet"), mg.pcm_for("jfk"), mg.pcm_for("mixed")[:int(15.3 * S)], mg.pcm_for("jfk"), mg.pcm_for("jfk")[::2][:int(1.7 * S)]]
    raw, spans = V.composite(pieces, [0.8, 0.8, 0.8, 0.8, 0], 40, lead=0.3)
    # what a 16-bit WAV file holds
    q = np.clip(np.round(raw * 32768.0), -32768, 32767).astype("<i2")
    pcm = q.astype(np.float32) / np.float32(32768.0)
    n = len(pcm)
    assert n == 70 * S and any(a < 30 * S < b for a, b in _piece_spans(spans, n)) and any(a < 60 * S < b for a, b in _piece_spans(spans, n))

    feat, _ = V.features(pcm)
    speech, _, margin = V.decide(feat)
    rules = []
    want_plan = V.plan(speech, feat[:, 0], n, rules=rules)
    print("margin %.1f ulps, plan %s, rules %s, gaps %s" % (margin, want_plan, rules, spans))
    assert margin > MARGIN_ULPS
    plan = api.plan_chunks(pcm)
    assert plan == want_plan and len(plan) == 3
    cut1, cut2 = plan[1][0], plan[2][0]
    assert any(a <= cut1 <= b and 15 * S < a and b <= 30 * S for a, b in spans), (cut1, spans)
    assert any(a <= cut2 <= b and cut1 + 15 * S < a and b <= cut1 + 30 * S for a, b in spans), (cut2, spans)
    # other parameters reach the planner; bad ones are refused
    assert api.plan_chunks(pcm, max_len=20 * S, min_len=8 * S) == V.plan(speech, feat[:, 0], n, max_len=20 * S, min_len=8 * S)
    assert api.plan_chunks(pcm[:30 * S]) == [(0, 30 * S)]
    with pytest.raises(api.WhisperError):
        api.plan_chunks(pcm, max_len=480001)

    path = str(tmp_path / "cond.bin")
    gf.write_model(path, mg.model_for(10))
    m = api.Model(path)
    runner = m.create_batch_runner(max_slots=4, groups=1)
    hr, got, per, got_plan = runner.run_split(pcm)
    assert hr == 0 and got_plan == plan
    hr2, want, per2 = runner.run([(pcm, f, c) for f, c in plan], flags=api.NO_CONTEXT)
    assert hr2 == 0 and per == per2 and len(got) == len(want) == 3
    for g, w in zip(got, want):
        assert strip(g) == strip(w) and len(w) >= 1
    # times are relative to the buffer: a piece's segments lie inside it
    for (f, c), g in zip(plan, got):
        assert all(f * 625 <= s["t0"] <= (f + c) * 625 and s["t0"] <= s["t1"] for s in g), (f, c)
    fixed_pieces = [(k * 30 * S, min(30 * S, n - k * 30 * S)) for k in range(3)]
    _, fixed, _ = runner.run([(pcm, f, c) for f, c in fixed_pieces], flags=api.NO_CONTEXT)
    text = lambda res: [s["text"].decode() for r in res for s in r]
    assert text(got) != text(fixed)
    runner.close()
    m.close()

    wav = str(tmp_path / "rec.wav")
    with wave.open(wav, "wb") as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(16000)
        w.writeframes(q.tobytes())
    for option, res, pieces_n in ((["-split", "silence"], got, 3), ([], fixed, 3), (["-split", "fixed"], fixed, 3)):
        out = str(tmp_path / ("t%d.txt" % len(option)))
        r = subprocess.run([build.MGPU_BIN, "-n", "1", "-m", path, "-f", wav, "-o", out, "-timeout", "60", "-job-timeout", "240"] + option,
                           stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
        print(r.stdout.decode(), r.stderr.decode()[-1500:])
        assert r.returncode == 0
        line = json.loads(r.stdout.decode().strip().splitlines()[-1])
        assert line["windows"] == pieces_n and line.get("split") == ("silence" if option[-1:] == ["silence"] else None)
        lines = open(out).read().splitlines()
        segs = [s for r_ in res for s in r_]
        assert len(lines) == len(segs)
        for ln, s in zip(lines, segs):
            assert ln.endswith("] " + s["text"].decode()), (ln, s["text"])
            t0, t1 = float(ln[1:10]), float(ln[15:24])
            assert abs(t0 - s["t0"] / 1e7) < 0.006 and abs(t1 - s["t1"] / 1e7) < 0.006


def _piece_spans(gaps, n):
    """the pieces between the gaps"""
    edges = [0] + [e for a, b in gaps for e in (a, b)] + [n]
    return [(edges[i], edges[i + 1]) for i in range(0, len(edges), 2) if edges[i + 1] > edges[i]]
