"""GPU tests of the FP8 cross-attention caches (whisper_amd/csrc/kv8.hip; DESIGN.md section 7 "FP8 cross-attention caches"): the quantizer bit for bit against
the numpy statement of the format (tests/cross_fp8_ref.py), the caches of an FP8 context against the quantized caches of an FP16 context, attentionDecG8 against
float64 on the dequantized values, a decode step end to end against the FP16 context, and the public face with its refusals."""
import ctypes as C
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import cross_fp8_ref as f8  # noqa: E402
import decode_step_ref as ds  # noqa: E402
from oracle import whisper_np as wn  # noqa: E402
from whisper_amd import binding, ggml_format as gf  # noqa: E402

pytestmark = pytest.mark.gpu
F32 = np.float32


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


# ---------------------------------------------------------------------------------------------------------------------
# 1. the quantizer
# ---------------------------------------------------------------------------------------------------------------------
TIES = [448, 17, 19, 1.0625, 1.1875, 2.0 ** -10, 3 * 2.0 ** -10]          # s = 1: halfway between two E4M3 values each ...
TIES_WANT = [448, 16, 20, 1.0, 1.25, 0.0, 2.0 ** -8]                      # ... and the neighbour with the even mantissa


@functools.lru_cache(None)
def _row_pool():
    """64 rows: the edge cases of the format, then seeded normal rows of several magnitudes."""
    rng = np.random.default_rng(8)
    base = lambda: (0.3 * rng.standard_normal(64)).astype(np.float16)          # noqa: E731
    rows = [np.zeros(64, np.float16), np.where(np.arange(64) % 3 == 0, -0.0, 0.0).astype(np.float16)]
    for k in (-3, 0, 5):                                                        # amax exactly 448 * 2^k, and one FP16 ulp above: the exponent steps
        for top in (np.float16(448 * 2.0 ** k), np.nextafter(np.float16(448 * 2.0 ** k), np.float16(np.inf))):
            r = base() * np.float16(2.0 ** k)
            r[rng.integers(64)] = top * (-1) ** k
            rows.append(r)
    sub = rng.integers(1, 1024, 64).astype(np.uint16) | (rng.integers(0, 2, 64) << 15).astype(np.uint16)
    rows.append(sub.view(np.float16))                                           # FP16 subnormals only
    r = base()
    r[5] = -65504
    rows.append(r)
    r = np.zeros(64, np.float16)
    r[:len(TIES)] = TIES
    rows.append(r)
    while len(rows) < 64:
        rows.append((rng.standard_normal(64) * 10.0 ** rng.uniform(-4, 3)).astype(np.float16))
    return np.stack(rows)


@pytest.mark.parametrize("n", [1, 7, 8, 9, 127, 128, 129, 1500])
def test_quantizer_bit_for_bit(n):
    """wh_op_quantize_kv == the helper, bytes and scales, at row counts around what a wave (8 rows) and a workgroup (128) cover; the row behind the last stays
    as it was."""
    pool = _row_pool()
    x = pool[(np.arange(n) + n) % 64]
    out_b = torch.full((n + 1, 64), 0xAA, dtype=torch.uint8, device="cuda")
    out_s = torch.full((n + 1,), float("nan"), dtype=torch.float32, device="cuda")
    binding.check(binding.lib().wh_op_quantize_kv(None, ptr(dev(x)), ptr(out_b), ptr(out_s), n))
    torch.cuda.synchronize()
    gb, gs = out_b.cpu().numpy(), out_s.cpu().numpy()
    wb, ws = f8.quantize_rows(x)
    assert np.array_equal(gs[:n], ws) and np.array_equal(gb[:n], wb)
    assert (gb[n] == 0xAA).all() and np.isnan(gs[n])
    if n >= 64:                                                                # the row of ties (row 10 of the pool), without the helper
        i = (10 - n) % 64
        assert gs[i] == 1.0 and np.array_equal(f8.dequantize(gb[i], gs[i])[:len(TIES)], np.asarray(TIES_WANT))


# ---------------------------------------------------------------------------------------------------------------------
# 2. FP8 cache == quantize( FP16 cache )
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def toy(tiny_model, golden):
    m = binding.HipModel.from_ggml(tiny_model)
    rng = np.random.default_rng(5)
    mel = np.stack([np.roll(golden["mel"], 37 * b, axis=1) + 0.01 * rng.standard_normal(golden["mel"].shape).astype(F32) for b in range(3)]).astype(F32)
    yield m, tiny_model.hparams, torch.from_numpy(mel).cuda()
    m.close()


def _contexts(m, max_batch, enc_chunk=128):
    binding.set_option("enc_chunk", enc_chunk)
    try:
        return binding.HipContext(m, max_batch), binding.HipContext(m, max_batch, cross_fp8=True)
    finally:
        binding.set_option("enc_chunk", 128)


@pytest.mark.parametrize("audio_ctx,enc_chunk", [(0, 128), (130, 128), (0, 2)])
def test_cache_identity(toy, audio_ctx, enc_chunk):
    """The same wh_encode of 3 windows on an FP16 and on an FP8 context: bytes and scales of the first and last decoder layer are the helper's quantization of
    the FP16 caches. Covers the per-layer product, a changed audio context, and the window offsets of an encode in chunks of 2 + 1."""
    m, hp, mel = toy
    c16, c8 = _contexts(m, 3, enc_chunk)
    T, H = audio_ctx or hp.n_audio_ctx, hp.n_audio_head
    for c in (c16, c8):
        c.set_audio_ctx(audio_ctx)
        c.encode(mel, offsets=[0, 7, 30])
    for il in (0, hp.n_text_layer - 1):
        for name in ("k", "v"):
            rows = c16.debug_read("cross-" + name, il).reshape(-1)[:3 * T * H * 64].reshape(3, T, H, 64).transpose(0, 2, 1, 3)
            wb, ws = f8.quantize_rows(rows.astype(np.float16))
            assert float(np.abs(rows).max()) > 0.05
            assert np.array_equal(c8.debug_read("cross-%s8-scale" % name, il), ws), (il, name)
            assert np.array_equal(c8.debug_read("cross-%s8" % name, il), wb), (il, name)
    c16.close()
    c8.close()


# ---------------------------------------------------------------------------------------------------------------------
# 3. attentionDecG8 against float64 on the dequantized values
# ---------------------------------------------------------------------------------------------------------------------
WINDOWS = 3


@functools.lru_cache(4)
def _caches(H, n_keys):
    """K and V of 3 windows as bytes and scales: values of unit size under scales 2^-10 .. 2^6 chosen per row (bytes clipped to +-448), rows behind the last
    key NaN. Returns device tensors and the float64 values."""
    rng = np.random.default_rng(H * 10000 + n_keys)
    out = []
    for gain in (0.8, 1.0):
        s = np.ldexp(1.0, rng.integers(-10, 7, (WINDOWS, H, n_keys + 3))).astype(F32)
        x = np.clip(gain * rng.standard_normal((WINDOWS, H, n_keys + 3, 64)) / s[..., None], -448, 448).astype(F32)
        b = torch.from_numpy(x).to(torch.float8_e4m3fn).view(torch.uint8).numpy().copy()
        b[:, :, n_keys:] = 0x7F
        s[:, :, n_keys:] = np.nan
        out += [dev(b), dev(s), f8.dequantize(b[:, :, :n_keys], s[:, :, :n_keys])]
    return out


@pytest.mark.parametrize("n_tok", [1, 3])
@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("group", [1, 2, 5, 8])
@pytest.mark.parametrize("H", [2, 20])
@pytest.mark.parametrize("n_keys", [1, 15, 16, 17, 127, 128, 129, 1499, 1500])
def test_attention_against_float64(n_keys, H, group, fused, n_tok):
    """wh_op_decoder_cross_attention_f8 against the float64 restatement evaluated on bytes x scale (exact in float64: the quantization error is not in the
    comparison), at the bounds test_gpu_decode_step_ops.py holds wh_op_decoder_cross_attention to against its float64 reference: 4e-3 max, 3e-4 mean. Measured
    with the packed-FP16 dot: see DESIGN.md section 7 "FP8 cross-attention caches"."""
    d = H * 64
    kb, ks, k64, vb, vs, v64 = _caches(H, n_keys)
    rows = WINDOWS * group * n_tok
    rng = np.random.default_rng(n_keys * 100 + group * 10 + n_tok)
    scale = F32(64.0 ** -0.25)
    if fused:
        x = (rng.standard_normal((rows, d)) * 2 + 0.3).astype(F32)
        lnw, lnb = (1 + 0.1 * rng.standard_normal(d)).astype(F32), (0.1 * rng.standard_normal(d)).astype(F32)
        wq, bq = (rng.standard_normal((d, d), dtype=F32) / np.sqrt(d)).astype(np.float16), (0.1 * rng.standard_normal(d)).astype(F32)
        q = ds.cross_query(x, lnw, lnb, wq, bq, scale)
        ops = [None] + [dev(t) for t in (x, lnw, lnb, wq, bq)]
    else:
        q = rng.standard_normal((rows, d), dtype=F32).astype(np.float16).astype(F32)
        ops = [dev(q.astype(np.float16))] + [None] * 5
    out = torch.full((rows + 1, d), float("nan"), dtype=torch.float16, device="cuda")
    binding.check(binding.lib().wh_op_decoder_cross_attention_f8(None, *[ptr(t) for t in ops], C.c_float(float(scale)), ptr(kb), ptr(ks), ptr(vb), ptr(vs), ptr(out),
                                                                 WINDOWS * group, H, n_tok, n_keys, n_keys + 3, group))
    torch.cuda.synchronize()
    got = out.cpu().numpy().astype(F32)
    want = np.zeros((rows, d), F32)
    per = group * n_tok                                                        # rows of a window: sequence-major, then token
    for w in range(WINDOWS):
        qw = q[w * per:(w + 1) * per].reshape(per, H, 64).astype(np.float64)
        s32 = np.einsum("rhj,hkj->rhk", qw, k64[w]).astype(F32)
        e = wn.exp16((s32 - s32.max(axis=2, keepdims=True)).astype(F32)).astype(np.float64)
        want[w * per:(w + 1) * per] = wn.r16(np.einsum("rhk,hkj->rhj", e, v64[w]) / e.sum(axis=2, keepdims=True)).reshape(per, d)
    dd = np.abs(got[:rows] - want)
    print("   keys %d H %d group %d fused %d nTok %d: max|diff| %.2e (bound 4e-3) mean %.2e (bound 3e-4)" % (n_keys, H, group, fused, n_tok, dd.max(), dd.mean()))
    assert np.isnan(got[rows]).all(), "the row behind the last was written"
    assert np.isfinite(got[:rows]).all() and dd.max() < 4e-3 and dd.mean() < 3e-4


# ---------------------------------------------------------------------------------------------------------------------
# 4. a decode step end to end, 5. the public face
# ---------------------------------------------------------------------------------------------------------------------
LOGIT_MAX_RECORDED = 3.644e-3       # max |logit( FP8 context ) - logit( FP16 context )| measured once on an MI355X (mean 5.14e-4, largest |logit| 2.45); the bound is 4 x this


def test_decode_steps_against_the_fp16_context(toy):
    """The prompt step and three single-token steps of 3 windows, the same tokens fed to both contexts after the same wh_encode. The bound is measured, not
    guessed: 4 x the recorded maximum (the kernels are deterministic; the margin is for a compiler or driver change). The project's own scale for such a
    number: the reference moves 0.05 .. 0.5 on logits between thread counts."""
    m, hp, mel = toy
    c16, c8 = _contexts(m, 3)
    sp = gf.special_tokens(hp)
    steps = [np.array([[sp["sot"], sp["transcribe"], sp["not_"]]] * 3, np.int32)] + [np.array([[100 + 7 * i + b] for b in range(3)], np.int32) for i in range(3)]
    worst, means, n_past = 0.0, [], 0
    for c in (c16, c8):
        c.encode(mel)
    for t in steps:
        l16, l8 = c16.decode(t, n_past)[0], c8.decode(t, n_past)[0]
        assert np.isfinite(l8).all()
        worst, n_past = max(worst, float(np.abs(l8 - l16).max())), n_past + t.shape[1]
        means.append(float(np.abs(l8 - l16).mean()))
    print("FP8 against FP16 context, 4 steps x 3 windows: max |d logit| %.3e, mean %.3e (max |logit| %.2f)" % (worst, np.mean(means), float(np.abs(l16).max())))
    assert worst > 0 and worst < 4 * LOGIT_MAX_RECORDED
    c16.close()
    c8.close()


def _pcm(seconds, tone, seed):
    t = np.arange(int(seconds * 16000)) / 16000.0
    return (0.25 * np.sin(2 * np.pi * tone * t) * (1 + 0.6 * np.sin(2 * np.pi * 2.5 * t)) + 0.05 * np.random.default_rng(seed).standard_normal(len(t))).astype(F32)


def test_batch_runner_with_fp8_caches(tmp_path):
    """BatchRunner( flags = BATCH_CROSS_FP8 ) over two synthetic streams of two windows each (the scripted-weights model of the other library tests): well-formed
    results, the same transcript from a second run."""
    from whisper_amd import api
    hp = gf.hparams_for("test-d128-ml")
    path = str(tmp_path / "cond.bin")
    gf.write_model(path, gf.conditioned_model(gf.conditioned_layout(hp), 4, kind="test-d128-ml", seed=10))
    model = api.Model(path)
    runner = api.BatchRunner(model, max_slots=4, flags=api.BATCH_CROSS_FP8)
    pcms = [_pcm(40, 330, 7), _pcm(35, 440, 8)]
    runs = []
    for _ in range(2):
        hr, segs, per = runner.run(pcms, language="en", prompt=[1000], n_max_text_ctx=0, flags=api.NO_CONTEXT | api.SINGLE_SEGMENT)
        assert hr == 0 and list(per) == [0, 0] and len(segs) == 2 and len(runner.window_stats) == 2
        assert all(s["t1"] >= s["t0"] and isinstance(s["text"], (str, bytes)) and all(0 <= t["id"] < hp.n_vocab for t in s["tokens"]) for r in segs for s in r)
        runs.append([[(s["t0"], s["t1"], s["text"], [t["id"] for t in s["tokens"]]) for s in r] for r in segs])
    assert runs[0] == runs[1] and any(len(r) for r in runs[0])
    runner.close()
    model.close()


def test_memory_and_refusals(toy):
    m, hp, mel = toy
    c16, c8 = _contexts(m, 64)
    print("context of 64 windows: %.1f MB with FP16 caches, %.1f MB with FP8 caches" % (c16.vram_bytes() / 1e6, c8.vram_bytes() / 1e6))
    assert c8.vram_bytes() < c16.vram_bytes()
    c8.encode(mel)
    sp = gf.special_tokens(hp)
    for what, call in (("one hypothesis per window", lambda: binding.HipContext(m, 2, hypotheses=2, cross_fp8=True)),
                       ("FP16 cross-attention keys", lambda: c8.align_tokens([[sp["sot"], sp["transcribe"], sp["not_"], 100, sp["eot"]]], [hp.n_audio_ctx])),
                       ("parity modes", lambda: c8.set_flags(binding.WH_FLAG_PARITY_EXACT)),
                       ("parity modes", lambda: c8.set_flags(binding.WH_FLAG_PARITY_PV, 2)),
                       ("cross-k8", lambda: c8.debug_read("cross-k", 0))):
        with pytest.raises(binding.WhisperHipError, match=what):
            call()
    c16.close()
    c8.close()
