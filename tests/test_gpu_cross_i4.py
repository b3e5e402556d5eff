"""GPU tests of the INT4 cross-attention caches (whisper_amd/csrc/kv4.hip; DESIGN.md section 7 "INT4 cross-attention caches"): the quantizer bit for bit against
the numpy statement of the format (tests/cross_i4_ref.py), the caches of an INT4 context against the quantized caches of an FP16 context, attentionDecG4 against
float64 on the dequantized values, decode steps end to end against the FP16 context, and the public face with its refusals."""
import ctypes as C
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import cross_i4_ref as i4  # noqa: E402
import decode_step_ref as ds  # noqa: E402
from oracle import whisper_np as wn  # noqa: E402
from whisper_amd import binding, ggml_format as gf  # noqa: E402

pytestmark = pytest.mark.gpu
F32 = np.float32
TIES = [7, 2.5, 0.5, 1.5, -2.5, 3.5, -6.5, -0.5]          # amax 7 -> s = 1: x / s halfway between two codes ...
TIES_WANT = [7, 2, 0, 2, -2, 4, -6, 0]                    # ... and the even neighbour


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


@functools.lru_cache(None)
def _row_pool():
    """32 rows: zeros, signed zeros, FP16 subnormals only, 65504, the ties, then seeded normal rows of several magnitudes."""
    rng = np.random.default_rng(4)
    rows = [np.zeros(64, np.float16), np.where(np.arange(64) % 3 == 0, -0.0, 0.0).astype(np.float16)]
    sub = rng.integers(1, 1024, 64).astype(np.uint16) | (rng.integers(0, 2, 64) << 15).astype(np.uint16)
    rows.append(sub.view(np.float16))
    r = (0.3 * rng.standard_normal(64)).astype(np.float16)
    r[5] = -65504
    rows.append(r)
    r = np.zeros(64, np.float16)
    r[:len(TIES)] = TIES
    rows.append(r)
    while len(rows) < 32:
        rows.append((rng.standard_normal(64) * 10.0 ** rng.uniform(-4, 3)).astype(np.float16))
    return np.stack(rows)


@pytest.mark.parametrize("n", [1, 7, 129])
def test_quantizer_bit_for_bit(n):
    """wh_op_quantize_cross_kv_i4 == the helper for 2 (window, head) blocks of n keys: K bytes, V bytes in their 64-key blocks, scales; what lies behind stays."""
    x = _row_pool()[(np.arange(2 * n) * 5 + n) % 32].reshape(2, n, 64)
    kb = (n + 63) // 64
    out_k = torch.full((2 * n + 1, 32), 0xAA, dtype=torch.uint8, device="cuda")
    out_v = torch.full((2 * kb + 1, 64, 32), 0xAA, dtype=torch.uint8, device="cuda")
    out_s = torch.full((2 * n + 1,), float("nan"), dtype=torch.float32, device="cuda")
    binding.check(binding.lib().wh_op_quantize_cross_kv_i4(None, ptr(dev(x)), ptr(out_k), ptr(out_v), ptr(out_s), 2, n))
    torch.cuda.synchronize()
    gk, gv, gs = out_k.cpu().numpy(), out_v.cpu().numpy(), out_s.cpu().numpy()
    codes, ws = i4.quantize(x)
    assert np.array_equal(gs[:2 * n], ws.reshape(-1))
    assert np.array_equal(gk[:2 * n], i4.pack_k(codes).reshape(-1, 32)) and np.array_equal(gv[:2 * kb], i4.pack_v(codes).reshape(-1, 64, 32))
    assert (gk[2 * n] == 0xAA).all() and (gv[2 * kb] == 0xAA).all() and np.isnan(gs[2 * n])
    if n == 129:                                                               # the row of ties (row 4 of the pool), without the helper's rounding
        j = int(np.flatnonzero((np.arange(2 * n) * 5 + n) % 32 == 4)[0])
        assert gs[j] == 1.0 and list(i4.unpack_k(gk[j])[:len(TIES)]) == TIES_WANT


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
        return binding.HipContext(m, max_batch), binding.HipContext(m, max_batch, cross_i4=True)
    finally:
        binding.set_option("enc_chunk", 128)


@pytest.mark.parametrize("audio_ctx,enc_chunk", [(0, 128), (130, 128), (0, 2)])
def test_cache_identity(toy, audio_ctx, enc_chunk):
    """The same wh_encode of 3 windows on an FP16 and on an INT4 context: nibbles and scales of the first and last decoder layer are the helper's quantization
    of the FP16 caches. Covers the per-layer product, a changed audio context, and the window offsets of an encode in chunks of 2 + 1."""
    m, hp, mel = toy
    c16, c4 = _contexts(m, 3, enc_chunk)
    T, H = audio_ctx or hp.n_audio_ctx, hp.n_audio_head
    for c in (c16, c4):
        c.set_audio_ctx(audio_ctx)
        c.encode(mel, offsets=[0, 7, 30])
    for il in (0, hp.n_text_layer - 1):
        for name, pack in (("k", i4.pack_k), ("v", i4.pack_v)):
            rows = c16.debug_read("cross-" + name, il).reshape(-1)[:3 * T * H * 64].reshape(3, T, H, 64).transpose(0, 2, 1, 3)
            codes, ws = i4.quantize(rows.astype(np.float16))
            assert float(np.abs(rows).max()) > 0.05
            assert np.array_equal(c4.debug_read("cross-%s4-scale" % name, il), ws), (il, name)
            assert np.array_equal(c4.debug_read("cross-%s4" % name, il), pack(codes)), (il, name)
    c16.close()
    c4.close()


WINDOWS = 3


@functools.lru_cache(4)
def _caches(H, n_keys):
    """K and V of 3 windows as nibbles and scales: values of unit size under scales 2^-10 .. 2^6 chosen per row (codes clipped to +-7); the 3 rows behind the
    last key hold nibbles 0xF under NaN scales. Returns device tensors and the float64 values."""
    rng = np.random.default_rng(H * 10000 + n_keys)
    out = []
    for gain, pack in ((0.8, i4.pack_k), (1.0, i4.pack_v)):
        s = np.ldexp(1.0, rng.integers(-10, 7, (WINDOWS, H, n_keys + 3))).astype(F32)
        n = np.clip(np.rint(gain * rng.standard_normal((WINDOWS, H, n_keys + 3, 64)) / s[..., None]), -7, 7).astype(np.int8)
        n[:, :, n_keys:] = 7
        s[:, :, n_keys:] = np.nan
        out += [dev(pack(n)), dev(s), i4.dequantize(n[:, :, :n_keys], s[:, :, :n_keys])]
    return out


@pytest.mark.parametrize("n_tok", [1, 3])
@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("group", [1, 5, 8])
@pytest.mark.parametrize("H", [2, 20])
@pytest.mark.parametrize("n_keys", [1, 15, 16, 17, 63, 64, 65, 129, 1499, 1500])
def test_attention_against_float64(n_keys, H, group, fused, n_tok):
    """wh_op_decoder_cross_attention_i4 against the float64 restatement evaluated on code x scale (exact in float64: the quantization error is not in the
    comparison), at the bounds test_gpu_decode_step_ops.py holds wh_op_decoder_cross_attention to against its float64 reference: 4e-3 max, 3e-4 mean.
    Measured: DESIGN.md section 7 "INT4 cross-attention caches"."""
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
    binding.check(binding.lib().wh_op_decoder_cross_attention_i4(None, *[ptr(t) for t in ops], C.c_float(float(scale)), ptr(kb), ptr(ks), ptr(vb), ptr(vs), ptr(out),
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


LOGIT_MAX_RECORDED = 1.416e-2       # max |logit( INT4 context ) - logit( FP16 context )| measured once on an MI355X; the bound is 4 x this


def test_decode_steps_against_the_fp16_context(toy):
    """The prompt step and three single-token steps of 3 windows, the same tokens fed to both contexts after the same wh_encode. The bound is measured, not
    guessed: 4 x the recorded maximum (the kernels are deterministic; the margin is for a compiler or driver change)."""
    m, hp, mel = toy
    c16, c4 = _contexts(m, 3)
    sp = gf.special_tokens(hp)
    steps = [np.array([[sp["sot"], sp["transcribe"], sp["not_"]]] * 3, np.int32)] + [np.array([[100 + 7 * i + b] for b in range(3)], np.int32) for i in range(3)]
    worst, means, n_past = 0.0, [], 0
    for c in (c16, c4):
        c.encode(mel)
    for t in steps:
        l16, l4 = c16.decode(t, n_past)[0], c4.decode(t, n_past)[0]
        assert np.isfinite(l4).all()
        worst, n_past = max(worst, float(np.abs(l4 - l16).max())), n_past + t.shape[1]
        means.append(float(np.abs(l4 - l16).mean()))
    print("INT4 against FP16 context, 4 steps x 3 windows: max |d logit| %.3e, mean %.3e (max |logit| %.2f)" % (worst, np.mean(means), float(np.abs(l16).max())))
    assert 0 < worst < 4 * LOGIT_MAX_RECORDED
    c16.close()
    c4.close()


def _pcm(seconds, tone, seed):
    t = np.arange(int(seconds * 16000)) / 16000.0
    return (0.25 * np.sin(2 * np.pi * tone * t) * (1 + 0.6 * np.sin(2 * np.pi * 2.5 * t)) + 0.05 * np.random.default_rng(seed).standard_normal(len(t))).astype(F32)


def test_public_face(toy, tmp_path, capfd):
    """BatchRunner( flags = BATCH_CROSS_INT4 ) over the two synthetic streams of test_batch_runner_with_fp8_caches: well-formed results, the same transcript from
    a second run; flags 2 and 8 together are refused; an INT4 context is smaller than an FP8 one and refuses what an FP8 context refuses."""
    from whisper_amd import api
    hp = gf.hparams_for("test-d128-ml")
    path = str(tmp_path / "cond.bin")
    gf.write_model(path, gf.conditioned_model(gf.conditioned_layout(hp), 4, kind="test-d128-ml", seed=10))
    model = api.Model(path)
    runner = api.BatchRunner(model, max_slots=4, flags=api.BATCH_CROSS_INT4 | api.BATCH_ENCODER_INT8)
    pcms = [_pcm(40, 330, 7), _pcm(35, 440, 8)]
    runs = []
    for _ in range(2):
        hr, segs, per = runner.run(pcms, language="en", prompt=[1000], n_max_text_ctx=0, flags=api.NO_CONTEXT | api.SINGLE_SEGMENT)
        assert hr == 0 and list(per) == [0, 0] and len(segs) == 2 and len(runner.window_stats) == 2
        assert all(s["t1"] >= s["t0"] and isinstance(s["text"], (str, bytes)) and all(0 <= t["id"] < hp.n_vocab for t in s["tokens"]) for r in segs for s in r)
        runs.append([[(s["t0"], s["t1"], s["text"], [t["id"] for t in s["tokens"]]) for s in r] for r in segs])
    assert runs[0] == runs[1] and any(len(r) for r in runs[0])
    runner.close()
    capfd.readouterr()
    with pytest.raises(api.WhisperError) as e:
        api.BatchRunner(model, max_slots=4, flags=api.BATCH_CROSS_INT4 | api.BATCH_CROSS_FP8)
    assert e.value.hr == 0x80070057 and "exclude each other" in capfd.readouterr().err
    model.close()

    m, hp, mel = toy
    c8, c4 = binding.HipContext(m, 64, cross_fp8=True), binding.HipContext(m, 64, cross_i4=True)
    print("context of 64 windows: %.1f MB with FP8 caches, %.1f MB with INT4 caches" % (c8.vram_bytes() / 1e6, c4.vram_bytes() / 1e6))
    assert c4.vram_bytes() < c8.vram_bytes()
    c8.close()
    c4.encode(mel)
    sp = gf.special_tokens(hp)
    for what, call in (("one hypothesis per window", lambda: binding.HipContext(m, 2, hypotheses=2, cross_i4=True)),
                       ("FP16 cross-attention keys", lambda: c4.align_tokens([[sp["sot"], sp["transcribe"], sp["not_"], 100, sp["eot"]]], [hp.n_audio_ctx])),
                       ("parity modes", lambda: c4.set_flags(binding.WH_FLAG_PARITY_EXACT)),
                       ("parity modes", lambda: c4.set_flags(binding.WH_FLAG_PARITY_PV, 2)),
                       ("cross-k4", lambda: c4.debug_read("cross-k", 0))):
        with pytest.raises(binding.WhisperHipError, match=what):
            call()
    c4.close()
