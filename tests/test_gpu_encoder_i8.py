"""GPU tests of the INT8 encoder products (whisper_amd/csrc/quant_i8.hip, gemm_i8.hip; DESIGN.md section 7 "INT8 encoder products"): the quantizers and the product
bit for bit against the numpy statement (tests/encoder_i8_ref.py), a decode end to end against the FP16 context, and the public face with its refusals."""
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import encoder_i8_ref as i8  # noqa: E402
import encoder_ops_ref as R  # noqa: E402
from whisper_amd import binding, ggml_format as gf  # noqa: E402

pytestmark = pytest.mark.gpu
F32 = np.float32
B = binding


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


# ---- 1. the quantizers -------------------------------------------------------------------------------------------------------------------------------
TIES = [127, 0.5, 1.5, 2.5, -0.5, -3.5, 126.5]                  # amax 127: s = 1 exactly, x / s halfway between two integers ...
TIES_WANT = [127, 0, 2, 2, 0, -4, 126]                          # ... goes to the even one


def _rows(K):
    """16 rows of K: zeros, amax 65504, FP16 subnormals only, the ties, then seeded normal rows of several magnitudes."""
    rng = np.random.default_rng(K)
    rows = [np.zeros(K, np.float16), (0.3 * rng.standard_normal(K)).astype(np.float16)]
    rows[1][K // 3] = -65504
    rows.append((rng.integers(1, 1024, K).astype(np.uint16) | (rng.integers(0, 2, K) << 15).astype(np.uint16)).view(np.float16))
    rows.append(np.resize(np.asarray(TIES, np.float16), K))
    while len(rows) < 16:
        rows.append((rng.standard_normal(K) * 10.0 ** rng.uniform(-4, 3)).astype(np.float16))
    return np.stack(rows)


@pytest.mark.parametrize("K", [128, 1024, 5120])
@pytest.mark.parametrize("rows", [1, 63, 64, 65])
def test_quantizer_bit_for_bit(rows, K):
    """wh_op_quantize_rows_i8 == the restatement, bytes and scales, rows K + 8 apart; the row behind the last stays as it was."""
    x = np.full((rows, K + 8), np.nan, np.float16)
    x[:, :K] = _rows(K)[(np.arange(rows) + rows // 63 * 3) % 16]              # a single row: the zeros; more: the ties first
    q = torch.full((rows + 1, K), 0x7F, dtype=torch.int8, device="cuda")
    s = torch.full((rows + 1,), float("nan"), dtype=torch.float32, device="cuda")
    B.check(B.lib().wh_op_quantize_rows_i8(None, ptr(dev(x)), K + 8, ptr(q), ptr(s), rows, K))
    torch.cuda.synchronize()
    gq, gs = q.cpu().numpy(), s.cpu().numpy()
    wq, ws = i8.quantize_rows(x[:, :K])
    assert np.array_equal(gs[:rows], ws) and np.array_equal(gq[:rows], wq) and wq.min() >= -127
    assert (gq[rows] == 0x7F).all() and np.isnan(gs[rows])
    if rows > 1:                                                               # the ties, without the restatement
        assert gs[0] == 1.0 and list(gq[0, :len(TIES)]) == TIES_WANT


@pytest.mark.parametrize("d", [128, 1024, 1280])
def test_layer_norm_i8_is_the_quantized_layer_norm(d):
    rows = 9
    rng = np.random.default_rng(d)
    x = dev((rng.standard_normal((rows, d)) * 3 + 0.5).astype(F32))
    w, b = dev((1 + 0.1 * rng.standard_normal(d)).astype(F32)), dev((0.1 * rng.standard_normal(d)).astype(F32))
    h = torch.zeros((rows, d), dtype=torch.float16, device="cuda")
    q = torch.full((rows + 1, d), 0x7F, dtype=torch.int8, device="cuda")
    s = torch.full((rows + 1,), float("nan"), dtype=torch.float32, device="cuda")
    B.check(B.lib().wh_op_layer_norm(None, ptr(x), ptr(w), ptr(b), ptr(h), rows, d))
    B.check(B.lib().wh_op_layer_norm_i8(None, ptr(x), ptr(w), ptr(b), ptr(q), ptr(s), rows, d))
    torch.cuda.synchronize()
    wq, ws = i8.quantize_rows(h.cpu().numpy())
    assert np.array_equal(s.cpu().numpy()[:rows], ws) and np.array_equal(q.cpu().numpy()[:rows], wq)
    assert (q.cpu().numpy()[rows] == 0x7F).all() and np.isnan(s.cpu().numpy()[rows])


# ---- 2. the product ----------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gelu_map():
    """gelu16 as the device computes it over every finite FP16 argument (the method of test_gpu_encoder_ops.py)."""
    x = np.arange(65536, dtype=np.uint32).astype(np.uint16)
    fin = np.isfinite(x.view(np.float16))
    a = np.zeros((int(fin.sum()), 64), np.float16)
    a[:, 0] = x[fin].view(np.float16)
    w = np.zeros((64, 64), np.float16)
    w[:, 0] = 1.0
    out = torch.zeros(a.shape, dtype=torch.float16, device="cuda")
    B.check(B.lib().wh_op_mul_mat_gelu(None, ptr(dev(a)), ptr(dev(w)), ptr(dev(np.zeros(64, F32))), ptr(out), len(a), 64, 64))
    m = np.zeros(65536, np.uint16)
    m[fin] = out.cpu().numpy()[:, 3].view(np.uint16)
    return m


# ( M, N, K, epi, bias, res, T of epi 3 / extra ldc of epi 0 and 1, operands ): every M edge, the smallest N, one and two K tiles, the column-store path (ldc + 4)
CASES = [(1, 128, 128, 0, 1, 1, 0, ""), (255, 128, 128, 0, 0, 0, 0, ""), (256, 128, 256, 0, 1, 0, 0, ""), (257, 384, 128, 0, 0, 1, 0, ""),
         (513, 1024, 256, 0, 1, 1, 0, ""), (256, 1024, 4096, 0, 1, 1, 0, "pm127"), (255, 384, 4096, 0, 1, 1, 0, ""), (1, 1024, 4096, 0, 0, 0, 0, ""),
         (513, 128, 4096, 0, 1, 1, 0, ""), (257, 128, 256, 0, 1, 1, 4, ""),
         (1, 128, 256, 1, 1, 0, 0, ""), (255, 1024, 128, 1, 1, 0, 0, ""), (256, 384, 256, 1, 1, 0, 0, ""), (257, 128, 4096, 1, 1, 0, 0, ""),
         (513, 1024, 128, 1, 1, 0, 0, ""), (255, 128, 128, 1, 1, 0, 4, ""),
         (1, 384, 128, 3, 1, 0, 1, ""), (255, 384, 256, 3, 1, 0, 85, ""), (256, 384, 128, 3, 1, 0, 128, ""), (257, 384, 256, 3, 1, 0, 257, ""),
         (513, 384, 128, 3, 1, 0, 171, ""), (256, 384, 4096, 3, 1, 0, 64, ""), (513, 384, 4096, 3, 1, 0, 513, "")]


@pytest.mark.parametrize("M,N,K,epi,has_bias,has_res,extra,operands", CASES)
def test_product_bit_for_bit(M, N, K, epi, has_bias, has_res, extra, operands, gelu_map):
    """wh_op_gemm_encoder_i8 == the restatement: the integer sum exact (float64), int32 -> FP32 and the two scale products rounded one by one, then epilogueOne's
    arithmetic. "pm127": every operand +-127 with the signs of a row nearly constant, |acc| up to 127^2 * 4096 > 2^24, mostly odd multiples that FP32 must round."""
    rng = np.random.default_rng(M * 7 + N + K + epi)
    if operands == "pm127":
        qa = np.outer(rng.choice([-127, 127], M), np.ones(K)).astype(np.int8)
        qw = np.outer(rng.choice([-127, 127], N), np.ones(K)).astype(np.int8)
        for m in range(M):
            qa[m, :m % 5] *= -1
        for n in range(N):
            qw[n, 5:5 + n % 3] *= -1
    else:
        qa, qw = rng.integers(-127, 128, (M, K)).astype(np.int8), rng.integers(-127, 128, (N, K)).astype(np.int8)
    sa, sw = (rng.uniform(0.5, 1.5, M) / 127).astype(F32), (rng.uniform(0.5, 1.5, N) / 127 / np.sqrt(K)).astype(F32)
    bias = (rng.standard_normal(N)).astype(F32) if has_bias else np.zeros(N, F32)
    y = i8.product(qa, sa, qw, sw)
    if operands == "pm127":
        acc = qa.astype(np.float64) @ qw.astype(np.float64).T
        assert np.abs(acc).max() > 2 ** 24 and (acc.astype(F32) != acc).mean() > 0.25
    qad, qwd, biasd = dev(qa), dev(qw), dev(bias)
    f = dict(a=qad.data_ptr(), w=qwd.data_ptr(), bias=biasd.data_ptr() if has_bias else None, M=M, N=N, K=K, lda=K, Mb=M, ldc=N, epi=epi)
    if epi == 3:
        T, H = extra, N // 192
        Tpad = R.round_up(T, 16)
        want = R.epi_qkv(y.reshape(M // T, T, N), bias, H, Tpad)
        outs = [torch.full((w.size + 64,), int(R.SENTINEL16), dtype=torch.int16, device="cuda") for w in want]
        f.update(q=outs[0].data_ptr(), k=outs[1].data_ptr(), v=outs[2].data_ptr(), T=T, Tpad=Tpad, H=H, B=M // T)
    else:
        ldc = N + extra
        f["ldc"] = ldc
        if epi == 0:                                                           # in place, like the encoder's residual stream: res == out32
            init = np.full((M + 1, ldc), R.SENTINEL32, np.uint32)
            if has_res:
                init[:M] = rng.standard_normal((M, ldc)).astype(F32).view(np.uint32)
            full = init.copy()
            full[:M, :N] = ((y + bias).astype(F32) + (init[:M, :N].view(F32) if has_res else F32(0))).astype(F32).view(np.uint32)
            outs = [dev(init.view(np.int32))]
            f.update(out32=outs[0].data_ptr(), res=outs[0].data_ptr() if has_res else None)
        else:
            full = np.full((M + 1, ldc), R.SENTINEL16, np.uint16)
            full[:M, :N] = gelu_map[R.gelu_arg_bits(y, bias)]
            outs = [torch.full((M + 1, ldc), int(R.SENTINEL16), dtype=torch.int16, device="cuda")]
            f.update(out16=outs[0].data_ptr())
        want = [full]
    sad, swd = dev(sa), dev(sw)
    wide = B.op_gemm_encoder_i8(ptr(sad), ptr(swd), **f)
    torch.cuda.synchronize()
    assert wide == (0 if extra == 4 and epi != 3 else 1)
    for o, w in zip(outs, want):
        got = o.cpu().numpy().reshape(-1).view(w.dtype)
        w = w.reshape(-1)
        bad = np.nonzero(got[:w.size] != w)[0]
        assert not len(bad), "%d of %d elements differ, first at %d: got 0x%x want 0x%x" % (len(bad), w.size, bad[0], got[bad[0]], w[bad[0]])
        assert (got[w.size:] == R.SENTINEL16).all()                            # the guard behind q, k and v


# ---- 3. end to end, 4. the public face -----------------------------------------------------------------------------------------------------------------
LOGIT_SHIFT_NUMPY = 3.8816e-2       # E: max |d logit| of oracle/whisper_np.py with the four encoder products replaced by the restatement (python tests/encoder_i8_ref.py)


@pytest.fixture(scope="module")
def toy(tiny_model, golden):
    m = B.HipModel.from_ggml(tiny_model)
    rng = np.random.default_rng(5)
    mel = np.stack([np.roll(golden["mel"], 37 * b, axis=1) + 0.01 * rng.standard_normal(golden["mel"].shape).astype(F32) for b in range(3)]).astype(F32)
    yield m, tiny_model.hparams, torch.from_numpy(mel).cuda()
    m.close()


def _logits(c, hp, mel):
    sp = gf.special_tokens(hp)
    steps = [np.array([[sp["sot"], sp["transcribe"], sp["not_"]]] * 3, np.int32)] + [np.array([[100 + 7 * i + b] for b in range(3)], np.int32) for i in range(3)]
    c.encode(mel)
    out, n_past = [], 0
    for t in steps:
        out.append(c.decode(t, n_past)[0].copy())
        n_past += t.shape[1]
    return out


def test_decode_steps_against_the_fp16_context(toy):
    """The inputs of test_gpu_cross_fp8.py's test of the same name on a context with the INT8 encoder products and on one without: finite logits that differ, by
    less than 4 E (the margin of the FP8 test: quantization steps that flip under the timed path's summation order). A context on which the setting was turned on
    and off again computes the bits of one that never had it."""
    m, hp, mel = toy
    c16, c8, cb = B.HipContext(m, 3), B.HipContext(m, 3), B.HipContext(m, 3)
    c8.set_encoder_i8(True)
    cb.set_encoder_i8(True)
    cb.set_encoder_i8(False)
    l16, l8, lb = _logits(c16, hp, mel), _logits(c8, hp, mel), _logits(cb, hp, mel)
    worst = max(float(np.abs(a - b).max()) for a, b in zip(l16, l8))
    print("INT8 encoder products against the FP16 context, 4 steps x 3 windows: max |d logit| %.3e (E = %.3e, bound 4 E)" % (worst, LOGIT_SHIFT_NUMPY))
    assert all(np.isfinite(a).all() for a in l8) and 0 < worst < 4 * LOGIT_SHIFT_NUMPY
    assert all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(l16, lb))
    assert c8.vram_bytes() > c16.vram_bytes()
    for c in (c16, c8, cb):
        c.close()


def test_refusals(toy):
    m, hp, mel = toy
    c = B.HipContext(m, 1)
    c.set_encoder_i8(True)
    for flags in ((B.WH_FLAG_PARITY_EXACT, 1), (B.WH_FLAG_PARITY_PV, 2)):
        with pytest.raises(B.WhisperHipError, match="parity modes"):
            c.set_flags(*flags)
    c.set_encoder_i8(False)
    c.set_flags(B.WH_FLAG_PARITY_PV, 2)
    with pytest.raises(B.WhisperHipError, match="parity modes"):
        c.set_encoder_i8(True)
    c.close()
    m192 = B.HipModel.from_ggml(gf.synth_model("test-d192", seed=3, n_audio_ctx=64, n_text_ctx=32))
    c = B.HipContext(m192, 1)
    with pytest.raises(B.WhisperHipError, match="multiple of 128"):
        c.set_encoder_i8(True)
    c.close()
    m192.close()


def _pcm(seconds, tone, seed):
    t = np.arange(int(seconds * 16000)) / 16000.0
    return (0.25 * np.sin(2 * np.pi * tone * t) * (1 + 0.6 * np.sin(2 * np.pi * 2.5 * t)) + 0.05 * np.random.default_rng(seed).standard_normal(len(t))).astype(F32)


@pytest.mark.parametrize("with_fp8", [False, True])
def test_batch_runner_with_int8_encoder(tmp_path, with_fp8):
    """BatchRunner( flags = BATCH_ENCODER_INT8 [ | BATCH_CROSS_FP8 ] ) over the two synthetic streams of test_batch_runner_with_fp8_caches: well-formed results,
    the same transcript from a second run."""
    from whisper_amd import api
    hp = gf.hparams_for("test-d128-ml")
    path = str(tmp_path / "cond.bin")
    gf.write_model(path, gf.conditioned_model(gf.conditioned_layout(hp), 4, kind="test-d128-ml", seed=10))
    model = api.Model(path)
    runner = api.BatchRunner(model, max_slots=4, flags=api.BATCH_ENCODER_INT8 | (api.BATCH_CROSS_FP8 if with_fp8 else 0))
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
