"""GPU tests of the INT8 decoder weights (whisper_amd/csrc/gemm_decode_w8.hip; DESIGN.md section 7 "INT8 decoder weights"): gemvW8 alone against the float64
product of the same int8 weights, a context's single-token steps against the float64 decoder with the quantized weights in place, the refusals, the batch runner."""
import copy
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import decode_step_ref as ds  # noqa: E402
import encoder_i8_ref as i8  # noqa: E402
from oracle import whisper_np as wn  # noqa: E402
from test_gpu_decode_step_ops import check_layer_norm_rows, ulp16  # noqa: E402
from test_gpu_encoder_i8 import _pcm  # noqa: E402
from whisper_amd import binding as B, ggml_format as gf  # noqa: E402

pytestmark = pytest.mark.gpu
F32 = np.float32


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def nan_out(rows, cols, dtype):
    return torch.full((rows, cols), float("nan"), dtype=dtype, device="cuda")


def bound32(K):
    """The project's bound for FP32 accumulation at N(0,1) operands (test_gemv_small_f32, test_mul_mat): the int8 products are exact, the scale adds one rounding."""
    return 2e-5 * max(1.0, np.sqrt(K / 128))


def operands(M, N, K, seed):
    """standard_normal weights quantized by the numpy statement, standard_normal FP16 rows, bias and residual; w64 = q * sw in float64."""
    rng = np.random.default_rng(seed)
    q, sw = i8.quantize_rows(rng.standard_normal((N, K), dtype=F32).astype(np.float16))
    a = rng.standard_normal((M, K), dtype=F32).astype(np.float16)
    return rng, q, sw, q.astype(np.float64) * sw.astype(np.float64)[:, None], a, rng.standard_normal(N).astype(F32), rng.standard_normal((M, N)).astype(F32)


def twice(M, N, dtype, launch):
    """Two launches into NaN-filled [M + 1][N] outputs: the same bits, the row beyond M untouched. Returns rows 0 .. M - 1 of the first."""
    outs = [nan_out(M + 1, N, dtype) for _ in range(2)]
    for o in outs:
        launch(o.data_ptr())
    torch.cuda.synchronize()
    assert torch.equal(outs[0][:M], outs[1][:M]), "two launches differ"
    got = outs[0].cpu().numpy()
    assert np.isnan(got[M]).all(), "a row beyond M was written"
    return got[:M]


# M: one tile, two, row groups of 32 and of 64; N: 4-row and 16-row workgroups with a partial last one, an N that is no multiple of 4; K: 2, 4 and 8 waves
F32_CASES = [(1, 16, 128), (1, 72, 4096), (1, 4104, 1280), (1, 200, 5120), (5, 72, 384), (5, 4104, 4096), (5, 16, 1280), (5, 51865, 128),
             (16, 200, 128), (16, 72, 5120), (16, 4104, 384), (17, 16, 4096), (17, 200, 1280), (32, 72, 1280), (32, 4104, 128), (32, 16, 5120),
             (33, 200, 4096), (33, 16, 384), (33, 72, 128), (70, 72, 5120), (70, 4104, 1280), (128, 4104, 4096), (128, 4104, 384), (128, 16, 1280), (128, 72, 128)]


@pytest.mark.parametrize("M,N,K", F32_CASES)
def test_gemv_w8_f32(M, N, K):
    """out = ( x . q ) sw + bias + residual against the float64 product of the same int8 weights, every output finite and within bound32( K )."""
    rng, q, sw, w64, a, bias, res = operands(M, N, K, M * 131 + N + K)
    qd, sd, ad, bd, rd = dev(q), dev(sw), dev(a), dev(bias), dev(res)
    got = twice(M, N, torch.float32, lambda o: B.op_gemv_w8(M, N, K, qd.data_ptr(), sd.data_ptr(), a=ad.data_ptr(), bias=bd.data_ptr(), res=rd.data_ptr(), out32=o))
    d = np.abs(got - (a.astype(np.float64) @ w64.T + bias + res)).max()
    print("gemv_w8 %dx%dx%d: max|diff| %.3e (bound %.3e)" % (M, N, K, d, bound32(K)))
    assert np.isfinite(got).all() and d <= bound32(K)


@pytest.mark.parametrize("M,K", [(m, k) for m in (1, 16, 17, 32) for k in (128, 1280)])
def test_gemv_w8_layer_norm_prologue(M, K):
    """pro = 1: the FP16 rows the kernel builds are read back through an int8 identity (1 . x with scale 1 is exact), held by check_layer_norm_rows' criterion,
    and are then the operands of the float64 product (test_gemv_small_f32's method)."""
    N = 72
    rng, q, sw, w64, _, bias, res = operands(M, N, K, M * 17 + K)
    x = (rng.standard_normal((M, K)) * 2 + 0.3).astype(F32)
    lnw, lnb = (1 + 0.1 * rng.standard_normal(K)).astype(F32), (0.1 * rng.standard_normal(K)).astype(F32)
    lnd = [dev(t) for t in (x, lnw, lnb)]
    ln = tuple(t.data_ptr() for t in lnd)
    eye, ones, probe = dev(np.eye(K, dtype=np.int8)), dev(np.ones(K, F32)), nan_out(M, K, torch.float32)
    B.op_gemv_w8(M, K, K, eye.data_ptr(), ones.data_ptr(), pro=1, ln=ln, out32=probe.data_ptr())
    torch.cuda.synchronize()
    xn = probe.cpu().numpy()
    check_layer_norm_rows("gemv_w8 %dx%dx%d" % (M, N, K), xn, x, lnw, lnb)
    qd, sd, bd, rd = dev(q), dev(sw), dev(bias), dev(res)
    got = twice(M, N, torch.float32, lambda o: B.op_gemv_w8(M, N, K, qd.data_ptr(), sd.data_ptr(), pro=1, ln=ln, bias=bd.data_ptr(), res=rd.data_ptr(), out32=o))
    d = np.abs(got - (xn.astype(np.float64) @ w64.T + bias + res)).max()
    print("gemv_w8 %dx%dx%d LayerNorm prologue: max|diff| %.3e (bound %.3e)" % (M, N, K, d, bound32(K)))
    assert np.isfinite(got).all() and d <= bound32(K)


@pytest.mark.parametrize("M,N,K", [(5, 200, 384), (32, 72, 1280), (70, 4104, 128)])
def test_gemv_w8_gelu(M, N, K, golden):
    """epi = 1: got = table[ fp16( pre + e ) ] with |e| <= bound32( K ): between the reference's table values at the two ends of that interval (and at pre), one
    FP16 ulp beyond for gelu16 against the table."""
    rng, q, sw, w64, a, bias, _ = operands(M, N, K, M + N + K)
    qd, sd, ad, bd = dev(q), dev(sw), dev(a), dev(bias)
    got = twice(M, N, torch.float16, lambda o: B.op_gemv_w8(M, N, K, qd.data_ptr(), sd.data_ptr(), epi=1, a=ad.data_ptr(), bias=bd.data_ptr(), out16=o)).astype(F32)
    pre = a.astype(np.float64) @ w64.T + bias
    ends = np.stack([ds.gelu_table(pre + e, golden["table_gelu"]) for e in (-bound32(K), 0.0, bound32(K))])
    lo, hi = ends.min(axis=0), ends.max(axis=0)
    print("gemv_w8 gelu %dx%dx%d: %.4f of the entries differ from table[ fp16( pre ) ]" % (M, N, K, (got != ends[1]).mean()))
    assert np.isfinite(got).all() and (got >= lo - ulp16(lo)).all() and (got <= hi + ulp16(hi)).all()


@pytest.mark.parametrize("M", [5, 33])
def test_gemv_w8_qkv_decode(M):
    """epi = 2 with two heads: q and the appended cache rows within one FP16 ulp of the float64 restatement plus the sum's round-off; no other cache element moves."""
    H, d, ctx = 2, 128, 24
    rng, q, sw, w64, a, bias, _ = operands(M, 3 * d, d, M)
    bias[d:2 * d] = 0.0
    scale = F32(64.0 ** -0.25)
    want = ds.qkv(a.astype(F32), w64, bias, scale)
    pos = (np.arange(M) * 5 % ctx).astype(np.int32)
    kc, vc = (rng.standard_normal((2, M, H, ctx, 64))).astype(np.float16)
    kd, vd, qd = dev(kc), dev(vc), nan_out(M + 1, d, torch.float16)
    ops = [dev(t) for t in (q, sw, a, bias, pos)]
    B.op_gemv_w8(M, 3 * d, d, ops[0].data_ptr(), ops[1].data_ptr(), epi=2, a=ops[2].data_ptr(), bias=ops[3].data_ptr(), q=qd.data_ptr(), kc=kd.data_ptr(),
                 vc=vd.data_ptr(), heads=H, text_ctx=ctx, n_past_dev=ops[4].data_ptr(), scale=scale)
    torch.cuda.synchronize()
    qg, kg, vg = qd.cpu().numpy().astype(F32), kd.cpu().numpy(), vd.cpu().numpy()
    assert np.isnan(qg[M]).all()
    rows = [qg[:M]] + [np.stack([c[s, :, pos[s]].reshape(d) for s in range(M)]).astype(F32) for c in (kg, vg)]
    for name, g, w in zip("qkv", rows, want):
        assert (np.abs(g - w) <= ulp16(w) + bound32(d)).all(), name
    for s in range(M):
        kc[s, :, pos[s]], vc[s, :, pos[s]] = kg[s, :, pos[s]], vg[s, :, pos[s]]
    assert np.array_equal(kg, kc) and np.array_equal(vg, vc), "a cache element outside the appended rows changed"


# ---- the context ---------------------------------------------------------------------------------------------------------------------------------------
W8_FAMILIES = [".attn.query.weight", ".attn.key.weight", ".attn.value.weight", ".attn.out.weight", ".cross_attn.out.weight", ".mlp.0.weight", ".mlp.2.weight"]
# max |logit - float64 decoder| of the FP16 batch path (the parent commit: setting off, TUNE_DECODE_SMALL cleared) on the steps below, 2 windows / 5 hypotheses;
# measured once on an MI355X (largest |logit| 2.6). The bound for the INT8 weights against THEIR float64 decoder is twice that
# (measured: 1.499e-3 and 1.603e-3).
FP16_PATH_DISTANCE = {(2, 1): 1.5761e-3, (1, 5): 1.6616e-3}


class _Embedding:
    """The token embedding as the decoder reads it: FP16 rows for the lookup, the quantized copy for the vocabulary product."""

    def __init__(self, rows, product):
        self.rows, self.T = rows, product.T

    def __getitem__(self, i):
        return self.rows[i]


def truth_logits(model, mels, hyp, steps, quantized):
    """[step][sequence][n_vocab] float64 of oracle.whisper_np.WhisperTruth; quantized: the six weight families replaced by q * sw of the numpy statement."""
    base = wn.WhisperTruth(model)
    if quantized:
        deq = lambda w: (lambda q, s: q.astype(np.float64) * s.astype(np.float64)[:, None])(*i8.quantize_rows(np.asarray(w, np.float16)))
        for name, w in model.tensors.items():
            if name.startswith("decoder.blocks.") and any(name.endswith(f) for f in W8_FAMILIES):
                base.t[name] = deq(w)
        te = "decoder.token_embedding.weight"
        base.t[te] = _Embedding(base.t[te], deq(model.tensors[te]))
    out = [[] for _ in steps]
    for b, mel in enumerate(mels):
        base.encode(mel.astype(np.float64))
        for h in range(hyp):
            seq = copy.copy(base)
            seq.self_k, seq.self_v = [k.copy() for k in base.self_k], [v.copy() for v in base.self_v]
            for i, t in enumerate(steps):
                out[i].append(seq.decode([int(t[b * hyp + h, 0])], i)[0])
    return [np.stack(o) for o in out]


def device_logits(c, mels, steps):
    c.encode(torch.from_numpy(mels).cuda())
    return [c.decode(t, i)[0].copy() for i, t in enumerate(steps)]


def context_inputs(golden, windows, hyp):
    rng = np.random.default_rng(5)
    mels = np.stack([np.roll(golden["mel"], 37 * b, axis=1) + 0.01 * rng.standard_normal(golden["mel"].shape).astype(F32) for b in range(windows)]).astype(F32)
    return mels, [np.array([[100 + 7 * i + 3 * s] for s in range(windows * hyp)], np.int32) for i in range(3)]


@pytest.mark.parametrize("windows,hyp", [(2, 1), (1, 5)])
def test_context_steps_against_the_float64_decoder(windows, hyp, tiny_model, golden):
    """Three single-token steps with the setting on against the float64 decoder whose six weight families are q * sw; then off again: the bits of a context
    that never had the setting."""
    mels, steps = context_inputs(golden, windows, hyp)
    m = B.HipModel.from_ggml(tiny_model)
    c, never = B.HipContext(m, windows, hypotheses=hyp), B.HipContext(m, windows, hypotheses=hyp)
    c.set_decoder_w8(True)
    got = device_logits(c, mels, steps)
    want = truth_logits(tiny_model, mels, hyp, steps, True)
    worst = max(float(np.abs(g - w).max()) for g, w in zip(got, want))
    bound = 2 * FP16_PATH_DISTANCE[(windows, hyp)]
    print("INT8 decoder weights, %d x %d sequences, 3 steps: max |logit - float64| %.3e (bound %.3e)" % (windows, hyp, worst, bound))
    assert all(np.isfinite(g).all() for g in got) and worst <= bound
    c.set_decoder_w8(False)
    for a, b in zip(device_logits(c, mels, steps), device_logits(never, mels, steps)):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    c.close()
    never.close()
    m.close()


def test_refusals(tiny_model):
    m = B.HipModel.from_ggml(tiny_model)
    c = B.HipContext(m, 1)
    c.set_decoder_w8(True)
    for flags in ((B.WH_FLAG_PARITY_EXACT, 1), (B.WH_FLAG_PARITY_PV, 2)):
        with pytest.raises(B.WhisperHipError, match="parity modes"):
            c.set_flags(*flags)
    c.set_decoder_w8(False)
    c.set_flags(B.WH_FLAG_PARITY_PV, 2)
    with pytest.raises(B.WhisperHipError, match="parity modes"):
        c.set_decoder_w8(True)
    c.close()
    m.close()
    m192 = B.HipModel.from_ggml(gf.synth_model("test-d192", seed=3, n_audio_ctx=64, n_text_ctx=32))
    c = B.HipContext(m192, 1)
    with pytest.raises(B.WhisperHipError, match="multiple of 128"):
        c.set_decoder_w8(True)
    c.close()
    m192.close()


@pytest.mark.parametrize("more", ["", "fp8+encoder"])
def test_batch_runner_with_int8_decoder_weights(tmp_path, more):
    """BatchRunner( flags = BATCH_DECODER_INT8 [ | BATCH_CROSS_FP8 | BATCH_ENCODER_INT8 ] ) over the two synthetic streams of test_batch_runner_with_fp8_caches:
    well-formed results, the same transcript from a second run."""
    from whisper_amd import api
    hp = gf.hparams_for("test-d128-ml")
    path = str(tmp_path / "cond.bin")
    gf.write_model(path, gf.conditioned_model(gf.conditioned_layout(hp), 4, kind="test-d128-ml", seed=10))
    model = api.Model(path)
    runner = api.BatchRunner(model, max_slots=4, flags=api.BATCH_DECODER_INT8 | (api.BATCH_CROSS_FP8 | api.BATCH_ENCODER_INT8 if more else 0))
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
