"""CPU tests of tests/encoder_ops_ref.py, the reference tests/test_gpu_encoder_ops.py holds the encoder's fused products to.

Three things are shown here, without a GPU: (1) the exactness claim the GPU tests rest on -- with dyadic() inputs the FP32 product equals the float64 product in any
summation order; (2) the restatements (im2col by slicing, the stride-2 slicing, the head split, the V operand order, the cache placement) agree with the numpy
restatement of the reference's CPU path, oracle/whisper_np.py, on the d = 128 test model with Gaussian weights: accumulators within the FP32 round-off of a K-term
dot product, and -- fed whisper_np's own FP32 accumulators -- every output bit for bit; (3) v_frag_index is a bijection for every T the GPU tests use.
"""
import numpy as np
import pytest

import encoder_ops_ref as R
from oracle import whisper_np as wn
from whisper_amd import ggml_format as gf

T_USED = (1500, 375, 130, 100, 50, 1)
N_CTX = 50                                   # the audio context of the comparison with whisper_np: T % 4 == 2, not a multiple of 16


def dot_bound(a16, w16, K):
    """Round-off of an FP32 dot product of K terms in any order (gamma_K sum |a_i w_i|, Higham 3.1), one more rounding for the conversion, per output element."""
    s = np.abs(a16.astype(np.float64)) @ np.abs(w16.astype(np.float64)).T
    return (K + 2) * 2.0 ** -24 * s


@pytest.mark.parametrize("K", [384, 1280])
def test_dyadic_products_are_exact_in_fp32(K):
    """The largest K of the GPU tests (conv2 at d = 128: 384) and the largest the claim is made for (1280): float32 == float64, whatever the order."""
    rng = np.random.default_rng(K)
    a, w = R.activations(rng, (257, K)), R.weights(rng, (130, K))
    want = R.mul_acc(a, w)
    assert np.abs(want).max() < 2.0 ** 12 and np.array_equal(np.round(want * 128), want * 128)
    a32, w32 = a.astype(np.float32), w.astype(np.float32)
    assert np.array_equal((a32 @ w32.T).astype(np.float64), want)
    # other orders: back to front, and 16 interleaved partial sums added at the end (what a matrix core's K slices amount to)
    assert np.array_equal((a32[:, ::-1] @ w32[:, ::-1].T).astype(np.float64), want)
    part = np.zeros((16,) + want.shape, np.float32)
    for k in range(K):
        part[k % 16] += a32[:, k:k + 1] * w32[None, :, k]
    tot = np.zeros(want.shape, np.float32)
    for p in part[::-1]:
        tot += p
    assert np.array_equal(tot.astype(np.float64), want)
    # the worst case stays exact too: every term at its largest magnitude
    worst = np.float32(2.0) * np.float32(1.0) * K
    assert worst < 2.0 ** 12 and np.float32(worst + np.float32(1.0 / 128)) - worst == np.float32(1.0 / 128)
    R.as_f32_exact(want)


@pytest.mark.parametrize("T", T_USED)
def test_v_frag_index_is_a_bijection(T):
    tp = R.round_up(T, 16)
    key, dd = np.meshgrid(np.arange(tp), np.arange(64), indexing="ij")
    idx = R.v_frag_index(key, dd).ravel()
    assert np.array_equal(np.sort(idx), np.arange(64 * tp))
    live = R.v_frag_index(key[:T], dd[:T]).ravel()
    assert len(np.unique(live)) == T * 64 and live.min() >= 0 and live.max() < 64 * tp


def gelu_map_np():
    """wn.gelu16 over all 65536 FP16 arguments, as bit patterns (the map the restatement's epilogues take; on the device it is read from the kernel)."""
    x = np.arange(65536, dtype=np.uint32).astype(np.uint16).view(np.float16).astype(np.float32)
    with np.errstate(all="ignore"):
        return wn.gelu16(x).astype(np.float16).view(np.uint16)


@pytest.fixture(scope="module")
def traced():
    model = gf.synth_model("test-d128", seed=11, n_audio_ctx=N_CTX, attn_sharpness=2.0)
    rng = np.random.default_rng(12)
    mel = rng.standard_normal((model.hparams.n_mels, 2 * N_CTX - 1)).astype(np.float32)
    oracle = wn.WhisperNP(model)
    trace = {}
    oracle.encode(mel, 3, trace=trace)
    return model, mel, oracle, trace


def test_mel_layout_and_convolutions_agree_with_whisper_np(traced):
    model, mel, oracle, trace = traced
    hp, t = model.hparams, model.tensors
    d, n_mels = hp.n_audio_state, hp.n_mels
    gmap = gelu_map_np()
    # the operand of conv1: offset 3 into a spectrogram that ends 4 frames before the window does
    x_bits = R.mel_to_conv_input([mel], [3], n_mels, 2 * N_CTX)
    xpad = x_bits.view(np.float16).reshape(1, 2 * N_CTX + 2, n_mels).copy()
    assert (x_bits[0, :n_mels] == R.SENTINEL16).all() and (x_bits[0, -n_mels:] == R.SENTINEL16).all()
    xpad[:, 0] = 0
    xpad[:, -1] = 0
    inp = np.zeros((n_mels, 2 * N_CTX), np.float32)
    inp[:, :mel.shape[1] - 3] = mel[:, 3:]
    assert np.array_equal(xpad[0, 1:-1].astype(np.float32), wn.r16(inp).T)
    # conv1
    kpad = R.round_up(3 * n_mels, 64)
    w1 = R.conv_weight_rows(t["encoder.conv1.weight"].astype(np.float16), kpad)
    acc = R.conv_acc(xpad, w1, 1)
    want = trace["enc.conv1"].T
    cols = np.concatenate([xpad[0, tap:tap + 2 * N_CTX] for tap in range(3)], axis=1)
    assert (np.abs(acc[0] - want) <= dot_bound(cols, w1[:, :3 * n_mels], 3 * n_mels)).all()
    y = R.epi_conv1(want[None].astype(np.float32), t["encoder.conv1.bias"], gmap)
    assert np.array_equal(y[0, 1:-1].view(np.float16).astype(np.float32), trace["enc.temp1"].T)
    # conv2 + positional embedding
    ypad = y.view(np.float16).copy()
    ypad[:, 0] = 0
    ypad[:, -1] = 0
    w2 = R.conv_weight_rows(t["encoder.conv2.weight"].astype(np.float16), 3 * d)
    acc2 = R.conv_acc(ypad, w2, 2)
    want2 = oracle.conv_1d(t["encoder.conv2.weight"], trace["enc.temp1"], 2).T
    cols2 = np.concatenate([ypad[0, tap:tap + 2 * N_CTX:2][:N_CTX] for tap in range(3)], axis=1)
    assert (np.abs(acc2[0] - want2) <= dot_bound(cols2, w2, 3 * d)).all()
    x0 = R.epi_conv2(want2[None].astype(np.float32), t["encoder.conv2.bias"], t["encoder.positional_embedding"].astype(np.float32), gmap)
    assert np.array_equal(x0, trace["enc.layer[ 0 ].in"])


def test_qkv_and_cross_kv_agree_with_whisper_np(traced):
    model, mel, oracle, trace = traced
    hp, t = model.hparams, model.tensors
    d, H, T = hp.n_audio_state, hp.n_audio_head, N_CTX
    # Q/K/V of layer 0: the fused [3 d][d] weight, the key third of the bias zero
    p = "encoder.blocks.0"
    cur = wn.layer_norm(trace["enc.layer[ 0 ].in"], t[p + ".attn_ln.weight"], t[p + ".attn_ln.bias"])
    names = (".attn.query.weight", ".attn.key.weight", ".attn.value.weight")
    w = np.concatenate([t[p + n].astype(np.float16) for n in names])
    bias = np.concatenate([t[p + ".attn.query.bias"].reshape(-1), np.zeros(d, np.float32), t[p + ".attn.value.bias"].reshape(-1)]).astype(np.float32)
    acc_np = np.concatenate([wn.mul_mat_w(t[p + n], cur) for n in names], axis=1)
    a16 = cur.astype(np.float16)
    assert (np.abs(R.mul_acc(a16, w) - acc_np) <= dot_bound(a16, w, d)).all()
    Tpad = R.round_up(T, 256)
    q, k, v = R.epi_qkv(acc_np[None], bias, H, Tpad)
    key, dd = np.meshgrid(np.arange(T), np.arange(64), indexing="ij")
    idx = R.v_frag_index(key, dd)
    for h in range(H):
        sl = slice(h * 64, (h + 1) * 64)
        assert np.array_equal(q[0, h].view(np.float16).astype(np.float32), wn.r16(trace["enc-Qcur-b"])[:, sl])
        assert np.array_equal(k[0, h].view(np.float16).astype(np.float32), wn.r16(trace["enc-Kcur"])[:, sl])
        assert np.array_equal(v[0, h][idx].view(np.float16).astype(np.float32), wn.r16(trace["enc-Vcur-b"])[:, sl])
        untouched = np.ones(64 * Tpad, bool)
        untouched[idx.ravel()] = False
        assert (v[0, h][untouched] == R.SENTINEL16).all()
    # cross-K/V of every decoder layer in one product, written at window 1 of caches of 3
    out = trace["encode-out"]
    ws, bs, accs = [], [], []
    for il in range(hp.n_text_layer):
        c = "decoder.blocks.%d.cross_attn" % il
        ws += [t[c + ".key.weight"].astype(np.float16), t[c + ".value.weight"].astype(np.float16)]
        bs += [np.zeros(d, np.float32), t[c + ".value.bias"].astype(np.float32).reshape(-1)]
        accs += [wn.mul_mat_w(t[c + ".key.weight"], out), wn.mul_mat_w(t[c + ".value.weight"], out)]
    w, bias, acc_np = np.concatenate(ws), np.concatenate(bs), np.concatenate(accs, axis=1)
    a16 = out.astype(np.float16)
    assert (np.abs(R.mul_acc(a16, w) - acc_np) <= dot_bound(a16, w, d)).all()
    kscale = np.float32(np.power(np.float64(np.float32(d) / np.float32(H)), -0.25))
    ck, cv = R.epi_cross(acc_np[None], bias, kscale, H, 3, 1)
    for il in range(hp.n_text_layer):
        for h in range(H):
            sl = slice(h * 64, (h + 1) * 64)
            assert np.array_equal(ck[il, 1, h].view(np.float16).astype(np.float32), oracle.kv.cross_k[il][:, sl])
            assert np.array_equal(cv[il, 1, h].view(np.float16).astype(np.float32), oracle.kv.cross_v[il][:, sl])
    assert (ck[:, [0, 2]] == R.SENTINEL16).all() and (cv[:, [0, 2]] == R.SENTINEL16).all()
