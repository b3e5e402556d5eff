"""tests/decode_step_ref.py checked on the CPU: at float32 its two halves of a decoder layer are WhisperNP's own single-token step.

The GPU tests of tests/test_gpu_decode_step_ops.py hold the kernels to decode_step_ref at float64; a restatement nobody checked would only move the question. Here the
d = 128 test model decodes a prompt and then one token through oracle.whisper_np.WhisperNP (exact_pv=False: P.V summed wide, the timed path's rule), and the self- and
cross-attention halves of layer 0 are rebuilt from decode_step_ref on the same state: same residual row, same caches."""
import numpy as np
import pytest

import decode_step_ref as ds
from oracle import whisper_np as wn
from whisper_amd import ggml_format as gf

F32 = np.float32


def _head_major(rows, H):
    """[n][d] FP16-valued float32 -> [1][H][n][64] FP16, the device's cache layout."""
    n, d = rows.shape
    return np.ascontiguousarray(rows.reshape(n, H, 64).transpose(1, 0, 2)[None]).astype(np.float16)


def _ulp16(a):
    """One FP16 ulp at |a| (normal range), never less than the ulp at 2^-14."""
    return 2.0 ** (np.floor(np.log2(np.maximum(np.abs(a), 2.0 ** -14))) - 10)


@pytest.fixture(scope="module")
def stepped(tiny_model):
    """WhisperNP on the test model with seeded cross-attention caches (no encoder run: the decoder only reads them)."""
    hp = tiny_model.hparams
    rng = np.random.default_rng(17)
    oracle = wn.WhisperNP(tiny_model)
    oracle.kv.cross_k = [wn.r16(0.8 * rng.standard_normal((hp.n_audio_ctx, hp.n_text_state))) for _ in range(hp.n_text_layer)]
    oracle.kv.cross_v = [wn.r16(rng.standard_normal((hp.n_audio_ctx, hp.n_text_state))) for _ in range(hp.n_text_layer)]
    return oracle, rng


@pytest.mark.parametrize("n_prompt", [3, 70])
def test_both_halves_at_float32_are_the_oracles_single_token_step(tiny_model, stepped, n_prompt):
    oracle, rng = stepped
    hp, t = tiny_model.hparams, tiny_model.tensors
    d, H = hp.n_text_state, hp.n_text_head
    prompt = [int(v) for v in rng.integers(0, 50000, n_prompt)]
    oracle.decode(prompt, 0, exact_pv=False)
    cache_k = _head_major(oracle.kv.self_k[0][:n_prompt], H)
    cache_v = _head_major(oracle.kv.self_v[0][:n_prompt], H)
    trace = {}
    oracle.decode([1234], n_prompt, exact_pv=False, trace=trace)
    x = trace["dec-rows"]
    s = F32(np.power(np.float64(F32(d) / F32(H)), -0.25))
    p = "decoder.blocks.0"

    # ---- self-attention half: LayerNorm -> fused Q/K/V -> append -> causal attention ----
    wqkv = np.concatenate([t[p + ".attn.query.weight"], t[p + ".attn.key.weight"], t[p + ".attn.value.weight"]])
    bqkv = np.concatenate([t[p + ".attn.query.bias"], np.zeros(d, F32), t[p + ".attn.value.bias"]])
    out, k_new, v_new = ds.self_block(x, t[p + ".attn_ln.weight"], t[p + ".attn_ln.bias"], wqkv, bqkv, s, cache_k, cache_v, [n_prompt], np.float32)
    assert np.array_equal(k_new[0], oracle.kv.self_k[0][n_prompt]) and np.array_equal(v_new[0], oracle.kv.self_v[0][n_prompt])
    want = wn.r16(trace["dec-KQV"])
    diff = np.abs(out - want)
    print("position %d, self-attention half: %d of %d outputs differ, max %.2e" % (n_prompt, int((diff > 0).sum()), diff.size, diff.max()))
    # the oracle sums P.V in float64 and its scores as a matrix product: an output may land on the other side of an FP16 rounding boundary, never farther
    assert (diff <= _ulp16(want)).all() and (diff > 0).mean() < 0.05

    # ---- cross-attention half on the residual row the oracle had there ----
    x1 = ((wn.mul_mat_w(t[p + ".attn.out.weight"], trace["dec-KQV"]) + t[p + ".attn.out.bias"]).astype(F32) + x).astype(F32)
    ck, cv = _head_major(oracle.kv.cross_k[0], H), _head_major(oracle.kv.cross_v[0], H)
    scores, out2 = ds.cross_split(x1, t[p + ".cross_attn_ln.weight"], t[p + ".cross_attn_ln.bias"], t[p + ".cross_attn.query.weight"],
                                  t[p + ".cross_attn.query.bias"], s, ck, cv, hp.n_audio_ctx, np.float32)
    want2 = wn.r16(trace["dec-KQV#2"])
    diff2 = np.abs(out2 - want2)
    print("position %d, cross-attention half: %d of %d outputs differ, max %.2e" % (n_prompt, int((diff2 > 0).sum()), diff2.size, diff2.max()))
    assert (diff2 <= _ulp16(want2)).all() and (diff2 > 0).mean() < 0.05
    # ... and the split form of wn.cross_attention_split (the kernel's order of the two sums) is the same function
    q = ds.cross_query(x1, t[p + ".cross_attn_ln.weight"], t[p + ".cross_attn_ln.bias"], t[p + ".cross_attn.query.weight"], t[p + ".cross_attn.query.bias"], s, np.float32)
    o_split, _ = wn.cross_attention_split(q[0, :64], ck[0, 0].astype(F32), cv[0, 0].astype(F32))
    assert (np.abs(wn.r16(o_split) - out2[0, :64]) <= _ulp16(out2[0, :64])).all()


def test_float64_and_float32_restatements_agree():
    """The two types differ by FP32 round-off, which the FP16 rounding points turn into rare one-ulp flips: the bound the GPU tests use has room for the kernels."""
    rng = np.random.default_rng(3)
    H, d, n = 2, 128, 90
    x = (rng.standard_normal((3, d)) * 2 + 0.3).astype(F32)
    lnw, lnb = (1 + 0.1 * rng.standard_normal(d)).astype(F32), (0.1 * rng.standard_normal(d)).astype(F32)
    wqkv = (rng.standard_normal((3 * d, d)) / np.sqrt(d)).astype(np.float16)
    bqkv = (0.1 * rng.standard_normal(3 * d)).astype(F32)
    kc = (0.8 * rng.standard_normal((3, H, 128, 64))).astype(np.float16)
    vc = rng.standard_normal((3, H, 128, 64)).astype(np.float16)
    s = F32(64.0 ** -0.25)
    o64, k64, v64 = ds.self_block(x, lnw, lnb, wqkv, bqkv, s, kc, vc, [0, 63, n], np.float64)
    o32, k32, v32 = ds.self_block(x, lnw, lnb, wqkv, bqkv, s, kc, vc, [0, 63, n], np.float32)
    assert np.abs(o64 - o32).max() < 4e-3 and np.abs(o64 - o32).mean() < 3e-4
    assert (np.abs(k64 - k32) <= _ulp16(k64)).all() and (np.abs(v64 - v32) <= _ulp16(v64)).all()
    # position 0: one key, p = 1, the output is the new value row itself
    assert np.array_equal(o64[0], v64[0])


def test_split_ranges_and_the_combine():
    """Ranges: every key in exactly one, trailing ranges empty for n <= 28; the combine on hand-made partials, an empty split (sum 0, zero vector) included."""
    for n in (1, 4, 5, 9, 28, 29, 32, 33, 700, 1499, 1500, 1536):
        r = ds.split_ranges(n)
        assert len(r) == 8 and r[0][0] == 0 and r[-1][1] == n and all(r[i][1] == r[i + 1][0] for i in range(7))
        assert max(b - a for a, b in r) <= 192
        if n <= 28:
            assert r[-1][0] == r[-1][1]
    rng = np.random.default_rng(1)
    part = np.zeros((2, 3, 8, 68), F32)
    part[..., :64] = rng.standard_normal((2, 3, 8, 64))
    sums = rng.uniform(0.5, 2.0, (2, 3, 8))
    sums[:, :, 5:] = 0.0
    part[:, :, 5:, :64] = 0.0
    part[..., 64:66] = sums[..., None].view(F32)
    want = wn.r16(part[..., :64].astype(np.float64).sum(axis=2) / sums.sum(axis=2)[..., None]).reshape(2, 192)
    for dt in (np.float32, np.float64):
        got = ds.combine_partials(part, dt)
        assert (np.abs(got - want) <= _ulp16(want)).all()
