"""The kernels of a single-token decode step, restated in numpy (WhisperContext.cpp:412-520; whisper_amd/csrc/decode1.hip, selfBlockDec of attn_dec.hip).

Every function evaluates its sums in the floating-point type it is given: float64 = the reference the GPU tests of tests/test_gpu_decode_step_ops.py hold the
kernels to, float32 = the straightforward single-precision evaluation, which tests/test_decode_step_ref_cpu.py pins on WhisperNP's own single-token step. The
rounding points are those of the kernels and do not move with the type:

    xn = fp16( LayerNorm( x ) * w + b )                                   the activations of every product are FP16
    q = fp16( ( W xn + b ) s ),  k = fp16( W xn s ),  v = fp16( W xn + b ) the caches and the query are FP16
    p = table softmax of the FP32 scores with the maximum over ALL keys    oracle.whisper_np.softmax_table: e = exp16( s - max ), double sum, e * float( 1 / sum )
    out = fp16( P V )                                                     summed in the wide type, rounded once
    split cross-attention: out = fp16( sum( e V ) / sum( e ) )             the eight key ranges share the global maximum, so they only re-order the two sums
    GELU: table[ fp16( acc + bias ) ]                                      the reference's own 65536-entry table

Caches are laid out as the device holds them: [sequence][head][row][64], FP16.
"""
from __future__ import annotations

import numpy as np

from oracle import whisper_np as wn

F32 = np.float32
HEAD_DIM = 64
CROSS_SPLITS = 8
CROSS_PART = 68


def layer_norm16(x, w, b, dtype=np.float64):
    """fp16( LayerNorm( x ) * w + b ) over the last axis, as FP16-valued float32. float32: the reference's norm + two FP32 ops (wn.layer_norm)."""
    if dtype == np.float32:
        return wn.r16(wn.layer_norm(x, w, b))
    xd = np.asarray(x, np.float64)
    v = xd - xd.mean(axis=-1, keepdims=True)
    y = v / np.sqrt((v * v).mean(axis=-1, keepdims=True) + np.float64(F32(1e-5)))
    return wn.r16(y * np.asarray(w, np.float64) + np.asarray(b, np.float64))


def product(w16, x16, dtype=np.float64):
    """sum_k w[n][k] x[m][k] for FP16 weights [N][K] and FP16-valued activations [M][K]: [M][N] in `dtype`. float32: wn.mul_mat_w."""
    if dtype == np.float32:
        return wn.mul_mat_w(w16, x16)
    return np.asarray(x16, np.float64) @ np.asarray(w16, np.float64).T


def gemv(w16, x16, bias=None, residual=None, dtype=np.float64):
    """The FP32 epilogue: acc (+ bias) (+ residual), in `dtype`."""
    r = product(w16, x16, dtype)
    if bias is not None:
        r = (r + np.asarray(bias, dtype)).astype(dtype)
    if residual is not None:
        r = (r + np.asarray(residual, dtype)).astype(dtype)
    return r


def gelu_table(pre, table_bits):
    """table[ fp16( pre ) ]: table_bits = golden["table_gelu"], the reference's table as uint16. FP16-valued float32."""
    return table_bits.view(np.float16)[np.asarray(pre, F32).astype(np.float16).view(np.uint16)].astype(F32)


def qkv(xn16, wqkv16, bqkv, scale, dtype=np.float64):
    """The fused [3d][d] product with the decoder's epilogue. Returns q, k, v [M][d], FP16-valued float32."""
    d = xn16.shape[-1]
    acc = product(wqkv16, xn16, dtype)
    b = np.asarray(bqkv, dtype)
    s = dtype(scale)
    q = wn.r16(((acc[:, :d] + b[:d]).astype(dtype) * s).astype(dtype))
    k = wn.r16((acc[:, d:2 * d] * s).astype(dtype))
    v = wn.r16((acc[:, 2 * d:] + b[2 * d:]).astype(dtype))
    return q, k, v


def attend(q, K, V, dtype=np.float64):
    """One head: q [64], K, V [n][64] (FP16 values). fp16( softmax_table( K q ) V ), [64] FP16-valued float32."""
    s = (np.asarray(K, dtype) @ np.asarray(q, dtype)).astype(F32)
    p = wn.softmax_table(s)
    return wn.r16(p.astype(dtype) @ np.asarray(V, dtype))


def self_block(x, ln_w, ln_b, wqkv16, bqkv, scale, k_cache, v_cache, pos, dtype=np.float64):
    """The self-attention half of a single-token step. x [seqs][d] FP32; caches FP16 [seqs][H][stride][64], rows 0 .. pos[s] - 1 of sequence s are live (the
    caches are not changed). Returns (out [seqs][d], k_new [seqs][d], v_new [seqs][d]), FP16-valued float32: the new rows belong at row pos[s]."""
    seqs, d = x.shape
    H = d // HEAD_DIM
    xn = layer_norm16(x, ln_w, ln_b, dtype)
    q, k, v = qkv(xn, wqkv16, bqkv, scale, dtype)
    out = np.zeros((seqs, d), F32)
    for s in range(seqs):
        n = int(pos[s])
        for h in range(H):
            sl = slice(h * HEAD_DIM, (h + 1) * HEAD_DIM)
            K = np.concatenate([k_cache[s, h, :n].astype(F32), k[s:s + 1, sl]])
            V = np.concatenate([v_cache[s, h, :n].astype(F32), v[s:s + 1, sl]])
            out[s, sl] = attend(q[s, sl], K, V, dtype)
    return out, k, v


def split_ranges(n_keys):
    """The key ranges of crossScores / crossSoftmaxPV: eight of ( ( n + 7 ) / 8 + 3 ) & ~3 keys, the trailing ones empty when n is small."""
    per = ((n_keys + CROSS_SPLITS - 1) // CROSS_SPLITS + 3) & ~3
    return [(min(i * per, n_keys), min((i + 1) * per, n_keys)) for i in range(CROSS_SPLITS)]


def cross_query(x, ln_w, ln_b, wq16, bq, scale, dtype=np.float64):
    """q = fp16( ( Wq fp16( LayerNorm( x ) ) + b ) s ), [seqs][d] FP16-valued float32."""
    xn = layer_norm16(x, ln_w, ln_b, dtype)
    return wn.r16(((product(wq16, xn, dtype) + np.asarray(bq, dtype)).astype(dtype) * dtype(scale)).astype(dtype))


def cross_split(x, ln_w, ln_b, wq16, bq, scale, k_cache, v_cache, n_keys, dtype=np.float64):
    """The cross-attention half over keys 0 .. n_keys - 1 of caches FP16 [seqs][H][stride][64]. Returns (scores [seqs][H][n_keys] in `dtype`,
    out [seqs][d] FP16-valued float32 = fp16( sum( e V ) / sum( e ) ) with e = exp16( fp32( score ) - the maximum over all keys ))."""
    seqs, d = x.shape
    H = d // HEAD_DIM
    q = cross_query(x, ln_w, ln_b, wq16, bq, scale, dtype)
    scores = np.zeros((seqs, H, n_keys), dtype)
    out = np.zeros((seqs, d), F32)
    for s in range(seqs):
        for h in range(H):
            sl = slice(h * HEAD_DIM, (h + 1) * HEAD_DIM)
            sc = np.asarray(k_cache[s, h, :n_keys], dtype) @ q[s, sl].astype(dtype)
            scores[s, h] = sc
            s32 = sc.astype(F32)
            e = wn.exp16((s32 - s32.max()).astype(F32))
            tot = e.astype(np.float64).sum()
            pv = e.astype(dtype) @ np.asarray(v_cache[s, h, :n_keys], dtype)
            out[s, sl] = wn.r16(pv * F32(1.0 / tot)) if dtype == np.float32 else wn.r16(pv / tot)
    return scores, out


def combine_partials(part, dtype=np.float32):
    """The combine prologue of gemvSmall on partials [M][H][8][68] (64 FP32 sums, the double sum of the exponentials in floats 64 .. 65): the splits added in
    order, scaled by float( 1 / sum ), rounded to FP16. float32 is the kernel's own arithmetic; float64 divides in double. [M][H*64] FP16-valued float32."""
    part = np.ascontiguousarray(part, F32)
    M, H = part.shape[:2]
    acc = part[:, :, 0, :HEAD_DIM].astype(dtype)
    for s in range(1, CROSS_SPLITS):
        acc = (acc + part[:, :, s, :HEAD_DIM].astype(dtype)).astype(dtype)
    sums = part[:, :, :, HEAD_DIM:HEAD_DIM + 2].copy().view(np.float64)[..., 0]          # [M][H][8]
    tot = sums[:, :, 0].copy()
    for s in range(1, CROSS_SPLITS):
        tot = tot + sums[:, :, s]
    with np.errstate(divide="ignore", invalid="ignore"):
        x = acc * (1.0 / tot).astype(F32)[..., None] if dtype == np.float32 else acc / tot[..., None]
    return wn.r16(x).reshape(M, H * HEAD_DIM)
