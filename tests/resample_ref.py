"""numpy restatement of the resampler of whisper_amd/csrc/resample.hip (include/whisper_hip.h: wh_resample), shared by tests/test_resample_cpu.py and
tests/test_gpu_resample.py. Written from the text of the header, not from the kernel: rational polyphase resampling with a Kaiser-windowed sinc,
taps evaluated in double and rounded once to float, sums in float64 over the float taps."""
from math import gcd

import numpy as np

ZEROS, ROLLOFF, BETA = 32, 0.9475937167399596, 14.769656459379492
OUT_RATE = 16000
U8, S16, S24, S32, F32 = range(5)           # wh_pcm_format
BYTES = {U8: 1, S16: 2, S24: 3, S32: 4, F32: 4}


def design(fin):
    """(L, M, half, K, taps float32 [L][K])"""
    g = gcd(fin, OUT_RATE)
    L, M = OUT_RATE // g, fin // g
    w = ROLLOFF * min(fin, OUT_RATE) / fin              # cutoff as a fraction of the input Nyquist
    half = int(np.ceil(ZEROS / w))
    K = 2 * half + 2
    p = np.arange(L, dtype=np.float64)[:, None] / L
    k = np.arange(K, dtype=np.float64)[None, :]
    d = k - half - p
    x = d / (half + 1.0)
    win = np.where(np.abs(x) < 1, np.i0(BETA * np.sqrt(np.clip(1 - x * x, 0, None))) / np.i0(BETA), 0.0)
    h = w * np.sinc(w * d) * win
    return L, M, half, K, h.astype(np.float32)


def out_len(n_frames, L, M):
    return (n_frames * L + M - 1) // M


def resample(x, L, M, half, K, taps):
    """y[n] = sum_k taps[p][k] x[base - half + k] in float64; x mono (float32 values), zero outside."""
    n_out = out_len(len(x), L, M)
    n = np.arange(n_out, dtype=np.int64)
    base, ph = (n * M) // L, (n * M) % L
    xp = np.concatenate([np.zeros(half), np.asarray(x, np.float64), np.zeros(K + M)])
    idx = base[:, None] + np.arange(K)[None, :]
    return (xp[idx] * taps[ph].astype(np.float64)).sum(1)


def block_outputs(L, M, K):
    """Outputs one workgroup owns (the rule stated at wh_resample in whisper_hip.h): the sizes at which the kernel's blocks begin and end."""
    return min(1024, max(64, ((8191 - K) * L // M + 1) // 64 * 64))


def to_float(raw, fmt):
    """Samples of a format as float32, by the formulas of the header. raw: uint8 / int16 / int32 (s24: int32 values in [-2^23, 2^23), s32: int32) / float32."""
    if fmt == U8:
        return ((raw.astype(np.int32) - 128).astype(np.float32) / np.float32(128.0)).astype(np.float32)
    if fmt == S16:
        return (raw.astype(np.float32) / np.float32(32768.0)).astype(np.float32)
    if fmt == S24:
        return (raw.astype(np.float32) / np.float32(8388608.0)).astype(np.float32)
    if fmt == S32:
        return (raw.astype(np.float64) * 2.0 ** -31).astype(np.float32)
    return raw.astype(np.float32)


def downmix(x, channel):
    """x float32 [n, C] -> mono float32: channel >= 0 that channel, -1 the FP32 sum in channel order times 1.0f / C."""
    if channel >= 0:
        return x[:, channel].copy()
    s = x[:, 0].astype(np.float32)
    for c in range(1, x.shape[1]):
        s = (s + x[:, c]).astype(np.float32)
    return (s * (np.float32(1.0) / np.float32(x.shape[1]))).astype(np.float32)


def pack(raw, fmt):
    """The bytes of the samples as they lie in a file / in device memory (little endian; s24 three bytes each)."""
    if fmt == S24:
        v = raw.astype("<i4").reshape(-1)
        b = v.view(np.uint8).reshape(-1, 4)[:, :3]
        return np.ascontiguousarray(b).reshape(-1)
    dt = {U8: np.uint8, S16: "<i2", S32: "<i4", F32: "<f4"}[fmt]
    return np.ascontiguousarray(raw.astype(dt)).reshape(-1).view(np.uint8)


def ulp32(v):
    return np.spacing(np.abs(np.asarray(v, np.float64)).astype(np.float32)).astype(np.float64)
