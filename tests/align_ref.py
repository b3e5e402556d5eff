"""Word-level timestamps from cross-attention: the definition, restated in numpy (DESIGN.md "Token alignment").

align_matrix evaluates steps 3 and 4 of the definition in the floating-point type it is given (float64 = the reference, float32 = the
straightforward single-precision evaluation whose distance from float64 sets the tolerance of tests/test_gpu_align.py); dtw is step 5
and always runs in float32, like the device.
"""
from __future__ import annotations

import numpy as np


def median7_reflect(z):
    """Median of 7 along the last axis with reflect padding (-1 -> 1, -2 -> 2, -3 -> 3, mirrored at the end); rows of 3 keys or fewer stay as they are."""
    n = z.shape[-1]
    if n <= 3:
        return z.copy()
    padded = np.pad(z, [(0, 0)] * (z.ndim - 1) + [(3, 3)], mode="reflect")
    win = np.lib.stride_tricks.sliding_window_view(padded, 7, axis=-1)
    return np.sort(win, axis=-1)[..., 3]


def head_weights(q, k, dtype=np.float64):
    """q [L][64], k [nKeys][64] (the FP16 values): softmax -> column standardisation over the L rows -> median filter. [L][nKeys] in `dtype`."""
    q = np.asarray(q).astype(dtype)
    k = np.asarray(k).astype(dtype)
    s = q @ k.T
    e = np.exp(s - s.max(axis=1, keepdims=True))
    p = e / e.sum(axis=1, keepdims=True, dtype=dtype)
    mean = p.mean(axis=0, keepdims=True, dtype=dtype)
    std = np.sqrt(((p - mean) ** 2).mean(axis=0, keepdims=True, dtype=dtype))
    z = np.where(std > 0, (p - mean) / np.where(std > 0, std, 1), 0).astype(dtype)
    return median7_reflect(z)


def align_matrix(q, k, heads, rows, n_keys, dtype=np.float64):
    """q [layers][rowsMax][H*64], k [layers][T][H*64] (token-major, as wh_debug_read gives "align-q" / "cross-k" for one window), heads = (layer, head)
    pairs in the fixed order. M [rows][n_keys] = the mean over the heads, summed in that order."""
    acc = np.zeros((rows, n_keys), dtype)
    for (l, h) in heads:
        acc = acc + head_weights(q[l][:rows, h * 64:(h + 1) * 64], k[l][:n_keys, h * 64:(h + 1) * 64], dtype)
    return acc / dtype(len(heads))


def dtw(x):
    """x [R][nKeys] float32 costs. Returns (frames [R], path): frames[r] = the smallest key index of the path inside row r."""
    x = np.asarray(x, np.float32)
    R, N = x.shape
    inf = np.float32(np.inf)
    cost = np.full((R + 1, N + 1), inf, np.float32)
    trace = np.full((R + 1, N + 1), -1, np.int8)
    cost[0, 0] = 0
    with np.errstate(invalid="ignore"):
        for i in range(1, R + 1):
            for j in range(1, N + 1):
                c0, c1, c2 = cost[i - 1, j - 1], cost[i - 1, j], cost[i, j - 1]
                if c0 < c1 and c0 < c2:
                    t = 0
                elif c1 < c0 and c1 < c2:
                    t = 1
                else:
                    t = 2
                cost[i, j] = np.float32(x[i - 1, j - 1] + min(c0, c1, c2))
                trace[i, j] = t
    trace[0, :] = 2
    trace[:, 0] = 1
    i, j = R, N
    frames = np.full(R, N, np.int64)
    path = []
    while i > 0 or j > 0:
        path.append((i - 1, j - 1))
        if i > 0:
            frames[i - 1] = min(frames[i - 1], max(j - 1, 0))
        t = trace[i, j]
        if t == 0:
            i -= 1
            j -= 1
        elif t == 1:
            i -= 1
        else:
            j -= 1
    return frames.astype(np.int32), path[::-1]


def dtw_fast(x):
    """The same recurrence, anti-diagonal by anti-diagonal (vectorised): for the 256 x 1500 case of the GPU tests."""
    x = np.asarray(x, np.float32)
    R, N = x.shape
    inf = np.float32(np.inf)
    cost = np.full((R + 1, N + 1), inf, np.float32)
    trace = np.full((R + 1, N + 1), 2, np.int8)
    cost[0, 0] = 0
    with np.errstate(invalid="ignore"):
        for d in range(2, R + N + 1):
            i = np.arange(max(1, d - N), min(R, d - 1) + 1)
            j = d - i
            c0, c1, c2 = cost[i - 1, j - 1], cost[i - 1, j], cost[i, j - 1]
            t = np.where((c0 < c1) & (c0 < c2), 0, np.where((c1 < c0) & (c1 < c2), 1, 2))
            cost[i, j] = x[i - 1, j - 1] + np.minimum(np.minimum(c0, c1), c2)
            trace[i, j] = t
    trace[0, :] = 2
    trace[:, 0] = 1
    i, j = R, N
    frames = np.full(R, N, np.int64)
    while i > 0 or j > 0:
        if i > 0:
            frames[i - 1] = min(frames[i - 1], max(j - 1, 0))
        t = trace[i, j]
        if t == 0:
            i -= 1
            j -= 1
        elif t == 1:
            i -= 1
        else:
            j -= 1
    return frames.astype(np.int32)


def token_times(ids, frames, seek, seg_t0, token_beg, token_eot):
    """Step 6: (t0, t1) in 10 ms units for every token of a segment list `ids` (text, timestamp and other special tokens mixed), given the frames of the
    window's text tokens in order (frames[k] for text token k, frames[n] for the eot row)."""
    out = []
    k = 0
    prev = seg_t0
    for t in ids:
        if t >= token_beg:
            t0 = t1 = seek + 2 * (t - token_beg)
        elif t >= token_eot:
            t0 = t1 = prev
        else:
            t0, t1 = seek + 2 * int(frames[k]), seek + 2 * int(frames[k + 1])
            k += 1
        out.append((t0, t1))
        prev = t1
    return out
