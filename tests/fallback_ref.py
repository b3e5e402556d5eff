"""The decoding fallback restated in Python / numpy float64: the generator, the draw and the host rules. The reference has no
temperature anywhere, so this file is the definition the device kernels (tests/test_gpu_fallback.py) and whisper_amd/host/decodeFallback.h
(tests/test_fallback_cpu.py) are held against."""
import math

import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = 0xFFFFFFFF
FLT_MIN = float(np.finfo(np.float32).tiny)


def philox4x32_10(counter, key):
    """Philox4x32-10 (Salmon et al., SC'11) on Python integers: counter 4 words, key 2 words -> 4 words."""
    c0, c1, c2, c3 = counter
    k0, k1 = key
    for _ in range(10):
        p0, p1 = M0 * c0, M1 * c2
        c0, c1, c2, c3 = ((p1 >> 32) ^ c1 ^ k0) & MASK, p1 & MASK, ((p0 >> 32) ^ c3 ^ k1) & MASK, p0 & MASK
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return c0, c1, c2, c3


def uniform(seed, nonce, position, row):
    """u in [0, 1): 53 bits of the block at counter (position, row, nonce, 0) under key (seed & 0xffffffff, seed >> 32); exact in float64."""
    x = philox4x32_10((position & MASK, row & MASK, nonce & MASK, 0), (seed & MASK, (seed >> 32) & MASK))
    return float(((x[0] << 21) | (x[1] >> 11))) * 2.0 ** -53


def uniforms(seed, nonce, positions):
    return np.array([uniform(seed, nonce, int(p), r) for r, p in enumerate(positions)], np.float64)


def sample_best_stats(p, n_vocab, beg, force_ts, initial):
    """tsEnd, sumTs, the best text probability and onlyTs as sampleBestKernel forms them (the sum in float64; rows of the tests keep it away from ties)."""
    ts_end = min(beg + 101, n_vocab) if initial else n_vocab
    sum_ts = float(np.sum(p[beg:ts_end].astype(np.float64)))
    tx = float(p[:beg].max()) if beg > 0 else -1.0
    only_ts = bool(sum_ts > max(tx, -1.0)) or bool(force_ts)
    return ts_end, sum_ts, tx, only_ts


def allowed_mask(n_vocab, beg, sot, solm, tnot, ts_end, only_ts):
    a = np.zeros(n_vocab, bool)
    a[beg:ts_end] = True
    if not only_ts:
        a[:beg] = True
        a[[sot, solm, tnot]] = False
    return a


def draw(p, beg, sot, solm, tnot, force_ts, initial, u):
    """One draw on a float32 row. Returns (id, margin): id None when W == 0 (the device then answers with sampleBest's pick); margin = the distance of u W to the
    nearest prefix boundary, relative to W (a draw closer than 1e-10 may be left out of a comparison: an FP64 sum of 52 k non-negative terms moves by less than
    5.8e-12 relative with its order)."""
    n_vocab = len(p)
    ts_end, _, _, only_ts = sample_best_stats(p, n_vocab, beg, force_ts, initial)
    a = allowed_mask(n_vocab, beg, sot, solm, tnot, ts_end, only_ts)
    w = np.where(a, p.astype(np.float64), 0.0)
    cum = np.cumsum(w)
    W = float(cum[-1])
    if W == 0.0:
        return None, 1.0
    target = u * W
    hit = np.nonzero(a & (cum > target))[0]
    if len(hit):
        tok = int(hit[0])
    else:
        tok = int(np.nonzero(a & (p > 0))[0][-1])
    bounds = np.unique(np.concatenate([[0.0], cum[a & (p > 0)]]))
    margin = float(np.min(np.abs(bounds - target))) / W
    return tok, margin


# ---- host rules -------------------------------------------------------------------------------------------------------------------------------

DEFAULTS = dict(inc=0.2, lpt=-1.0, et=2.4, nth=0.6, seed=0)
ACCEPT, RETRY, SKIP, HAND_OVER = 0, 1, 2, 3


def schedule(inc):
    inc = np.float32(inc)
    out = [np.float32(0.0)]
    if not inc > 0:
        return out
    k = 1
    while True:
        v = np.float32(k) * inc
        if not float(v) <= 1.0 + 1e-6:
            break
        out.append(v)
        k += 1
    return out


def score(tokens, result_len):
    """tokens: [(id, p)]. (avgLogprob, entropy) over tokens[:result_len]."""
    if result_len <= 0:
        return 0.0, 0.0
    s = 0.0
    for _, p in tokens[:result_len]:
        p = float(np.float32(p))
        s += math.log(p if p > FLT_MIN else FLT_MIN)
    n = min(32, result_len)
    counts = {}
    for tid, _ in tokens[result_len - n:result_len]:
        counts[tid] = counts.get(tid, 0) + 1
    h = 0.0
    for tid in sorted(counts):
        q = counts[tid] / n
        h -= q * math.log(q)
    return s / result_len, h


def attempt_failed(prm, scan_failed, result_len, avg, entropy):
    return bool(scan_failed or result_len == 0 or avg < float(np.float32(prm["lpt"])) or (result_len > 32 and entropy < float(np.float32(prm["et"]))))


def attempt_silent(prm, scan_failed, avg, no_speech):
    return bool((not scan_failed) and np.float32(no_speech) > np.float32(prm["nth"]) and avg < float(np.float32(prm["lpt"])))


def plan(prm, seek, attempts):
    """attempts: [(scan_failed, result_len, avg, entropy, no_speech)] in the order they would be decoded. Returns [(index, temperature, nonce, attempts, verdict)]
    up to and including the first verdict that is not RETRY."""
    temps = schedule(prm["inc"])
    out, index = [], 0
    for scan_failed, result_len, avg, entropy, no_speech in attempts:
        rec = [index, float(temps[index]), (seek * 8 + index) & MASK, index + 1]
        if attempt_silent(prm, scan_failed, avg, no_speech):
            verdict = SKIP
        elif not attempt_failed(prm, scan_failed, result_len, avg, entropy):
            verdict = ACCEPT
        elif index + 1 < len(temps):
            verdict = RETRY
        else:
            verdict = HAND_OVER
        out.append(tuple(rec + [verdict]))
        if verdict != RETRY:
            break
        index += 1
    return out


# ---- rows of the draw tests (tests/test_gpu_fallback.py; their margins are checked without a device by tests/test_fallback_cpu.py) -------------

DRAW_KINDS = ("softmax", "ts_above", "initial_cap", "specials", "one_allowed", "only_specials", "zero")
DRAW_SEED, DRAW_NONCE = 0x9E3779B97F4A7C15, 0xC0FFEE


def draw_row(kind, V, sp, rng):
    """One float32 row of probabilities (not necessarily normalised) for a branch of the draw."""
    beg, sot, solm, tnot = sp["beg"], sp["sot"], sp["solm"], sp["not_"]
    if kind == "softmax":                       # a broad distribution: the best text token outweighs the timestamps (the sum rule is false)
        x = (4.0 * rng.standard_normal(V)).astype(np.float64)
        x[beg:] -= 4.0
        e = np.exp(x - x.max())
        return (e / e.sum()).astype(np.float32)
    r = np.zeros(V, np.float32)
    idx = rng.integers(0, beg, 3000)
    r[idx] = rng.uniform(1e-7, 1e-5, len(idx)).astype(np.float32)
    if kind == "ts_above":                      # the sum rule is true: timestamps only
        r[rng.integers(0, beg)] = 0.05
        ts = rng.integers(beg, V, 40)
        r[ts] = rng.uniform(0.001, 0.02, len(ts)).astype(np.float32)
    elif kind == "initial_cap":                 # most timestamp mass above beg + 100: under isInitial only beg .. beg + 100 may be drawn
        r[rng.integers(0, beg)] = 0.01
        r[beg + 101:beg + 400] = rng.uniform(0.001, 0.003, 299).astype(np.float32)
        r[beg + 3:beg + 101:7] = rng.uniform(0.0005, 0.002, 14).astype(np.float32)
    elif kind == "specials":                    # most mass on sot / solm / not, which are never drawn while W > 0
        r[[sot, solm, tnot]] = (0.4, 0.3, 0.2)
        r[rng.integers(0, beg - 200, 50)] = rng.uniform(0.0005, 0.002, 50).astype(np.float32)
    elif kind == "one_allowed":                 # one allowed token with mass
        r[:] = 0
        r[[sot, solm]] = (0.5, 0.25)
        r[int(rng.integers(0, beg - 200))] = 0.125
    elif kind == "only_specials":               # W == 0 with mass on the specials alone
        r[:] = 0
        r[[sot, solm, tnot]] = (0.5, 0.25, 0.125)
    elif kind == "zero":
        r[:] = 0
    return r


def draw_cases(V, sp, rows, first_kind=0):
    """`rows` rows cycling through the kinds from `first_kind`, and one decoder position per row."""
    rng = np.random.default_rng(V * 1000 + rows * 10 + first_kind)
    kinds = [DRAW_KINDS[(first_kind + i) % len(DRAW_KINDS)] for i in range(rows)]
    probs = np.stack([draw_row(k, V, sp, rng) for k in kinds])
    positions = rng.integers(0, 448, rows).astype(np.int32)
    return kinds, probs, positions


def draw_batches(V, sp):
    """The launches of the draw test: every kind alone (1 row), then 5 and 64 rows."""
    return [draw_cases(V, sp, 1, k) for k in range(len(DRAW_KINDS))] + [draw_cases(V, sp, 5), draw_cases(V, sp, 64, 3)]
