"""numpy restatement of the voice-activity features (include/whisper_hip.h: wh_vad_features), of the decision loop over them (whisper_amd/host/vad.h) and
of the chunk planner (whisper_amd/host/chunkPlanner.h), shared by tests/test_vad_cpu.py and tests/test_gpu_vad.py. Written from the text of the headers,
not from the code: features in float64 from the exact DFT of the float32-scaled samples, rounded to float32 where the definition rounds; the decision
loop in np.float32 scalars; the planner in Python integers."""
import os

import numpy as np

FRAME = 256
MAX_LEN, MIN_LEN, PAUSE_FRAMES, MIN_TAIL = 480000, 240000, 21, 16000
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
f32 = np.float32


# ---------------------------------------------------------------------------------------------------------------------
# features
# ---------------------------------------------------------------------------------------------------------------------
def frames_of(pcm):
    """x[n] = pcm[n] * 32768.0f of the whole frames, float32 [nFrames][256]; the last partial frame is ignored"""
    pcm = np.asarray(pcm, np.float32)
    n = len(pcm) // FRAME
    return (pcm[:n * FRAME] * f32(32768.0)).reshape(n, FRAME)


def dft_fft(x):
    return np.fft.fft(x.astype(np.float64), axis=1)


def dft_direct(x):
    """The same spectrum as a float64 matrix product with the twiddles cos / -sin( 2 pi ( n k mod 256 ) / 256 )"""
    idx = (np.arange(FRAME)[:, None] * np.arange(FRAME)[None, :]) % FRAME
    ang = 2.0 * np.pi * idx / FRAME
    x = x.astype(np.float64)
    return x @ np.cos(ang) + 1j * (x @ -np.sin(ang))


def features(pcm, dft=dft_fft):
    """(feat float32 [nFrames][3] = energy, F, SFM; power float64 [nFrames][256] = |X|^2). An all-zero frame has energy 0, F 0 and SFM NaN; a frame
    with a bin that is exactly zero has SFM +inf."""
    x = frames_of(pcm)
    n = len(x)
    feat = np.zeros((n, 3), np.float32)
    if n == 0:
        return feat, np.zeros((0, FRAME))
    sq = (x * x).astype(np.float32)                             # the square is rounded to float, the sum is in double
    feat[:, 0] = np.sqrt((sq.astype(np.float64).sum(1) / FRAME).astype(np.float32).astype(np.float64)).astype(np.float32)
    X = dft(x)
    mag = np.abs(X)
    power = X.real ** 2 + X.imag ** 2
    feat[:, 1] = f32(62.5) * np.argmax(power[:, :FRAME // 2], axis=1).astype(np.float32)        # argmax returns the first maximum
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = (np.exp(np.log(mag).sum(1) / FRAME) / (mag.sum(1) / FRAME)).astype(np.float32)
        # log10 of a float, correctly rounded to float: evaluated in double
        feat[:, 2] = f32(-10.0) * np.log10(ratio.astype(np.float64)).astype(np.float32)
    return feat, power


def fragile_frames(power):
    """Frames whose F or SFM another exact evaluation may legitimately give differently: the two largest |X|^2 of bins 0 .. 127 closer than 1e-9
    relative, or a non-zero bin below 1e-7 of the frame's norm."""
    if len(power) == 0:
        return np.zeros(0, bool)
    top = np.sort(power[:, :FRAME // 2], axis=1)[:, -2:]
    tie = (top[:, 1] - top[:, 0]) < 1e-9 * top[:, 1]
    tie &= top[:, 1] > 0
    mag = np.sqrt(power)
    norm = np.sqrt(power.sum(1))[:, None]
    tiny = ((mag > 0) & (mag < 1e-7 * norm)).any(1)
    return tie | tiny


# ---------------------------------------------------------------------------------------------------------------------
# the decision loop
# ---------------------------------------------------------------------------------------------------------------------
def _ulps(a, b):
    """distance of two finite float32 in ulps of the larger operand"""
    big = max(abs(float(a)), abs(float(b)))
    return abs(float(a) - float(b)) / float(np.spacing(f32(big))) if big > 0 else np.inf


def decide(feat):
    """(speech uint8 [nFrames], last_speech, margin): margin = the smallest distance, in float32 ulps of the larger operand, between the two sides of
    any comparison of the loop whose sides are both finite (inf when there is none)."""
    feat = np.asarray(feat, np.float32).reshape(-1, 3)
    n = len(feat)
    speech = np.zeros(n, np.uint8)
    last, margin = 0, np.inf
    m = [f32(0), f32(0), f32(0)]
    run = f32(0)
    thr_fixed = (None, f32(185.0), f32(5.0))
    with np.errstate(all="ignore"):
        for i in range(n):
            cur = [feat[i, 0], feat[i, 1], feat[i, 2]]
            if i == 0:
                m = list(cur)
            elif i < 30:
                # std::min( m, c ): c only when c < m, so a NaN on either side keeps m
                m = [c if c < mm else mm for mm, c in zip(m, cur)]
            thr = [f32(40.0) * np.log10(m[0]), thr_fixed[1], thr_fixed[2]]
            votes = 0
            for k in range(3):
                lhs = cur[k] - m[k]
                if np.isfinite(lhs) and np.isfinite(thr[k]):
                    margin = min(margin, _ulps(lhs, thr[k]))
                if lhs >= thr[k]:
                    votes += 1
            if votes > 1:
                speech[i] = 1
                last = (i + 1) * FRAME
                run = f32(0)
            else:
                run = run + f32(1)
                m[0] = ((run * m[0]) + cur[0]) / (run + f32(1))
    return speech, last, margin


# ---------------------------------------------------------------------------------------------------------------------
# the planner
# ---------------------------------------------------------------------------------------------------------------------
def pauses_of(speech, pause_frames):
    out, i, n = [], 0, len(speech)
    while i < n:
        if speech[i]:
            i += 1
            continue
        b = i
        while b < n and not speech[b]:
            b += 1
        if b - i >= pause_frames:
            out.append((i, b))
        i = b
    return out


def plan(speech, energy, N, max_len=MAX_LEN, min_len=MIN_LEN, pause_frames=PAUSE_FRAMES, rules=None):
    """[(first, count)]; ValueError for parameters the planner refuses. rules (optional list) receives "pause" or "energy" per cut."""
    max_len, min_len, pause_frames = max_len or MAX_LEN, min_len or MIN_LEN, pause_frames or PAUSE_FRAMES
    if not (MIN_TAIL <= min_len <= max_len - 2 * MIN_TAIL and max_len <= MAX_LEN and pause_frames >= 1):
        raise ValueError("E_INVALIDARG")
    n_frames = N // FRAME
    assert len(speech) == n_frames and len(energy) == n_frames
    pauses = pauses_of(speech, pause_frames)
    energy = np.asarray(energy, np.float32).astype(np.float64)
    chunks, start = [], 0
    while N - start > max_len:
        hi = min(start + max_len, N - MIN_TAIL) // FRAME
        lo = -((start + min_len) // -FRAME)
        cut = None
        for a, b in pauses:
            c = min((a + b) // 2, hi)
            if lo <= c and a < c < b:
                cut = c
        if rules is not None:
            rules.append("pause" if cut is not None else "energy")
        if cut is None:
            best = np.inf
            for c in range(lo, hi + 1):
                if c < 10 or c + 11 > n_frames:
                    continue
                s = 0.0
                for k in range(c - 10, c + 11):
                    s += float(energy[k])
                if s < best:
                    best, cut = s, c
            if cut is None:
                cut = hi
        chunks.append((start, FRAME * cut - start))
        start = FRAME * cut
    chunks.append((start, N - start))
    return chunks


# ---------------------------------------------------------------------------------------------------------------------
# recordings
# ---------------------------------------------------------------------------------------------------------------------
def jfk_pcm():
    """the 11 s clip of tests/golden/ref_test_d128.npz: it begins and ends with frames of exact zeros"""
    return np.load(os.path.join(GOLDEN, "ref_test_d128.npz"))["pcm16"].astype(np.float32) / f32(32768.0)


def gap(seconds, seed, amplitude=5e-4):
    return (amplitude * np.random.default_rng(seed).standard_normal(int(seconds * 16000))).astype(np.float32)


def composite(pieces, gaps, seed, lead=0.5):
    """lead seconds of faint noise, then the pieces with a gap of gaps[i] seconds of faint noise behind each. Returns (pcm, [(first, end)] of the gaps
    in samples, the lead included)."""
    parts, spans, pos = [], [], 0
    if lead > 0:
        parts.append(gap(lead, seed))
        spans.append((0, len(parts[-1])))
        pos = len(parts[-1])
    for i, (p, g) in enumerate(zip(pieces, gaps)):
        parts.append(np.asarray(p, np.float32))
        pos += len(p)
        if g > 0:
            parts.append(gap(g, seed + 1 + i))
            spans.append((pos, pos + len(parts[-1])))
            pos += len(parts[-1])
    return np.concatenate(parts).astype(np.float32), spans


def recordings():
    """the recordings of the decision-loop tests: tests/test_vad_cpu.py runs them through the driver, tests/test_gpu_vad.py two of them through api.vad"""
    j = jfk_pcm()
    live = j[8000:]                                          # the clip without its silent lead
    return {
        # 63 s: pieces of the clip between gaps of faint noise, half a second of it in front
        "composite": composite([j, 0.6 * j[::-1], j[20000:150000], j, j[::2], j], [0.7, 1.0, 0.5, 0.8, 0.9, 0.6], 1)[0],
        # begins with speech: the minima of the first 30 frames come from speech
        "speech_first": np.concatenate([live, gap(0.8, 5), j]),
        # a span of exact zeros in the middle: energy 0, SFM NaN there
        "zeros_in_the_middle": np.concatenate([gap(0.5, 7), live[:82000], np.zeros(6000, np.float32), live]),
        # exact zeros at the start: the minima are 0 / NaN from frame 0 on, log10f( 0 )
        "zeros_at_the_start": j,
        "fewer_than_30_frames": j[16000:16000 + 256 * 17 + 100],
        "no_frames": j[16000:16000 + 255],
    }
