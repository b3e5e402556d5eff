"""numpy / plain Python restatement of the span rules and the time map of whisper_amd/host/speechSpans.h, shared by tests/test_speech_spans_cpu.py and
tests/test_gpu_speech_filter.py. Written from the rules as the header's comment states them, in Python integers: frames for the rules, samples and 100 ns
ticks for the map."""
import numpy as np

FRAME = 256
MIN_SILENCE, MIN_SPEECH, PAD = 125, 16, 25
MAX_PARAM = 1 << 20
TICKS = 625          # 100 ns ticks per sample at 16 kHz


def spans(speech, N, min_silence=0, min_speech=0, pad=0):
    """[(a, b)] in samples; ValueError for parameters the header refuses. 0 selects a parameter's default."""
    for v in (min_silence, min_speech, pad):
        if v < 0 or v > MAX_PARAM:
            raise ValueError("E_INVALIDARG")
    min_silence, min_speech, pad = min_silence or MIN_SILENCE, min_speech or MIN_SPEECH, pad or PAD
    speech = np.asarray(speech, np.uint8)
    n = N // FRAME
    assert len(speech) == n
    # 1. maximal runs: where the padded flags change
    edges = np.flatnonzero(np.diff(np.concatenate([[0], (speech != 0).astype(np.int8), [0]])))
    runs = [(int(a), int(b)) for a, b in zip(edges[0::2], edges[1::2])]
    # 2. merge across short gaps
    merged = []
    for a, b in runs:
        if merged and a - merged[-1][1] < min_silence:
            merged[-1] = (merged[-1][0], b)
        else:
            merged.append((a, b))
    # 3. drop short runs
    kept = [(a, b) for a, b in merged if b - a >= min_speech]
    # 4. pad, clamp, merge what touches
    out = []
    for a, b in kept:
        a, b = max(a - pad, 0), min(b + pad, n)
        if out and a <= out[-1][1]:
            out[-1] = (out[-1][0], max(out[-1][1], b))
        else:
            out.append((a, b))
    # 5. samples; the span that reaches the last frame takes the partial frame behind it
    return [(a * FRAME, N if b == n else b * FRAME) for a, b in out]


def pack(pcm, sp, channels=1):
    """the packed copy: the spans' samples one after the other (interleaved frames of `channels`)"""
    pcm = np.asarray(pcm)
    if not sp:
        return pcm[:0].copy()
    return np.concatenate([pcm[a * channels:b * channels] for a, b in sp])


def offsets(sp):
    out = [0]
    for a, b in sp:
        out.append(out[-1] + (b - a))
    return out


def map_start(sp, s):
    """packed sample position -> position in the recording, the start rule; a position behind the packed copy lies as far behind the last span's end"""
    out = offsets(sp)
    if s >= out[-1]:
        return sp[-1][1] + (s - out[-1])
    s = max(s, 0)
    for i, (a, b) in enumerate(sp):
        if out[i] <= s < out[i + 1]:
            return a + (s - out[i])
    raise AssertionError("unreachable")


def map_end(sp, s):
    if s <= 0:
        return sp[0][0]
    return map_start(sp, s - 1) + 1


def start_ticks(sp, t):
    t = max(int(t), 0)
    s = t // TICKS
    return map_start(sp, s) * TICKS + (t - s * TICKS)


def end_ticks(sp, t):
    t = max(int(t), 0)
    s = -(-t // TICKS)
    if s == 0:
        return map_end(sp, 0) * TICKS
    return map_end(sp, s) * TICKS - (s * TICKS - t)
