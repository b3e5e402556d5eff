"""The score of a given token under a row of logits (wh_token_score, include/whisper_hip.h; DESIGN.md section 7 "Scoring"), restated in float64 numpy.

A row of logits x[0 .. V) and a target id t give
    logprob     = x[t] - m - ln sum_j exp(x[j] - m),  m = max_j x[j]
    bestLogprob = -ln sum_j exp(x[j] - m)             (the log-probability of the arg-max)
    best        = the lowest id j with x[j] == m
    rank        = #{j : x[j] > x[t]} + #{j < t : x[j] == x[t]}   (0: t is what an arg-max with ties to the lower id takes)
An entry of -inf adds 0 to the sum; a target at -inf scores -inf with a finite bestLogprob. Every row has a finite entry."""
import numpy as np

SCORE_DT = np.dtype([("logprob", "<f8"), ("bestLogprob", "<f8"), ("best", "<i4"), ("rank", "<i4")])


def score_row(x, t):
    """One record of a row x (any float type, taken as float64 values) and a target id t: (logprob, bestLogprob, best, rank)."""
    x = np.asarray(x, np.float64)
    t = int(t)
    assert x.ndim == 1 and 0 <= t < x.size and np.isfinite(x.max())
    m = x.max()
    with np.errstate(invalid="ignore"):
        e = np.where(np.isneginf(x), 0.0, np.exp(x - m))
    ln_s = np.log(e.sum())
    rank = int((x > x[t]).sum()) + int((x[:t] == x[t]).sum())
    return float(x[t] - m - ln_s), float(-ln_s), int(np.argmax(x)), rank     # (argmax returns the first of equal maxima)


def score_rows(x, targets):
    """Rows x [rows][V] against targets [rows]: a structured array [rows] of SCORE_DT."""
    x = np.asarray(x)
    out = np.zeros(x.shape[0], SCORE_DT)
    for r in range(x.shape[0]):
        out[r] = score_row(x[r], targets[r])
    return out
