"""The timestamp rules ("Timestamp rules") restated in numpy, straight from their definition, for the tests.

The functions take the FULL sampled history of one row -- every token the window has sampled so far, in order -- and look at nothing else. There is no running
record here on purpose: the device kernel keeps one (last token a timestamp, the one before it, the last timestamp id, a count), and a restatement that kept one
as well would share its bookkeeping.

A token is a timestamp when its id is >= beg (<|0.00|>).
  * last token a timestamp and the one before it too (or fewer than two tokens sampled): [beg, nVocab) is masked;
  * last token a timestamp and the one before it not: [0, eot) is masked;
  * any timestamp sampled so far, `last` the latest: [beg, last) is masked in the text-then-timestamp case, [beg, min(last + 1, nVocab)) otherwise;
  * an empty history (the prompt step's sample) masks nothing."""
import numpy as np


def masked_ranges(history, eot, beg, n_vocab):
    """[(lo, hi), ...]: the half-open column ranges that become -inf before the token after `history` is sampled."""
    history = [int(t) for t in history]
    ranges = []
    if not history:
        return ranges
    last_is_ts = history[-1] >= beg
    before_is_ts = len(history) < 2 or history[-2] >= beg
    if last_is_ts:
        ranges.append((beg, n_vocab) if before_is_ts else (0, eot))
    stamps = [t for t in history if t >= beg]
    if stamps:
        hi = stamps[-1] if (last_is_ts and not before_is_ts) else min(stamps[-1] + 1, n_vocab)
        ranges.append((beg, hi))
    return [(lo, hi) for lo, hi in ranges if hi > lo]


def mask(history, eot, beg, n_vocab):
    """bool [n_vocab]: True where the logits become -inf."""
    m = np.zeros(n_vocab, bool)
    for lo, hi in masked_ranges(history, eot, beg, n_vocab):
        m[lo:hi] = True
    return m


def apply(logits, history, eot, beg):
    """A copy of the row `logits` with -inf over the masked columns; every other float keeps its bits."""
    out = np.array(logits, np.float32, copy=True)
    out[mask(history, eot, beg, len(out))] = -np.inf
    return out


def violations(sampled, eot, beg, n_vocab):
    """The indices i >= 1 at which sampled[i] lies in the mask its own history sampled[:i] gives: empty = the sequence obeys all three clauses. Index 0 is the
    prompt step's sample, which the rules leave alone."""
    sampled = [int(t) for t in sampled]
    return [i for i in range(1, len(sampled)) if mask(sampled[:i], eot, beg, n_vocab)[sampled[i]]]


def histories(eot, beg, n_vocab):
    """The histories the tests cover, by name. ts / ts2 are timestamps with ts < ts2, text is a text token."""
    ts, ts2, text = beg + 37, beg + 301, 1234
    return {
        "empty": [],
        "ts": [ts],
        "text": [text],
        "text_ts": [text, ts],
        "ts_ts": [ts, ts2],
        "ts_text": [ts, text],
        "ts_ts_text_ts": [ts, ts, text, ts2],
        "last_is_beg": [text, beg],
        "closed_at_beg": [beg, beg],
        "last_is_top": [text, n_vocab - 1],
        "closed_at_top": [text, n_vocab - 1, n_vocab - 1],
        "text_after_top": [n_vocab - 1, n_vocab - 1, text],
    }
