"""The no-repeat n-gram rule ("No-repeat n-grams") restated in numpy, straight from its definition, for the tests.

The functions take the FULL sampled history of one row -- every token the window has sampled so far, timestamps included, in order -- and look at nothing
else. There is no running record here on purpose: the device kernel keeps one (a history row with a count and a cap), and a restatement that kept one as well
would share its bookkeeping.

With h[0 .. L) the history and n the size, the token t is forbidden before the sample at position L when

    exists i, 0 <= i <= L - n:   h[i .. i+n-1) == h[L-n+1 .. L)   and   h[i+n-1] == t   and   t < eot

  * n = 1: the prefix is empty, every text token of the history is forbidden;
  * L < n: nothing is forbidden;
  * only text tokens (id < eot) are ever forbidden: eot, the special ids and the timestamps stay."""
import numpy as np


def banned(history, n, eot):
    """The sorted list of forbidden token ids before the token after `history` is sampled."""
    h = [int(t) for t in history]
    L = len(h)
    if n < 1 or L < n:
        return []
    suffix = h[L - n + 1:L]
    out = set()
    for i in range(0, L - n + 1):
        if h[i:i + n - 1] == suffix:
            t = h[i + n - 1]
            if 0 <= t < eot:
                out.add(t)
    return sorted(out)


def mask(history, n, eot, n_vocab):
    """bool [n_vocab]: True where the logits become -inf."""
    m = np.zeros(n_vocab, bool)
    ids = [t for t in banned(history, n, eot) if t < n_vocab]
    m[ids] = True
    return m


def apply(logits, history, n, eot):
    """A copy of the row `logits` with -inf over the forbidden columns; every other float keeps its bits."""
    out = np.array(logits, np.float32, copy=True)
    out[mask(history, n, eot, len(out))] = -np.inf
    return out


def violations(sampled, n, eot):
    """The indices i at which sampled[i] lies in the mask its own prefix sampled[:i] gives: empty = the sequence obeys the rule."""
    sampled = [int(t) for t in sampled]
    return [i for i in range(len(sampled)) if sampled[i] in banned(sampled[:i], n, eot)]


def alphabet(eot, beg):
    """Six ids on which n-grams recur constantly: three text tokens, eot and two timestamps."""
    return [17, 4242, eot - 1, eot, beg + 3, beg + 250]


def histories(rng, count, length, eot, beg):
    """`count` histories of `length` tokens over alphabet( eot, beg ), text tokens three times as likely as the others; the first is a plain loop a b a b ..."""
    ids = np.array(alphabet(eot, beg))
    p = np.array([3, 3, 3, 1, 1, 1], np.float64)
    out = [[int(ids[k % 2]) for k in range(length)]]
    while len(out) < count:
        out.append([int(t) for t in rng.choice(ids, size=length, p=p / p.sum())])
    return out[:count]
