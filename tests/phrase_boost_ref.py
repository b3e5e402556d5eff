"""Phrase boosting by brute force ("Phrase boosting"): the definition restated with no automaton, in numpy float32.

A context holds phrases (each 1 .. 16 text-token ids in [0, eot)) and one boost. For a row, h = the text tokens it has sampled since its last non-text token
(any id >= eot empties h). The offered set O(h) = { t : for some suffix u of h, the empty one included, u . t is a prefix of a phrase }. Before the softmax,
logits[t] += boost for every t in O(h), once each; every other float keeps its bits.

Also the phrase sets and histories the tests run: sets( eot ) and histories( phrases, eot, V, seed )."""
import numpy as np


def tail(samples, eot):
    """h: the text tokens since the last sampled id >= eot"""
    h = []
    for t in samples:
        h = h + [int(t)] if 0 <= int(t) < eot else []
    return h


def offered(phrases, h):
    """O(h), by trying every suffix of h against every phrase"""
    h = [int(t) for t in h]
    out = set()
    for k in range(len(h) + 1):
        u = h[len(h) - k:]
        for p in phrases:
            p = [int(t) for t in p]
            if len(p) > k and p[:k] == u:
                out.add(p[k])
    return out


def longest(phrases, h):
    """The longest suffix of h that is a prefix of a phrase: what an automaton's state stands for"""
    h = [int(t) for t in h]
    for k in range(min(len(h), 16), 0, -1):
        u = h[len(h) - k:]
        if any([int(t) for t in p[:k]] == u and len(p) >= k for p in phrases):
            return tuple(u)
    return ()


def apply(row, phrases, samples, eot, boost):
    """The row a step hands to the softmax when the row's samples so far are `samples`: a copy, float32"""
    out = np.array(row, np.float32, copy=True)
    cols = np.array(sorted(offered(phrases, tail(samples, eot))), np.int64)
    out[cols] = out[cols] + np.float32(boost)
    return out


def sets(eot):
    """name -> phrases. a .. e are five text tokens away from the edges."""
    a, b, c, d, e = 1000, 1001, 2002, 3003, 40004 % (eot - 2) + 1
    assert eot >= 1100 and len({a, b, c, d, e}) == 5
    out = {
        "one token": [[a]],
        "shared prefix": [[a, b, c], [a, b, d]],
        "interior prefix": [[a, b, c, d], [b, c, e]],                               # after a b c the state's failure link is b c, no root
        "self overlap": [[a, a, a]],
        "suffix of another": [[a, b, c], [b, c], [c]],
        "duplicates": [[a, b], [a, b], [c], [a, b]],
        "edge ids": [[0], [eot - 1], [eot - 1, 0, eot - 2], [0, 0, eot - 1], [eot - 3, a]],
        "sixteen": [[a, b, c, d, e, a, a, b, c, d, e, e, b, a, c, d], [a, a, b, d]],
        "many first tokens": [[7 + 3 * i] + ([a, 7 + 3 * ((i + 1) % 1024)] if i % 5 == 0 else []) for i in range(1024)],
    }
    for ps in out.values():
        assert all(1 <= len(p) <= 16 and all(0 <= t < eot for t in p) for p in ps) and len(ps) <= 1024
    return out


def histories(phrases, eot, V, seed, count=6, length=24):
    """`count` sample sequences of `length` ids: stretches of phrases from any offset, broken off anywhere, tokens of the set out of order, foreign text
    tokens, timestamps and eot mixed in"""
    rng = np.random.default_rng(seed)
    alphabet = sorted({t for p in phrases for t in p})
    out = []
    for _ in range(count):
        s = []
        while len(s) < length:
            kind = rng.integers(0, 10)
            if kind < 5:
                p = phrases[rng.integers(0, len(phrases))]
                i = rng.integers(0, len(p))
                s += p[i:i + 1 + rng.integers(0, len(p) - i)]
            elif kind < 7:
                s.append(alphabet[rng.integers(0, len(alphabet))])
            elif kind == 7:
                s.append(int(rng.integers(0, eot)))
            elif kind == 8:
                s.append(int(rng.integers(eot, max(V, eot + 1))))                  # eot itself, a special token or a timestamp
            else:
                s.append(eot)
        out.append([int(t) for t in s[:length]])
    return out
