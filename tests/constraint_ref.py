"""Constrained decoding ("Constrained decoding") restated without a table of bits: every question is answered by walking bytes.

A constraint is ( class_of [256], trans [nStates][nClasses] with -1 = no transition, accept [nStates], start ) and the vocabulary's byte strings
( tok_offsets [eot + 1], tok_bytes ). A state is an int, -1 = dead."""
import numpy as np


def token_bytes(tok_offsets, tok_bytes, t):
    return bytes(bytearray(tok_bytes[int(tok_offsets[t]):int(tok_offsets[t + 1])]))


def walk_bytes(class_of, trans, s, data):
    """The state after `data` from s; -1 as soon as a transition is missing or when s is -1. (No bytes leave s where it is: prefixes use this.)"""
    s = int(s)
    for b in data:
        if s < 0:
            return -1
        s = int(trans[s][int(class_of[b])])
    return s if s >= 0 else -1


def walk(class_of, trans, s, data):
    """walk( s, t ) for a token that spells `data`: a token of zero bytes is dead from everywhere."""
    return walk_bytes(class_of, trans, s, data) if len(data) else -1


def allowed_words(class_of, trans, tok_offsets, tok_bytes, eot):
    """uint32 [nStates][ceil( eot / 32 )]: bit t % 32 of word t / 32 of line s = walk( s, t ) != -1. (All states of a token at once: one numpy gather per byte.)"""
    trans = np.asarray(trans, np.int64)
    n_states = trans.shape[0]
    dead = np.concatenate([trans, np.full((1, trans.shape[1]), -1, np.int64)])   # line -1: the dead state stays dead
    out = np.zeros((n_states, (eot + 31) // 32), np.uint32)
    for t in range(eot):
        data = token_bytes(tok_offsets, tok_bytes, t)
        cur = np.arange(n_states) if len(data) else np.full(n_states, -1)
        for b in data:
            cur = dead[cur, int(class_of[b])]
        out[:, t // 32] |= (cur >= 0).astype(np.uint32) << np.uint32(t % 32)
    return out


def advance(class_of, trans, tok_offsets, tok_bytes, s, tok, eot):
    """The state after the sampled token: a text token walks its bytes, an id >= eot leaves the state."""
    return int(s) if tok >= eot else walk(class_of, trans, s, token_bytes(tok_offsets, tok_bytes, tok))


def dead_tokens(class_of, trans, tok_offsets, tok_bytes, s, eot):
    """bool [eot]: walk( s, t ) == -1"""
    return np.array([walk(class_of, trans, s, token_bytes(tok_offsets, tok_bytes, t)) < 0 for t in range(eot)], bool)


def apply(row, dead, s, accept, eot, penalty):
    """The row (float32, copied) with the penalty subtracted, in float32, from every text token that dies from s (dead = dead_tokens of s) and from eot unless s
    accepts or is dead. -inf - inf is -inf."""
    out = np.array(row, np.float32, copy=True)
    p = np.float32(penalty)
    out[:eot][dead] = out[:eot][dead] - p
    if s >= 0 and not accept[s] and eot < len(out):
        out[eot] = out[eot] - p
    return out
