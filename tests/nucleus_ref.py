"""Top-k and nucleus sampling restated in float64 ("Top-k and nucleus sampling"): which entries of a row of logits become -inf.

The order is ( value descending, id ascending ) over the entries above -inf; NaN and -inf are nobody's entry. top_k keeps the first k (a row with k or fewer entries
is left alone); top_p < 1 keeps, of those, the shortest prefix whose cumulative softmax( x * inv_t ) reaches top_p, never none."""
import numpy as np

MARGIN = 1e-3


def order(x):
    """ids of the entries of the float32 row x, likeliest first"""
    ids = np.flatnonzero(x > -np.inf)
    return ids[np.argsort(-x[ids].astype(np.float64), kind="stable")]


def discarded(x, top_k, top_p, inv_t, ranked=None, margin=MARGIN):
    """bool [len(x)]: the entries that become -inf. Asserts the condition on the INPUT that makes an exact comparison fair: the cumulative mass at the cut and one
    entry before it are each MARGIN away from top_p, far beyond what single-precision exponentials and the fixed-point sum can move them (margin = 0: rows that are
    not designed, a model's)."""
    ranked = order(x) if ranked is None else ranked
    keep = ranked[:top_k] if 0 < top_k < len(ranked) else ranked
    if top_p < 1.0 and len(keep):
        z = x[keep].astype(np.float64) * float(inv_t)
        e = np.exp(z - z[0])
        cum = np.cumsum(e / e.sum())
        cut = int(np.argmax(cum >= top_p)) if cum[-1] >= top_p else len(cum) - 1
        assert abs(cum[cut] - top_p) >= margin and (cut == 0 or abs(cum[cut - 1] - top_p) >= margin), (top_k, top_p, cum[max(cut - 1, 0):cut + 1])
        keep = keep[:cut + 1]
    gone = np.zeros(len(x), bool)
    gone[ranked] = True
    gone[keep] = False
    return gone
