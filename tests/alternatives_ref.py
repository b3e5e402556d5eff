"""Token alternatives (DESIGN.md section 7 "Token alternatives"; wh_op_top_logprobs) restated in float64. This is the definition, not the kernel's algorithm."""
import numpy as np


def top_logprobs(row, k):
    """row: FP32 logits. Returns ( ids int32 [k], logprob float64 [k] ): the k largest entries, descending, equal values in ascending id, with
    logprob = x - lse and lse = max + log( sum exp( x - max ) ) over the entries above -inf (NaN counts as -inf). Fewer than k such entries: -1 / -inf."""
    x = np.asarray(row, np.float32)
    with np.errstate(invalid="ignore"):
        live = np.nonzero(x > -np.inf)[0]
    ids, lp = np.full(k, -1, np.int32), np.full(k, -np.inf, np.float64)
    if len(live):
        v = x[live].astype(np.float64)
        lse = v.max() + np.log(np.exp(v - v.max()).sum())
        order = np.lexsort((live, -v))[:k]
        ids[:len(order)], lp[:len(order)] = live[order], v[order] - lse
    return ids, lp
