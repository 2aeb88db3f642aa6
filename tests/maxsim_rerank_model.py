"""The model of the exact MaxSim rerank (include/bbq.h "Exact MaxSim rerank"), in plain Python over the oracle's computeSimilarity:
c(t, r) = O.true_similarity per (token, row); M_t(G) the greatest c(t, r) over the accepted rows of G - a NaN below every number,
numbers by value with -0.0 below +0.0, NaN if every accepted row gives NaN; T = M_0 + M_1 + ... in f64, in ascending token from M_0, a
NaN sum written as the one quiet NaN."""
import numpy as np

import orclib as O

NAN_BITS = 0x7ff8000000000000
CANON_NAN = np.array([NAN_BITS], np.uint64).view(np.float64)[0]
SIGN = np.uint64(1 << 63)


def true_scores(tokens, base, sim):
    """c: f64 [tokens, rows]"""
    return O.true_similarity(tokens, base, sim)


def rank_keys(c):
    """uint64 keys that order f64 values as the maximum does: NaN lowest (1), then -Inf .. -0.0 < +0.0 .. +Inf"""
    c = np.ascontiguousarray(c, np.float64)
    b = c.view(np.uint64)
    k = np.where((b & SIGN) != 0, ~b, b | SIGN)
    return np.where(np.isnan(c), np.uint64(1), k)


def group_max(c_rows):
    """M over the f64 scores of a group's accepted rows (at least one)"""
    c_rows = np.ascontiguousarray(c_rows, np.float64)
    assert c_rows.shape[0] >= 1
    best = c_rows[int(np.argmax(rank_keys(c_rows)))]
    return CANON_NAN if np.isnan(best) else best


def rep_true(c, off, mask, groups):
    """M: f64 [tokens, len(groups)] - per token and listed group (every one live) its greatest accepted true score"""
    out = np.zeros((c.shape[0], len(groups)), np.float64)
    for i, g in enumerate(groups):
        rows = np.arange(off[g], off[g + 1])
        rows = rows[mask[rows]]
        for t in range(c.shape[0]):
            out[t, i] = group_max(c[t, rows])
    return out


def reduce_true(rep):
    """T: f64 [groups] - the ordered sum over the tokens, from M_0, NaN as NAN_BITS"""
    rep = np.ascontiguousarray(rep, np.float64)
    out = np.zeros(rep.shape[1], np.float64)
    with np.errstate(all="ignore"):
        for g in range(rep.shape[1]):
            acc = rep[0, g]
            for t in range(1, rep.shape[0]):
                acc = np.float64(acc + rep[t, g])
            out[g] = CANON_NAN if np.isnan(acc) else acc
    return out


def live_groups(off, mask):
    """the groups with an accepted row, ascending"""
    return np.array([g for g in range(len(off) - 1) if mask[off[g]:off[g + 1]].any()], np.int64)


def scores(c, off, mask, cand):
    """T of every entry of a candidate list, in list order"""
    cand = np.asarray(cand, np.int64)
    if len(cand) == 0:
        return np.zeros(0, np.float64)
    uniq, inv = np.unique(cand, return_inverse=True)
    return reduce_true(rep_true(c, off, mask, uniq))[inv]


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)
