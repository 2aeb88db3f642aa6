"""The model the exact search is held to, composed of what tests/orclib.py pins to the reference through the rerank_* goldens:
computeSimilarity for every (query, row) from the oracle, the reference's stable descending sort over the accepted rows, the first k
(getTrueTopK, reference tests/recall-common.ts:143-149), mapped back through the accepted rows.  Beside it the ranking of include/bbq.h
restated in numpy - true_key of the score's bits descending, equal keys by ascending row - which is what a row of scores with a NaN is
ranked by: there the reference's comparator leaves the order to the engine."""
import numpy as np

import orclib as O

NAN_BITS = np.uint64(0x7ff8000000000000)
SIGN = np.uint64(0x8000000000000000)


def canon64(a):
    a = np.array(a, np.float64)
    a[np.isnan(a)] = np.nan
    return a.view(np.uint64)


def scores(queries, base, sim):
    """c(q, r) for every query and row: float64 [nq, n], read-only"""
    c = O.true_similarity(np.atleast_2d(queries), base, sim)
    c.setflags(write=False)
    return c


def true_key(score_row):
    """true_key (bbq_device.h) of every score: 1 for a NaN, ~bits for a negative number, bits | 2^63 otherwise"""
    s = np.ascontiguousarray(score_row, np.float64)
    bits = s.view(np.uint64)
    key = np.where(bits >> np.uint64(63) != 0, ~bits, bits | SIGN)
    return np.where(np.isnan(s), np.uint64(1), key)


def by_key(score_row, k, accepted=None):
    """the header's ranking with a plain sorted() over (-key, row): (rows, score bits with a NaN as NAN_BITS)"""
    s = np.ascontiguousarray(score_row, np.float64)
    rows = np.arange(s.shape[0]) if accepted is None else np.flatnonzero(accepted)
    key = true_key(s)
    order = sorted((-int(key[r]), int(r)) for r in rows)[:max(int(k), 0)]
    idx = np.array([r for _, r in order], np.int32)
    return idx, canon64(s[idx])


def topk(score_row, k, accepted=None):
    """the model: (rows int32, score bits uint64) of the first min(k, accepted rows) rows.  A row of scores without a NaN goes through
    the oracle's sort, and the header's ranking has to say the same; with a NaN only the header's ranking is defined"""
    s = np.ascontiguousarray(score_row, np.float64)
    rows = np.arange(s.shape[0]) if accepted is None else np.flatnonzero(accepted)
    want = by_key(s, k, accepted)
    if k <= 0 or rows.shape[0] == 0 or np.isnan(s[rows]).any():
        return want
    pos = O.rerank_select(s[rows], int(k), "sort")
    idx = rows[pos].astype(np.int32)
    bits = canon64(s[idx])
    assert idx.tolist() == want[0].tolist() and bits.tolist() == want[1].tolist(), "the header's ranking is not the oracle's sort"
    return idx, bits
