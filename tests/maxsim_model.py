"""The MaxSim search's contract restated in numpy: per token vector the representatives of the live groups by the grouped search's rule
(test_groups_cpu.representatives) over the oracle's per-row f32 scores, the ordered f64 sum of their scores per group, and the oracle's
literal heap over the live groups in ascending group number.  The status rule is the span search's over the sums."""
import numpy as np

import orclib as O
import test_groups_cpu as GC
import test_spans_cpu as SC


def rep_scores(s32_of_tokens, offsets, mask):
    """(float32 [T, L]: token t's representative's score of every live group; int64 [L]: the live groups' numbers, ascending).
    s32_of_tokens: per token vector the f32 score of every row of the index"""
    rows, groups = [], None
    for s32 in s32_of_tokens:
        ords, g = GC.representatives(s32, offsets, mask)
        assert groups is None or (g == groups).all()          # which groups are live does not depend on the token
        groups = g
        rows.append(np.asarray(s32, np.float32)[ords])
    return np.array(rows, np.float32).reshape(len(rows), len(groups)), groups


def reduce(rep):
    """S[slot] = (float)((double)rep[0][slot] + (double)rep[1][slot] + ...): the f64 adds in ascending token, from rep[0] and not from
    0.0, one rounding at the end"""
    rep = np.asarray(rep, np.float32)
    assert rep.ndim == 2 and rep.shape[0] >= 1
    acc = rep[0].astype(np.float64)
    for t in range(1, rep.shape[0]):
        acc = acc + rep[t].astype(np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        return acc.astype(np.float32)


def answer(s32_of_tokens, offsets, mask, k):
    """(groups, scores, status, L) of one query"""
    rep, groups = rep_scores(s32_of_tokens, offsets, mask)
    S = reduce(rep) if len(groups) else np.zeros(0, np.float32)
    oi, osc = O.heap_topk(S, k)
    return groups[oi].astype(np.int32), osc, SC.expected_status(S, k), len(groups)
