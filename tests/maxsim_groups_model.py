"""MaxSim over chosen groups - bbq_score_maxsim_groups_batch, bbq_search_maxsim_groups_batch - restated in numpy on top of the MaxSim
search's model (maxsim_model.rep_scores / reduce) and the oracle's literal heap (orclib.heap_topk): a candidate scores the sum its group
scores in the MaxSim search, and a query's answer is the heap's over its candidates IN THE ORDER GIVEN.  Also the candidate lists the
GPU tests run and what each of them is there to reach (tests/test_maxsim_groups_cpu.py holds them to it)."""
import numpy as np

import maxsim_model as M
import orclib as O

WAVE, PIECE = 64, 256                      # lanes of a wave, expanded rows of a workgroup of the score pass
TOTALS = (64, 65, 256, 257)                # expanded row totals that end on and one behind those two


def scores(rep, live_groups, cand):
    """float32 [len(cand)]: the MaxSim sum of every candidate, duplicates included.  rep [T, L]: the query's tokens' representative
    scores of the L live groups `live_groups` (maxsim_model.rep_scores); every candidate is one of them"""
    cand = np.asarray(cand, np.int64)
    if len(cand) == 0:
        return np.zeros(0, np.float32)
    S = M.reduce(rep)
    slot = np.searchsorted(live_groups, cand)
    assert (np.asarray(live_groups)[slot] == cand).all(), "a candidate that is not live has no score: the call refuses it"
    return S[slot]


def answer(rep, live_groups, cand, k):
    """(groups int32, scores float32) of one query: the reference's heap of min(k, len(cand)) over the candidates in list order"""
    S = scores(rep, live_groups, cand)
    oi, osc = O.heap_topk(S, k)
    return np.asarray(cand, np.int64)[oi].astype(np.int32), osc


def sorted_answer(rep, live_groups, cand, k):
    """what a stable descending sort of the list would answer: differs from `answer` only where scores tie (or are NaN)"""
    S = scores(rep, live_groups, cand)
    order = np.argsort(-S.astype(np.float64), kind="stable")[:max(k, 0)]
    return np.asarray(cand, np.int64)[order].astype(np.int32), S[order]


def first_bad(offsets, mask, lists):
    """(query, position, group) of the first candidate, in call order, that is no group of the set or not live; None if there is none"""
    off = np.asarray(offsets, np.int64)
    for q, cand in enumerate(lists):
        for i, g in enumerate(np.asarray(cand, np.int64)):
            if g < 0 or g >= len(off) - 1 or not np.asarray(mask[off[g]:off[g + 1]], bool).any():
                return q, i, int(g)
    return None


def positions(offsets, cand):
    """int64 [len(cand) + 1]: where each candidate's first row stands among the query's expanded rows; the last entry is their total"""
    off = np.asarray(offsets, np.int64)
    cand = np.asarray(cand, np.int64)
    pos = np.zeros(len(cand) + 1, np.int64)
    pos[1:] = np.cumsum(off[cand + 1] - off[cand])
    return pos


def cut_by(offsets, cand, step):
    """the positions in `cand` of the candidates whose expanded rows lie on both sides of a multiple of `step`"""
    pos = positions(offsets, cand)
    return [i for i in range(len(cand)) if pos[i] // step != (pos[i + 1] - 1) // step]


def list_with_total(offsets, live_groups, target, seed):
    """distinct live groups, shuffled, whose rows number exactly `target`; None where the greedy pass over the shuffle does not get there"""
    off = np.asarray(offsets, np.int64)
    order = np.random.default_rng(seed).permutation(np.asarray(live_groups, np.int64))
    out, left = [], target
    for g in order:
        size = int(off[g + 1] - off[g])
        if size <= left:
            out.append(int(g))
            left -= size
    return np.array(out, np.int64) if left == 0 and out else None


def candidate_lists(offsets, live_groups, seed=20):
    """the lists of one (layout, mask), by name: every live group ascending; the same reversed; a seeded subset with duplicates; one
    candidate; none; and, where the layout can make them, lists of exactly 64, 65, 256 and 257 expanded rows"""
    live = np.asarray(live_groups, np.int64)
    rng = np.random.default_rng(seed + len(live))
    out = {"ascending": live.copy(), "reversed": live[::-1].copy(), "empty": np.zeros(0, np.int64)}
    if len(live):
        sub = rng.choice(live, size=min(len(live), 37))              # with replacement ...
        out["random_dups"] = np.concatenate([sub, sub[:3], [sub[0]]])  # ... and four certain duplicates, one of them three times
        out["one"] = live[[len(live) // 2]]
        for t in TOTALS:
            lst = list_with_total(offsets, live, t, seed + t)
            if lst is not None:
                out["total_%d" % t] = lst
    return out
