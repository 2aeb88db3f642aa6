"""CPU: the span search's contract restated in numpy - span expansion and the rule that says which path answers a query
(bbq_search_spans_batch's out_status) - and, from the goldens and the oracle alone, a check that the inputs tests/test_gpu_spans.py runs
exercise both paths: the device's selection for at least half of their cases, the host's heap because of equal scores on every tie
fixture."""
import functools

import numpy as np
import pytest

import orclib as O
import test_gpu_score_ords as SO          # FIXTURES: the names alone (nothing here touches a device)

SELECT_MAX = 4096                         # largest k the device selects for
TIE_FIXTURES = ["ties_cos_qb4", "ties_euc_qb4", "ib2_ties_cos_qb4"]


def spans_of(pairs):
    return np.asarray(pairs, np.int64).reshape(-1, 2)


def expand(spans):
    """the rows a span list visits, in visiting order"""
    sp = spans_of(spans)
    return np.concatenate([np.arange(b, e) for b, e in sp]) if len(sp) else np.zeros(0, np.int64)


def spans_are_valid(spans, n):
    sp = spans_of(spans)
    return bool((sp[:, 0] >= 0).all() and (sp[:, 0] <= sp[:, 1]).all() and (sp[:, 1] <= n).all() and (sp[1:, 0] >= sp[:-1, 1]).all())


def expected_status(visited, k):
    """out_status of a query whose visited rows score `visited` (f32, visiting order): 0 - the device selects the answer - exactly when
    L > k, 1 <= k <= 4096, no score is NaN and no two of the k + 1 largest scores compare equal as floats (+0.0 == -0.0); 0 as well
    for k == 0 or L == 0, where there is nothing to answer"""
    s = np.asarray(visited, np.float32)
    L = len(s)
    if k == 0 or L == 0:
        return 0
    if not (L > k and 1 <= k <= SELECT_MAX) or np.isnan(s).any():
        return 1
    top = np.sort(s)[::-1][:k + 1]        # equal floats are neighbours in any descending order, +0.0 and -0.0 included
    return int((top[:-1] == top[1:]).any())


def tie_is_the_reason(visited, k):
    s = np.asarray(visited, np.float32)
    return len(s) > k >= 1 and k <= SELECT_MAX and not np.isnan(s).any() and expected_status(s, k) == 1


def span_sets(n):
    """the span sets the golden tests ask every query with, each where it fits an index of n rows"""
    sets = [[(0, n)], []]
    if n >= 2:
        sets.append([(0, 1), (n - 1, n)])
    sets += [[(b, e)] for b, e in ((63, 65), (64, 128), (511, 513)) if e <= n]
    sets.append([(r, r + 1) for r in range(0, n, 7)])
    if n >= 100:
        sets.append([(0, 64), (64, 100)])                                   # adjacent
    if n >= 12:
        sets.append([(0, 0), (2, 5), (5, 5), (7, 7), (9, 12), (n, n)])      # empty spans between non-empty ones
    out = [spans_of(s) for s in sets]
    assert all(spans_are_valid(s, n) for s in out)
    return out


def k_values(sets):
    """one call per k: {0, 1, 3, 10, L - 1, L, L + 5} for the length L of every span set"""
    ks = {0, 1, 3, 10}
    for s in sets:
        L = int((s[:, 1] - s[:, 0]).sum())
        ks |= {L - 1, L, L + 5}
    return sorted(k for k in ks if k >= 0)


@functools.lru_cache(maxsize=None)
def golden_scores(name):
    """per query of a golden fixture, the f32 score of every row as the reference stores it: from the golden file alone"""
    g = O.load_golden(name)
    return g["n"], [O.dec(rec["score_f64"], "<f8").astype(np.float32) for rec in g["queries"]]


@functools.lru_cache(maxsize=None)
def tie_scores(name):
    """the same for a tie fixture, whose golden file holds no per-row scores: the oracle's index and the oracle's scores"""
    g = O.load_golden(name)
    sim = O.SIMS[g["sim"]]
    base, queries = O.golden_inputs(g)
    codes, corr, cen = O.build_index(base, sim, g["lambda"], g["iters"], g["ib"])
    assert O.sha(codes) == g["codes_sha256"]
    cdp = O.centroid_dp(cen)
    out = []
    for q in queries:
        qq, qc = O.quantize_query(q, cen, sim, g["qb"], g["lambda"], g["iters"])
        out.append(O.score_all(codes, corr, g["dim"], qq, qc, g["qb"], sim, cdp, g["ib"])[2])
    return g["n"], out


def tie_span_sets(n):
    """everything, and halves"""
    h = n // 2
    return [spans_of(s) for s in ([(0, n)], [(0, h)], [(h, n)], [(0, h // 2), (h, h + h // 2)])]


TIE_KS = (1, 3, 10, 100)


def test_the_rule_on_small_cases():
    f = np.float32
    assert expected_status([], 3) == 0 and expected_status([1, 2], 0) == 0
    assert expected_status([3, 1, 2], 2) == 0 and expected_status([3, 1, 2], 3) == 1 and expected_status([3, 1, 2], 8) == 1
    assert expected_status([5, 4, 3, 3], 2) == 0          # the two equal scores are not both among the k + 1 largest
    assert expected_status([5, 4, 3, 3], 3) == 1 and expected_status([5, 5, 3, 2], 1) == 1 and expected_status([5, 5, 3, 2], 2) == 1
    assert expected_status([1, f(0.0), f(-0.0)], 1) == 0 and expected_status([1, f(0.0), f(-0.0)], 2) == 1
    assert expected_status([1, np.nan, 0.5], 1) == 1
    big = np.arange(SELECT_MAX + 10, dtype=np.float32)
    assert expected_status(big, SELECT_MAX) == 0 and expected_status(big, SELECT_MAX + 1) == 1
    assert tie_is_the_reason([5, 5, 3, 2], 1) and not tie_is_the_reason([1, np.nan, 0.5], 1) and not tie_is_the_reason([3, 1, 2], 3)


def test_expansion():
    np.testing.assert_array_equal(expand([(0, 0), (2, 5), (5, 5), (9, 11)]), [2, 3, 4, 9, 10])
    assert len(expand([])) == 0
    assert spans_are_valid([(0, 64), (64, 100)], 100) and not spans_are_valid([(63, 65), (64, 128)], 1000)
    assert not spans_are_valid([(5, 3)], 10) and not spans_are_valid([(0, 11)], 10) and not spans_are_valid([(4, 6), (0, 2)], 10)
    for n in (1, 2, 12, 100, 1000):
        for s in span_sets(n):
            rows = expand(s)
            assert (np.diff(rows) > 0).all() and (len(rows) == 0 or (rows[0] >= 0 and rows[-1] < n))


def test_the_golden_inputs_exercise_the_device_selection():
    """of the (query, span set, k) cases of the golden GPU test with L > k >= 1, at least half are answered by the device"""
    total = by_device = 0
    for name in SO.FIXTURES:
        n, scores = golden_scores(name)
        sets = span_sets(n)
        ks = k_values(sets)
        for s32 in scores:
            assert len(s32) == n
            for sp in sets:
                v = s32[expand(sp)]
                for k in ks:
                    if len(v) > k >= 1:
                        total += 1
                        by_device += expected_status(v, k) == 0
    assert total > 1000 and 2 * by_device >= total, "%d of %d cases have expected status 0" % (by_device, total)


@pytest.mark.parametrize("name", TIE_FIXTURES)
def test_every_tie_fixture_has_a_replay_because_of_ties(name):
    n, scores = tie_scores(name)
    hits = sum(tie_is_the_reason(s32[expand(sp)], k) for s32 in scores for sp in tie_span_sets(n) for k in TIE_KS)
    assert hits >= 1
