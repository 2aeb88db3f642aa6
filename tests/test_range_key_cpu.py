"""CPU: bbq_range_key (host-only C ABI) - the key a range search's sweeps compare against.

The sweeps test key(score) > K, a range search asks score >= t: K is the key of the largest float strictly below t, with +0 and -0
taken as one threshold.  Held here, for every pair of an edge-case table, to the IEEE comparison itself, together with the numpy
restatement of a range answer that the GPU tests use as their expectation."""
import itertools

import numpy as np
import pytest

from bbqlib import bbq_amd as B, capi

F = np.float32
ONE = F(1.0)
POS = [F(0.0), np.nextafter(F(0.0), F(1.0)),                      # +0, the smallest subnormal
       np.finfo(np.float32).tiny,                                # the smallest normal
       np.nextafter(ONE, F(0.0)), ONE, np.nextafter(ONE, F(2.0)),  # 1 and its two neighbours
       np.finfo(np.float32).max, F(np.inf)]
TABLE = [v for p in POS for v in (p, -p)]


def range_answer(s32, t):
    """the rows of a range answer over these f32 scores: no NaN score, score >= t as floats compare; ascending"""
    s32 = np.asarray(s32, np.float32)
    with np.errstate(invalid="ignore"):
        return np.flatnonzero(~np.isnan(s32) & (s32 >= F(t)))


def test_table_holds_what_it_says():
    assert len(TABLE) == 16 and len({v.tobytes() for v in TABLE}) == 16
    assert TABLE[2] == F(1.401298464324817e-45) and TABLE[4] == F(1.1754943508222875e-38)
    assert np.signbit(TABLE[1]) and TABLE[1] == 0.0


@pytest.mark.parametrize("s,t", list(itertools.product(TABLE, TABLE)))
def test_key_rule(s, t):
    assert (B.key_of_score(s) > B.range_key(t)) == bool(s >= t), "score %r threshold %r" % (s, t)


def test_both_zeros_are_one_threshold():
    assert B.range_key(0.0) == B.range_key(-0.0) == B.key_of_score(-0.0) - 1


def test_key_is_the_float_below():
    for t in TABLE:
        if t == 0.0:
            continue
        if t == F(-np.inf):
            continue
        with np.errstate(over="ignore"):      # the float below -max is -inf
            below = np.nextafter(t, F(-np.inf))
        assert B.range_key(t) == B.key_of_score(below), repr(t)
    # -inf: below the key of every score that is no NaN
    assert B.range_key(-np.inf) < B.key_of_score(-np.inf)


def test_nan_threshold_is_refused():
    for nan in (np.nan, -np.nan, F(np.nan)):
        with pytest.raises(B.BBQError) as e:
            B.range_key(nan)
        assert e.value.code == capi.ERR_INVALID_ARG
    assert capi.lib().bbq_range_key(1.0, None) == capi.ERR_INVALID_ARG


def test_numpy_restatement():
    s = np.array([0.5, np.nan, -0.0, 0.0, np.inf, -np.inf, 0.25, -np.nan], np.float32)
    np.testing.assert_array_equal(range_answer(s, -np.inf), [0, 2, 3, 4, 5, 6])
    np.testing.assert_array_equal(range_answer(s, np.inf), [4])
    np.testing.assert_array_equal(range_answer(s, 0.0), range_answer(s, -0.0))
    np.testing.assert_array_equal(range_answer(s, 0.0), [0, 2, 3, 4, 6])
    np.testing.assert_array_equal(range_answer(s, 0.25), [0, 4, 6])
    np.testing.assert_array_equal(range_answer(s, np.nextafter(F(0.5), F(1.0))), [4])
    # ... and it is the key rule, row by row
    for t in TABLE:
        K = B.range_key(t)
        want = [i for i, v in enumerate(s) if not np.isnan(v) and B.key_of_score(v) > K]
        np.testing.assert_array_equal(range_answer(s, t), want)
