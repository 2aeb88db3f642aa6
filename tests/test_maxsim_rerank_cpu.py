"""CPU: bbq_maxsim_reduce_true - the normative sum of the exact MaxSim rerank - against the model of tests/maxsim_rerank_model.py, byte
for byte; and the refusals of the two device calls that need no device: null handles, a similarity outside 0 .. 2."""
import itertools

import numpy as np
import pytest

import maxsim_rerank_model as MR
from bbqlib import capi

INF, NAN = np.inf, np.nan


def _same(rep):
    rep = np.asarray(rep, np.float64)
    got, want = capi.maxsim_reduce_true(rep), MR.reduce_true(rep)
    assert got.dtype == np.float64 and got.tobytes() == want.tobytes(), (rep.tolist(), got.tolist(), want.tolist())
    return got


def test_symbols_are_bound():
    names = {"bbq_maxsim_reduce_true", "bbq_rerank_maxsim_groups_batch", "bbq_search_maxsim_rerank_batch"}
    assert names <= set(capi.SYMBOLS)
    L = capi.lib()
    assert all(getattr(L, n) for n in names)
    assert hasattr(capi.Vectors, "rerank_maxsim_groups_batch") and hasattr(capi, "search_maxsim_rerank_batch")


def test_the_sum_is_ordered():
    """1e16 + 1.0 - 1e16 is 0.0 in this order and 1.0 in another: every permutation is a column, each summed in its own order"""
    perms = list(itertools.permutations([1e16, 1.0, -1e16]))
    got = _same(np.array(perms, np.float64).T)
    assert got[perms.index((1e16, 1.0, -1e16))] == 0.0 and got[perms.index((1e16, -1e16, 1.0))] == 1.0
    assert len(set(got.tolist())) > 1


def test_the_sum_starts_from_the_first_token():
    got = _same([[-0.0, 0.0, 5.0]])                           # n_vectors = 1: a single -0.0 stays -0.0
    assert MR.bits(got).tolist() == MR.bits([-0.0, 0.0, 5.0]).tolist()
    got = _same([[-0.0], [-0.0]])
    assert np.signbit(got[0])
    _same([[-0.0], [0.0]])


def test_nan_is_the_one_quiet_nan():
    odd = np.array([0xfff8000000000001, 0x7ff0000000000001], np.uint64).view(np.float64)    # NaNs of other payloads and sign
    for pos in range(3):                                      # a NaN in the first, a middle and the last token
        for nan in (NAN, odd[0], odd[1]):
            col = [1.5, -2.0, 3.25]
            col[pos] = nan
            got = _same(np.array([col, [1.0, 2.0, 3.0]], np.float64).T)
            assert MR.bits(got).tolist() == [MR.NAN_BITS, MR.bits([6.0])[0]]
    got = _same([[INF, -INF, INF, 1.0], [-INF, INF, INF, INF], [1.0, 1.0, 1.0, -INF]])
    assert MR.bits(got).tolist()[:2] == [MR.NAN_BITS] * 2 and got[2] == INF and MR.bits(got)[3] == MR.NAN_BITS
    assert MR.bits(_same([[NAN]])).tolist() == [MR.NAN_BITS]


def test_random_columns():
    rng = np.random.default_rng(77)
    rep = rng.standard_normal((33, 50)) * 10.0 ** rng.integers(-20, 20, (33, 50))
    rep[rng.integers(0, 33, 6), rng.integers(0, 50, 6)] = [NAN, INF, -INF, 0.0, -0.0, NAN]
    _same(rep)
    assert capi.maxsim_reduce_true(np.zeros((3, 0))).shape == (0,)


def test_reduce_arguments():
    L = capi.lib()
    out = np.zeros(2)
    assert L.bbq_maxsim_reduce_true(np.zeros(2).ctypes.data, 0, 2, out.ctypes.data) == capi.ERR_INVALID_ARG
    assert L.bbq_maxsim_reduce_true(np.zeros(2).ctypes.data, 1, -1, out.ctypes.data) == capi.ERR_INVALID_ARG
    assert L.bbq_maxsim_reduce_true(None, 1, 2, out.ctypes.data) == capi.ERR_INVALID_ARG
    assert L.bbq_maxsim_reduce_true(np.zeros(2).ctypes.data, 1, 2, None) == capi.ERR_INVALID_ARG


def test_the_model_on_a_small_case():
    c = np.array([[1.0, NAN, -0.0, 0.0, NAN, 7.0], [NAN, 2.0, -3.0, -INF, NAN, 7.0]])
    off = np.array([0, 2, 2, 4, 5, 6], np.int64)              # groups: rows {0, 1}, none, {2, 3}, {4}, {5}
    mask = np.array([1, 1, 1, 1, 1, 0], bool)
    assert MR.live_groups(off, mask).tolist() == [0, 2, 3]
    rep = MR.rep_true(c, off, mask, [0, 2, 3])
    assert MR.bits(rep[0]).tolist() == [MR.bits([1.0])[0], MR.bits([0.0])[0], MR.NAN_BITS]     # a NaN below a number; -0.0 below +0.0
    assert MR.bits(rep[1]).tolist() == [MR.bits([2.0])[0], MR.bits([-3.0])[0], MR.NAN_BITS]    # -Inf below a number
    assert MR.bits(MR.scores(c, off, mask, [2, 0, 2, 3])).tolist() == [MR.bits([-3.0])[0], MR.bits([3.0])[0], MR.bits([-3.0])[0], MR.NAN_BITS]
    assert MR.group_max(np.array([-INF, NAN])) == -INF


def test_refusals_that_need_no_device():
    L = capi.lib()
    one = np.zeros(1, np.int64)
    for sim in (-1, 3):
        assert L.bbq_rerank_maxsim_groups_batch(None, None, 0, None, None, sim, None, None, None) == capi.ERR_INVALID_ARG
        assert "不支持的相似性函数" in L.bbq_last_error().decode("utf-8")
        assert L.bbq_search_maxsim_rerank_batch(None, None, None, 0, None, None, None, None, 4, 1, 1, 1, 0, sim, None, None, None, None) == capi.ERR_INVALID_ARG
        assert "不支持的相似性函数" in L.bbq_last_error().decode("utf-8")
    assert L.bbq_rerank_maxsim_groups_batch(None, None, 1, one.ctypes.data, None, 1, one.ctypes.data, None, None) == capi.ERR_INVALID_ARG
    assert "null" in L.bbq_last_error().decode("utf-8")
    assert L.bbq_search_maxsim_rerank_batch(None, None, None, 0, None, None, None, None, 4, 1, 1, 1, 0, 1, None, None, None, None) == capi.ERR_INVALID_ARG
    assert "null handle" in L.bbq_last_error().decode("utf-8")
