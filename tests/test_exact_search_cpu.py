"""CPU: the host-only part of the exact search.  bbq_true_topk - the normative statement of the ranking - against the model of
tests/exact_model.py (the oracle's computeSimilarity and its stable descending sort) for all three similarities, byte for byte; a
hand-made score row that pins NaN last, ties by row and the one NaN written; the key restated in numpy; the argument errors; and what
the device entry points answer without a device."""
import ctypes as C
import functools

import numpy as np
import pytest

import exact_model as EM
from bbqlib import bbq_amd as B, capi

N, DIM = 300, 24


@functools.lru_cache(maxsize=None)
def _base():
    rng = np.random.default_rng(4100)
    base = rng.standard_normal((N, DIM)).astype(np.float32)
    base[40:47] = base[7]          # a block of duplicated rows
    base[200] = base[7]            # and one far behind it
    base[13] = 0.0                 # COSINE: 0.0
    base[150] = 0.0
    queries = rng.standard_normal((3, DIM)).astype(np.float32)
    queries[2] = base[7]           # the duplicates lead this query's ranking
    base.setflags(write=False)
    queries.setflags(write=False)
    return base, queries


@functools.lru_cache(maxsize=None)
def _scores(sim):
    base, queries = _base()
    return EM.scores(queries, base, sim)


def _masks():
    rng = np.random.default_rng(4101)
    wave = np.ones(N, bool)
    wave[64:128] = False           # a whole accept word
    single = np.zeros(N, bool)
    single[131] = True
    return {"none": None, "half": rng.random(N) < 0.5, "wave_out": wave, "empty": np.zeros(N, bool), "single": single}


def _same(got, want, msg):
    assert got[0].dtype == np.int32 and got[1].dtype == np.float64
    assert got[0].tolist() == want[0].tolist(), msg + ": rows"
    assert got[1].view(np.uint64).tolist() == want[1].tolist(), msg + ": score bits"


@pytest.mark.parametrize("sim", [0, 1, 2])
def test_true_topk_equals_the_model(sim):
    c = _scores(sim)
    for name, mask in _masks().items():
        accepted = N if mask is None else int(mask.sum())
        for q in range(c.shape[0]):
            for k in (0, 1, 5, 64, accepted, N, N + 9):
                _same(capi.true_topk(c[q], k, mask), EM.topk(c[q], k, mask), "sim %d, mask %s, query %d, k %d" % (sim, name, q, k))


@pytest.mark.parametrize("sim", [0, 1, 2])
def test_true_topk_on_identical_rows(sim):
    base, queries = _base()
    same = np.repeat(base[5:6], 130, axis=0)
    c = EM.scores(queries[:1], same, sim)
    assert len(set(c[0].view(np.uint64).tolist())) == 1
    for k in (1, 64, 130, 200):
        got = capi.true_topk(c[0], k)
        _same(got, EM.topk(c[0], k), "k %d" % k)
        assert got[0].tolist() == list(range(min(k, 130)))


def test_zero_rows_score_zero_under_cosine():
    c = _scores(1)
    assert (c[:, [13, 150]].view(np.uint64) == 0).all()


def test_nan_last_ties_by_row_and_one_nan():
    inf = np.inf
    odd_nan = np.array([0xfff8000000000123], np.uint64).view(np.float64)[0]   # a NaN with a sign and a payload
    s = np.array([1.0, np.nan, 3.0, -inf, 3.0, inf, odd_nan, 1.0, -2.0, inf, 0.0, -inf], np.float64)
    rows, out = capi.true_topk(s, 100)
    assert rows.tolist() == [5, 9, 2, 4, 0, 7, 10, 8, 3, 11, 1, 6]
    bits = out.view(np.uint64)
    assert bits[-2:].tolist() == [int(EM.NAN_BITS)] * 2
    assert bits[:-2].tolist() == s[rows[:-2]].view(np.uint64).tolist()
    _same((rows, out), EM.by_key(s, 100), "the hand-made row")
    for k in range(0, 13):
        _same(capi.true_topk(s, k), EM.by_key(s, k), "k %d" % k)
    mask = np.array([1, 1, 0, 1, 1, 0, 1, 0, 1, 1, 1, 0], bool)
    got = capi.true_topk(s, 5, mask)
    assert got[0].tolist() == [9, 4, 0, 10, 8]
    _same(got, EM.by_key(s, 5, mask), "masked")
    # NaNs alone: by ascending row
    assert capi.true_topk(np.array([np.nan, odd_nan, np.nan]), 2)[0].tolist() == [0, 1]


def test_the_key_is_true_key():
    """the order bbq_true_topk gives is a plain sorted() over (-key, row) with the key recomputed from the header's formula, on scores
    of every class: both zeros, subnormals, both infinities, NaNs, equal values"""
    rng = np.random.default_rng(4102)
    tiny = np.array([5e-324, -5e-324, 2.2e-308, -2.2e-308])
    s = np.concatenate([rng.standard_normal(200), [0.0, -0.0, np.inf, -np.inf, np.nan, 1.5, 1.5, -1.5, -1.5], tiny, rng.standard_normal(50) * 1e300])
    key = EM.true_key(s)
    assert int(key[np.flatnonzero(np.isnan(s))[0]]) == 1 and int(EM.true_key(np.array([-np.inf]))[0]) == 0x000fffffffffffff
    assert int(EM.true_key(np.array([0.0]))[0]) == 1 << 63 and int(EM.true_key(np.array([-0.0]))[0]) == (1 << 63) - 1
    want = [r for _, r in sorted((-int(key[r]), r) for r in range(s.shape[0]))]
    assert capi.true_topk(s, s.shape[0])[0].tolist() == want
    finite = np.flatnonzero(~np.isnan(s))
    order = [r for r in want if r in set(finite.tolist())]
    assert (np.diff(s[order]) <= 0).all(), "descending by value"


def test_true_topk_arguments():
    L = capi.lib()
    s = np.array([1.0, 2.0, 3.0])
    idx, out, n = np.full(4, -7, np.int32), np.full(4, -7.0), C.c_int64(-1)
    assert L.bbq_true_topk(s.ctypes.data, 3, None, -1, idx.ctypes.data, out.ctypes.data, C.byref(n)) == capi.ERR_NEGATIVE_K
    assert "k必须是非负数" in L.bbq_last_error().decode("utf-8") and n.value == 0
    assert L.bbq_true_topk(s.ctypes.data, -1, None, 2, idx.ctypes.data, out.ctypes.data, C.byref(n)) == capi.ERR_INVALID_ARG
    assert L.bbq_true_topk(None, 3, None, 2, idx.ctypes.data, out.ctypes.data, C.byref(n)) == capi.ERR_INVALID_ARG
    assert L.bbq_true_topk(s.ctypes.data, 3, None, 2, None, out.ctypes.data, C.byref(n)) == capi.ERR_INVALID_ARG
    assert L.bbq_true_topk(s.ctypes.data, 3, None, 2, idx.ctypes.data, None, C.byref(n)) == capi.ERR_INVALID_ARG
    assert L.bbq_true_topk(s.ctypes.data, 3, None, 2, idx.ctypes.data, out.ctypes.data, None) == capi.ERR_INVALID_ARG
    assert (idx == -7).all() and (out == -7.0).all()
    # nothing to do needs no arrays
    assert L.bbq_true_topk(None, 0, None, 5, None, None, C.byref(n)) == capi.OK and n.value == 0
    assert L.bbq_true_topk(s.ctypes.data, 3, None, 0, None, None, C.byref(n)) == capi.OK and n.value == 0
    none = np.zeros(1, np.uint64)
    assert L.bbq_true_topk(s.ctypes.data, 3, none.ctypes.data, 2, None, None, C.byref(n)) == capi.OK and n.value == 0
    assert L.bbq_true_topk(s.ctypes.data, 3, None, 2, idx.ctypes.data, out.ctypes.data, C.byref(n)) == capi.OK
    assert n.value == 2 and idx.tolist() == [2, 1, -7, -7] and out.tolist() == [3.0, 2.0, -7.0, -7.0]
    with pytest.raises(B.BBQError) as e:
        capi.true_topk(s, 2, np.ones(4, bool))
    assert e.value.code == capi.ERR_INVALID_ARG


def test_device_entry_points_without_a_device():
    """no vectors handle can exist without a device (creation is BBQ_ERR_NO_DEVICE: there is no CPU fallback), and the exact search's
    entry points refuse what they can see without one"""
    L = capi.lib()
    if B.device_count() == 0:
        with pytest.raises(B.BBQError) as e:
            B.Vectors(np.zeros((4, 8), np.float32))
        assert e.value.code == capi.ERR_NO_DEVICE
    q, idx, out, n = np.zeros(8, np.float32), np.zeros(4, np.int32), np.zeros(4), np.zeros(1, np.int64)
    call = lambda v, sim, k: L.bbq_vectors_search_batch(v, None, 1, q.ctypes.data, sim, k, idx.ctypes.data, out.ctypes.data, n.ctypes.data)
    assert call(None, 1, 4) == capi.ERR_INVALID_ARG
    assert call(None, 3, 4) == capi.ERR_INVALID_ARG and "不支持的相似性函数: 3" in L.bbq_last_error().decode("utf-8")
    assert call(None, -1, 4) == capi.ERR_INVALID_ARG
    assert L.bbq_vectors_set_option(None, b"exact_slab_rows", 256) == capi.ERR_INVALID_ARG
