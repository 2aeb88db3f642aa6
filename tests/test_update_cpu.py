"""CPU: the host-only part of the in-place update - bbq_update_winners against a dict restatement - the argument errors the device
entry points see without a device, and updateVectors on api.py's host path against the oracle recipe."""
import ctypes as C

import numpy as np
import pytest

import orclib as O
from bbqlib import bbq_amd as B, capi
from append_recipe import oracle_rows


def winners_by_dict(ords):
    """positions of the last occurrence of every distinct ord, ascending by ord"""
    last = {}
    for i, o in enumerate(ords):
        last[int(o)] = i
    return [last[o] for o in sorted(last)]


@pytest.mark.parametrize("ords,n_rows", [
    ([], 0), ([], 10), ([4], 5), (list(range(50)), 50), ([7] * 33, 8), ([5, 3, 5, 0, 3, 9], 10),
    (list(np.random.default_rng(9000).integers(0, 300, 10000)), 300), (list(range(299, -1, -1)), 300)])
def test_update_winners_equals_the_dict(ords, n_rows):
    got = capi.update_winners(ords, n_rows)
    assert got.dtype == np.int64
    assert list(got) == winners_by_dict(ords)
    if len(ords):
        assert list(np.asarray(ords)[got]) == sorted(set(int(o) for o in ords))


def test_update_winners_arguments():
    L = capi.lib()
    ords = np.array([5, 3, 5, 0, 3, 9], np.int32)
    out = np.full(8, -7, np.int64)
    n = C.c_int64(-1)
    # cap too small: the count is right, nothing is written
    assert L.bbq_update_winners(ords.ctypes.data, 6, 10, out.ctypes.data, 3, C.byref(n)) == capi.ERR_INVALID_ARG
    assert n.value == 4 and (out == -7).all()
    assert L.bbq_update_winners(ords.ctypes.data, 6, 10, None, 0, C.byref(n)) == capi.ERR_INVALID_ARG and n.value == 4
    assert L.bbq_update_winners(ords.ctypes.data, 6, 10, out.ctypes.data, 4, C.byref(n)) == capi.OK
    assert n.value == 4 and list(out[:4]) == [3, 4, 2, 5] and (out[4:] == -7).all()
    # an ord outside [0, n_rows)
    out[:] = -7
    for bad, n_rows in ((-1, 10), (10, 10), (0, 0)):
        o = np.array([1 % max(n_rows, 1), bad], np.int32)
        assert L.bbq_update_winners(o.ctypes.data, 2, n_rows, out.ctypes.data, 8, C.byref(n)) == capi.ERR_INVALID_ARG
        assert "向量索引 %d 不存在" % bad in L.bbq_last_error().decode("utf-8") and (out == -7).all()
    with pytest.raises(B.BBQError) as e:
        capi.update_winners([3, 2**40], 10)
    assert e.value.code == capi.ERR_INVALID_ARG
    # nothing to do, and null / negative arguments
    assert L.bbq_update_winners(None, 0, 10, None, 0, C.byref(n)) == capi.OK and n.value == 0
    assert L.bbq_update_winners(None, 2, 10, out.ctypes.data, 8, C.byref(n)) == capi.ERR_INVALID_ARG
    assert L.bbq_update_winners(ords.ctypes.data, 6, 10, out.ctypes.data, 8, None) == capi.ERR_INVALID_ARG
    assert L.bbq_update_winners(ords.ctypes.data, -1, 10, out.ctypes.data, 8, C.byref(n)) == capi.ERR_INVALID_ARG
    assert L.bbq_update_winners(ords.ctypes.data, 6, -1, out.ctypes.data, 8, C.byref(n)) == capi.ERR_INVALID_ARG
    assert L.bbq_update_winners(ords.ctypes.data, 6, 10, out.ctypes.data, -1, C.byref(n)) == capi.ERR_INVALID_ARG


def test_device_entry_points_without_a_device():
    """no index or vectors handle can exist without a device (creation is BBQ_ERR_NO_DEVICE: there is no CPU fallback), and the update
    entry points refuse what they can see without one"""
    L = capi.lib()
    if B.device_count() == 0:
        with pytest.raises(B.BBQError) as e:
            B.Index(np.zeros((4, 1), np.uint8), np.zeros((4, 4)), 8, 0.0)
        assert e.value.code == capi.ERR_NO_DEVICE
        with pytest.raises(B.BBQError) as e:
            B.Vectors(np.zeros((4, 8), np.float32))
        assert e.value.code == capi.ERR_NO_DEVICE
    o = np.zeros(1, np.int32)
    z, d, f = np.zeros((1, 8), np.uint8), np.zeros((1, 4)), np.zeros(64, np.float32)
    assert L.bbq_index_update_rows(None, o.ctypes.data, z.ctypes.data, d.ctypes.data, 1) == capi.ERR_INVALID_ARG
    assert L.bbq_index_update(None, o.ctypes.data, f.ctypes.data, 1, f.ctypes.data, 1, 0.1, 5, None, None, None, None) == capi.ERR_INVALID_ARG
    assert L.bbq_vectors_update(None, o.ctypes.data, f.ctypes.data, 1) == capi.ERR_INVALID_ARG
    # a negative n is refused before a device is opened

    class _FakeIndex(C.Structure):
        _fields_ = [("bytes", C.c_uint8 * 8192)]
    fake = _FakeIndex()
    assert L.bbq_index_update_rows(C.byref(fake), o.ctypes.data, z.ctypes.data, d.ctypes.data, -1) == capi.ERR_INVALID_ARG
    assert L.bbq_index_update(C.byref(fake), o.ctypes.data, f.ctypes.data, -1, f.ctypes.data, 1, 0.1, 5, None, None, None, None) == capi.ERR_INVALID_ARG
    assert L.bbq_vectors_update(C.byref(fake), o.ctypes.data, f.ctypes.data, -1) == capi.ERR_INVALID_ARG


@pytest.mark.parametrize("ib", [1, 4])
@pytest.mark.parametrize("simname", ["EUCLIDEAN", "COSINE", "MAXIMUM_INNER_PRODUCT"])
def test_api_update_vectors_without_a_device(simname, ib, monkeypatch):
    """updateVectors on the host path (what api.py takes when the library finds no device; a machine that has one is made to look
    like one that has not): the updated ords hold the oracle recipe's rows, the last of equal ords wins, nothing else moves"""
    monkeypatch.setattr(capi, "device_count", lambda: 0)
    sim, dim, n = O.SIMS[simname], 100, 130
    a = O.mulberry32(31, n * dim).reshape(n, dim)
    ords = [129, 5, 64, 5, 0, 5]
    b = O.mulberry32(32, len(ords) * dim).reshape(len(ords), dim)
    fmt = B.BinaryQuantizationFormat({"indexBits": ib, "quantizer": {"similarityFunction": simname, "lambda": 0.1, "iters": 5}})
    tv = fmt.quantizeVectors(list(a))["quantizedVectors"]
    handed_out = tv.vectorValue(5)
    kept = handed_out.copy()
    assert fmt.updateVectors(tv, ords, list(b)) is tv and tv.size() == n
    want_codes, want_corr, ocen = O.build_index(a, sim, ib=ib)
    bcodes, bcorr = oracle_rows(b, ocen, sim, ib)
    for i, o in enumerate(ords):
        want_codes[o], want_corr[o] = bcodes[i], bcorr[i]
    for ord_ in range(n):
        np.testing.assert_array_equal(tv.vectorValue(ord_), want_codes[ord_])
        t = tv.getCorrectiveTerms(ord_)
        got = np.array([t["lowerInterval"], t["upperInterval"], t["additionalCorrection"], t["quantizedComponentSum"]])
        np.testing.assert_array_equal(got.view(np.uint64), want_corr[ord_].view(np.uint64))
    np.testing.assert_array_equal(handed_out, kept)   # a row handed out earlier stays valid
    # argument checks as appendVectors': dimension, NaN with its position inside the block, an ord outside the set; nothing changed
    with pytest.raises(Exception, match="维度"):
        fmt.updateVectors(tv, [1], [np.zeros(dim + 1, np.float32)])
    bad = b[:5].copy()
    bad[3, 7] = np.nan
    with pytest.raises(Exception, match="向量 3 位置 %d 包含NaN值" % (0 if sim == 1 else 7)):
        fmt.updateVectors(tv, ords[:5], list(bad))
    for o in (-1, n):
        with pytest.raises(Exception, match="向量索引 %d 不存在" % o):
            fmt.updateVectors(tv, [3, o], list(b[:2]))
    with pytest.raises(Exception, match="不匹配"):
        fmt.updateVectors(tv, [3], list(b[:2]))
    with pytest.raises(Exception, match="目标向量集合不能为空"):
        fmt.updateVectors(None, [3], list(b[:1]))
    np.testing.assert_array_equal(tv.vectorValue(3), want_codes[3])
    assert fmt.updateVectors(tv, [], []) is tv and tv.size() == n
