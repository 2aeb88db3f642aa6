"""CPU: the host side of appending rows.  bbq_quantize_rows - quantizeVectors' per-row part against a GIVEN centroid - against the
oracle recipe, bit for bit: orc_normalize (COSINE), orc_scalar_quantize(row, centroid) and, for 1-bit rows, orc_pack_binary.  That
recipe reproduces every row orc_build_index / orc_build_index_unpacked makes with the centroid it returns (checked below as well),
and it is what every append test compares with.  No tolerances."""
import ctypes as C

import numpy as np
import pytest

import orclib as O
from append_recipe import oracle_rows
from bbqlib import bbq_amd as B, capi


def same_rows(got, want, msg):
    np.testing.assert_array_equal(got[0], want[0], err_msg=msg + ": codes")
    np.testing.assert_array_equal(got[1].view(np.uint64), want[1].view(np.uint64), err_msg=msg + ": corrections")


def vectors_for(seed, n, dim):
    v = O.mulberry32(seed, n * dim).reshape(n, dim).copy()
    v[1] = 0.0                      # a zero vector
    v[2] = 0.37                     # a constant vector
    return v


@pytest.mark.parametrize("ib", [1, 2, 4, 8])
@pytest.mark.parametrize("dim", [1, 64, 100, 768])
@pytest.mark.parametrize("sim", [0, 1, 2])
def test_quantize_rows_matches_the_oracle_recipe(sim, dim, ib):
    n = 40
    v = vectors_for(100 + dim, n, dim)
    cen = O.mulberry32(7 + dim, dim) * np.float32(0.25)   # any centroid: not the mean of these rows
    same_rows(B.quantize_rows(v, cen, sim, ib), oracle_rows(v, cen, sim, ib), "sim %d dim %d ib %d" % (sim, dim, ib))
    same_rows(B.quantize_rows(v, cen, sim, ib, lam=0.3, iters=2, n_threads=3), oracle_rows(v, cen, sim, ib, 0.3, 2), "lambda / iters / threads")


@pytest.mark.parametrize("ib", [1, 2, 4])
@pytest.mark.parametrize("dim", [100, 768])
@pytest.mark.parametrize("sim", [0, 1, 2])
def test_quantize_rows_reproduces_quantize_vectors_and_the_oracle_build(sim, dim, ib):
    v = vectors_for(5, 300, dim)
    codes, corr, cen = B.quantize_vectors(v, sim, ib)
    same_rows(B.quantize_rows(v, cen, sim, ib), (codes, corr), "the rows of bbq_quantize_vectors")
    ocodes, ocorr, ocen = O.build_index(v, sim, ib=ib)
    np.testing.assert_array_equal(cen.view(np.uint32), ocen.view(np.uint32))
    same_rows(oracle_rows(v, ocen, sim, ib), (ocodes, ocorr), "the recipe against the oracle's own build")
    # ... and a block quantized on its own equals the same rows quantized among others
    same_rows(B.quantize_rows(v[100:164], cen, sim, ib), (codes[100:164], corr[100:164]), "a block on its own")


@pytest.mark.parametrize("sim", [0, 1, 2])
@pytest.mark.parametrize("bad,code", [(np.nan, capi.ERR_NAN_INPUT), (np.inf, capi.ERR_INF_INPUT), (-np.inf, capi.ERR_INF_INPUT)])
def test_quantize_rows_reports_nan_and_infinity(sim, bad, code):
    dim = 64
    v = vectors_for(9, 200, dim)
    v[150, 3] = bad      # a later offender as well: the first in row-major order is reported
    v[137, 41] = bad
    cen = np.zeros(dim, np.float32)
    with pytest.raises(B.BBQError) as e:
        B.quantize_rows(v, cen, sim, 1, n_threads=4)
    # COSINE validates the NORMALISED rows (src/binaryQuantizationFormat.ts:174-211): a NaN or an Infinity anywhere in a row makes its
    # norm NaN / Infinity, so position 0 of that row is the first offender - NaN for a NaN row, and for an Infinity row x / Infinity = 0
    # everywhere but Infinity / Infinity = NaN at the offender itself
    if sim == 1:
        want = (capi.ERR_NAN_INPUT, 137, 0 if bad != bad else 41)
    else:
        want = (code, 137, 41)
    assert (e.value.code, e.value.bad_row, e.value.bad_col) == want
    # the same position and code the whole-set quantizer reports
    br, bc = C.c_int64(-1), C.c_int32(-1)
    out = (np.zeros((200, 8), np.uint8), np.zeros((200, 4)), np.zeros(dim, np.float32))
    rc = capi.lib().bbq_quantize_vectors(v.ctypes.data, 200, dim, sim, 1, 0.1, 5, 0, out[0].ctypes.data, out[1].ctypes.data, out[2].ctypes.data,
                                         C.byref(br), C.byref(bc))
    assert (rc, br.value, bc.value) == want


def test_new_symbols_are_exported_bound_and_check_arguments_without_a_device():
    new = ["bbq_index_append_rows", "bbq_index_append", "bbq_index_reserve", "bbq_index_capacity", "bbq_vectors_append", "bbq_quantize_rows"]
    L = capi.lib()
    raw = C.CDLL(capi.LIB_PATH)
    for name in new:
        assert name in capi.SYMBOLS and hasattr(raw, name), name
    assert L.bbq_abi_version() == 3
    z = np.zeros(64, np.uint8)
    f = np.zeros(64, np.float32)
    d = np.zeros(4)
    assert L.bbq_index_append_rows(None, z.ctypes.data, d.ctypes.data, 1) == capi.ERR_INVALID_ARG
    assert L.bbq_index_append(None, f.ctypes.data, 1, f.ctypes.data, 1, 0.1, 5, None, None, None, None) == capi.ERR_INVALID_ARG
    assert L.bbq_index_reserve(None, 10) == capi.ERR_INVALID_ARG
    assert L.bbq_vectors_append(None, f.ctypes.data, 1) == capi.ERR_INVALID_ARG
    assert L.bbq_index_capacity(None) == 0
    assert L.bbq_quantize_rows(f.ctypes.data, -1, 64, f.ctypes.data, 1, 1, 0.1, 5, 0, z.ctypes.data, d.ctypes.data, None, None) == capi.ERR_INVALID_ARG
    assert L.bbq_quantize_rows(f.ctypes.data, 0, 64, f.ctypes.data, 1, 1, 0.1, 5, 0, z.ctypes.data, d.ctypes.data, None, None) == capi.OK
    assert L.bbq_quantize_rows(f.ctypes.data, 1, 64, None, 1, 1, 0.1, 5, 0, z.ctypes.data, d.ctypes.data, None, None) == capi.ERR_INVALID_ARG
    assert L.bbq_quantize_rows(f.ctypes.data, 1, 64, f.ctypes.data, 3, 1, 0.1, 5, 0, z.ctypes.data, d.ctypes.data, None, None) == capi.ERR_INVALID_ARG
    # a negative n is refused before anything is looked at: the handle may be anything, no device is opened
    class _FakeIndex(C.Structure):
        _fields_ = [("bytes", C.c_uint8 * 8192)]
    fake = _FakeIndex()
    assert L.bbq_index_append_rows(C.byref(fake), z.ctypes.data, d.ctypes.data, -1) == capi.ERR_INVALID_ARG
    assert L.bbq_index_append(C.byref(fake), f.ctypes.data, -1, f.ctypes.data, 1, 0.1, 5, None, None, None, None) == capi.ERR_INVALID_ARG
    assert L.bbq_vectors_append(C.byref(fake), f.ctypes.data, -1) == capi.ERR_INVALID_ARG


@pytest.mark.parametrize("ib", [1, 4])
@pytest.mark.parametrize("simname", ["EUCLIDEAN", "COSINE", "MAXIMUM_INNER_PRODUCT"])
def test_api_append_vectors_without_a_device(simname, ib, monkeypatch):
    """appendVectors on the host path (what api.py takes when the library finds no device; a machine that has one is made to look
    like one that has not): size() and the row accessors over the new ords are the oracle recipe's rows"""
    monkeypatch.setattr(capi, "device_count", lambda: 0)
    sim, dim = O.SIMS[simname], 100
    a, b = vectors_for(21, 130, dim), vectors_for(22, 70, dim)
    fmt = B.BinaryQuantizationFormat({"indexBits": ib, "quantizer": {"similarityFunction": simname, "lambda": 0.1, "iters": 5}})
    tv = fmt.quantizeVectors(list(a))["quantizedVectors"]
    first = tv.vectorValue(0).copy()
    assert fmt.appendVectors(tv, list(b)) is tv
    assert tv.size() == 200
    ocodes, ocorr, ocen = O.build_index(a, sim, ib=ib)
    bcodes, bcorr = oracle_rows(b, ocen, sim, ib)
    want_codes, want_corr = np.concatenate([ocodes, bcodes]), np.concatenate([ocorr, bcorr])
    for ord_ in (0, 129, 130, 131, 199):
        np.testing.assert_array_equal(tv.vectorValue(ord_), want_codes[ord_])
        t = tv.getCorrectiveTerms(ord_)
        got = np.array([t["lowerInterval"], t["upperInterval"], t["additionalCorrection"], t["quantizedComponentSum"]])
        np.testing.assert_array_equal(got.view(np.uint64), want_corr[ord_].view(np.uint64))
    np.testing.assert_array_equal(first, tv.vectorValue(0))
    with pytest.raises(Exception, match="不存在"):
        tv.vectorValue(200)
    # argument checks: the dimension like quantizeVectors, NaN with its position, nothing changed afterwards
    with pytest.raises(Exception, match="维度"):
        fmt.appendVectors(tv, [np.zeros(dim + 1, np.float32)])
    bad = b[:5].copy()
    bad[3, 7] = np.nan
    with pytest.raises(Exception, match="向量 3 位置 %d 包含NaN值" % (0 if sim == 1 else 7)):
        fmt.appendVectors(tv, list(bad))
    assert tv.size() == 200
    assert fmt.appendVectors(tv, []) is tv and tv.size() == 200
