"""CPU: the compaction's host side without a device.  (1) The four entry points are declared, exported and bound.  (2)
bbq_filter_kept_rows - the old ord of every row a compaction keeps, ascending - against numpy.flatnonzero, at and around the 64-row
word and the 512-row chunk.  (3) The argument checks that come before anything touches the device."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from bbqlib import ROOT, bbq_amd as B, capi

NAMES = ("bbq_index_compact", "bbq_index_remove_rows", "bbq_vectors_compact", "bbq_filter_kept_rows")
LENGTHS = (1, 63, 64, 65, 511, 512, 513, 1000)


def _err():
    return capi.lib().bbq_last_error().decode("utf-8")


def _masks(n):
    rng = np.random.default_rng(1000 + n)
    alt = np.arange(n) % 2 == 0
    last = np.zeros(n, bool)
    last[-1] = True
    first = np.zeros(n, bool)
    first[0] = True
    return {"ones": np.ones(n, bool), "zeros": np.zeros(n, bool), "alternating": alt, "last": last, "first": first,
            "random_50": rng.random(n) < 0.5}


def test_the_four_names_are_declared_exported_and_bound():
    src = open(os.path.join(ROOT, "include", "bbq.h"), encoding="utf-8").read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(bbq_[a-z0-9_]+)\s*\(", src))
    lib = C.CDLL(capi.LIB_PATH)
    for name in NAMES:
        assert name in declared, "%s is not declared in include/bbq.h" % name
        assert hasattr(lib, name), "libbbq.so does not export %s" % name
        assert name in capi.SYMBOLS, "capi.py does not bind %s" % name
    assert lib.bbq_abi_version() == 3   # symbols only


@pytest.mark.parametrize("n", LENGTHS)
def test_kept_rows_is_flatnonzero(n):
    for name, mask in _masks(n).items():
        got = capi.kept_rows(mask)
        assert got.dtype == np.int32
        np.testing.assert_array_equal(got, np.flatnonzero(mask), err_msg="%s n=%d" % (name, n))
    assert B.kept_rows is capi.kept_rows


@pytest.mark.parametrize("n", LENGTHS)
def test_kept_rows_ignores_the_bits_at_and_beyond_n_rows(n):
    L = capi.lib()
    mask = _masks(n)["random_50"]
    words = capi.pack_mask(mask).copy()
    dirty = words.copy()
    if n & 63:
        dirty[-1] |= np.uint64(0xFFFFFFFFFFFFFFFF) << np.uint64(n & 63)
    dirty = np.concatenate([dirty, np.full(2, 0xFFFFFFFFFFFFFFFF, np.uint64)])   # whole words behind the last one are not read as rows
    out = np.full(n + 8, -7, np.int32)
    cnt = C.c_int64(-1)
    assert L.bbq_filter_kept_rows(dirty.ctypes.data, n, out.ctypes.data, n, C.byref(cnt)) == capi.OK
    want = np.flatnonzero(mask)
    assert cnt.value == len(want)
    np.testing.assert_array_equal(out[:len(want)], want)
    assert (out[len(want):] == -7).all()


@pytest.mark.parametrize("n", LENGTHS)
def test_kept_rows_cap_too_small_reports_the_count_and_writes_nothing(n):
    L = capi.lib()
    mask = np.ones(n, bool)
    words = capi.pack_mask(mask)
    out = np.full(n + 1, -7, np.int32)
    cnt = C.c_int64(-1)
    assert L.bbq_filter_kept_rows(words.ctypes.data, n, out.ctypes.data, n - 1, C.byref(cnt)) == capi.ERR_INVALID_ARG
    assert cnt.value == n and "room for %d" % (n - 1) in _err()
    assert (out == -7).all()
    # exactly enough room
    assert L.bbq_filter_kept_rows(words.ctypes.data, n, out.ctypes.data, n, C.byref(cnt)) == capi.OK
    np.testing.assert_array_equal(out[:n], np.arange(n))
    assert out[n] == -7


def test_kept_rows_of_no_rows_and_bad_arguments():
    L = capi.lib()
    cnt = C.c_int64(-1)
    out = np.zeros(4, np.int32)
    words = np.ones(1, np.uint64)
    assert L.bbq_filter_kept_rows(None, 0, None, 0, C.byref(cnt)) == capi.OK and cnt.value == 0
    assert len(capi.kept_rows(np.zeros(0, bool))) == 0
    assert L.bbq_filter_kept_rows(words.ctypes.data, 1, out.ctypes.data, 4, None) == capi.ERR_INVALID_ARG
    assert L.bbq_filter_kept_rows(None, 1, out.ctypes.data, 4, C.byref(cnt)) == capi.ERR_INVALID_ARG
    assert L.bbq_filter_kept_rows(words.ctypes.data, -1, out.ctypes.data, 4, C.byref(cnt)) == capi.ERR_INVALID_ARG
    assert L.bbq_filter_kept_rows(words.ctypes.data, 1, out.ctypes.data, -1, C.byref(cnt)) == capi.ERR_INVALID_ARG
    assert L.bbq_filter_kept_rows(words.ctypes.data, 1, None, 4, C.byref(cnt)) == capi.ERR_INVALID_ARG
    assert "bbq_filter_kept_rows" in _err()


def test_null_handles_are_invalid_arguments():
    L = capi.lib()
    rows = np.zeros(3, np.int32)
    assert L.bbq_index_compact(None, None) == capi.ERR_INVALID_ARG
    assert "null" in _err()
    assert L.bbq_index_remove_rows(None, rows.ctypes.data, 3) == capi.ERR_INVALID_ARG
    assert "bbq_index_remove_rows" in _err()
    assert L.bbq_index_remove_rows(None, None, 0) == capi.ERR_INVALID_ARG
    assert L.bbq_vectors_compact(None, None) == capi.ERR_INVALID_ARG
    assert "bbq_vectors_compact" in _err()


def test_device_entry_points_fail_without_a_device_as_the_others_do():
    """an index, a filter or a vectors handle only exists on a device: without one their creation already fails loudly, so no handle
    ever reaches the compaction (there is no CPU fallback to compact)"""
    if B.device_count() > 0:
        pytest.skip("a HIP device is present")
    with pytest.raises(B.BBQError) as e:
        B.Index(np.zeros((4, 1), np.uint8), np.zeros((4, 4)), 8, 0.0)
    assert e.value.code == capi.ERR_NO_DEVICE
    with pytest.raises(B.BBQError) as e:
        B.Vectors(np.zeros((4, 8), np.float32))
    assert e.value.code == capi.ERR_NO_DEVICE


def test_python_mirror_compacts_host_rows_without_a_device():
    if B.device_count() > 0:
        pytest.skip("a HIP device is present: tests/test_gpu_compact.py covers the device path")
    rng = np.random.default_rng(3)
    dim, n = 40, 200
    a = rng.standard_normal((n, dim)).astype(np.float32)
    fmt = B.BinaryQuantizationFormat({"queryBits": 4, "indexBits": 1, "quantizer": {"similarityFunction": "COSINE", "lambda": 0.1, "iters": 5}})
    tv = fmt.quantizeVectors(list(a))["quantizedVectors"]
    codes, corr = tv._codes.copy(), tv._corr.copy()
    mask = rng.random(n) < 0.5
    assert fmt.compactVectors(tv, mask) is tv and tv.size() == int(mask.sum())
    np.testing.assert_array_equal(tv._codes, codes[mask])
    np.testing.assert_array_equal(tv._corr.view(np.uint64), corr[mask].view(np.uint64))
    kept = np.flatnonzero(mask)
    assert fmt.removeVectors(tv, [3, 0, 3]) is tv and tv.size() == len(kept) - 2
    np.testing.assert_array_equal(tv.vectorValue(0), codes[kept[1]])
    np.testing.assert_array_equal(tv.vectorValue(2), codes[kept[4]])
    with pytest.raises(Exception, match="向量索引 %d 不存在" % tv.size()):
        fmt.removeVectors(tv, [tv.size()])
    assert tv.size() == len(kept) - 2
