"""GPU: bbq_quantize_queries_device (bbq_query_kernels.hip, one wave per query) returns bbq_quantize_queries' bytes - the host quantizer's,
and for the first and last query of every batch the oracle's - on the hostile batches and parameters of tests/quant_hostile.py (what
they reach is asserted on the CPU in tests/test_quantizer_hostile_cpu.py); its errors are the host's; option device_queries changes no
byte of bbq_search_raw_batch's answer.  qquant byte for byte, qcorr through canon64 (JS has one NaN); no tolerances."""
import ctypes as C

import numpy as np
import pytest

import orclib as O
import quant_hostile as Q
from bbqlib import bbq_amd as B, capi
from quant_hostile import canon64

pytestmark = pytest.mark.gpu

DIMS = (1, 3, 13, 64, 65, 131, 768)   # below a round of 64, dim % 4 != 0, one exact round, one element into the second, the workload's width
N = 257


def _index(dim):
    """any index of that dimension: the call reads the handle's dimension and device only"""
    return B.Index(np.zeros((1, (dim + 7) // 8), np.uint8), np.zeros((1, 4)), dim, 0.0)


def _call(ix, q, cen, sim, qb, lam, iters):
    """(code, bad_query, message, qquant, qcorr) of the device call on `ix`, of the host call without one"""
    q, cen = np.ascontiguousarray(q, np.float32), np.ascontiguousarray(cen, np.float32)
    n, dim = q.shape
    qq, qc, bad = np.zeros((n, dim), np.uint8), np.zeros((n, 4)), C.c_int32(-9)
    L = capi.lib()
    if ix is None:
        rc = L.bbq_quantize_queries(q.ctypes.data, n, dim, cen.ctypes.data, sim, qb, lam, iters, 4, qq.ctypes.data, qc.ctypes.data, C.byref(bad))
    else:
        rc = L.bbq_quantize_queries_device(ix._h, n, q.ctypes.data, cen.ctypes.data, sim, qb, lam, iters, qq.ctypes.data, qc.ctypes.data, C.byref(bad))
    return rc, bad.value, L.bbq_last_error().decode("utf-8") if rc else "", qq, qc


def _check(ix, q, cen, sim, qb, lam, iters, msg, oracle_rows=()):
    want, got = _call(None, q, cen, sim, qb, lam, iters), _call(ix, q, cen, sim, qb, lam, iters)
    assert got[:3] == want[:3], msg
    if want[0] != capi.OK:
        return want
    np.testing.assert_array_equal(got[3], want[3], err_msg=msg + " qquant")
    np.testing.assert_array_equal(canon64(got[4]), canon64(want[4]), err_msg=msg + " qcorr")
    for r in oracle_rows:
        oq, oc = O.quantize_query(q[r], cen, sim, qb, lam, iters)
        np.testing.assert_array_equal(got[3][r], oq, err_msg="%s oracle qquant, query %d" % (msg, r))
        np.testing.assert_array_equal(canon64(got[4][r]), canon64(oc), err_msg="%s oracle qcorr, query %d" % (msg, r))
    return want


@pytest.mark.parametrize("qb,lam,iters", Q.GRID)
@pytest.mark.parametrize("sim", [0, 1, 2])
def test_device_queries_equal_the_host(sim, qb, lam, iters):
    for dim in DIMS:
        ix, cen = _index(dim), Q.benign(1, dim, 2)[0]
        try:
            for name in ("mixed", "extreme", "overflow", "identical", "benign"):
                q = Q.benign(N, dim) if name == "benign" else Q.batch(name, N, dim)
                want = _check(ix, q, cen, sim, qb, lam, iters, "%s dim=%d" % (name, dim), oracle_rows=(0, N - 1))
                assert want[0] == capi.OK, "a finite batch"
        finally:
            ix.close()


def test_sub_batch_boundary():
    q = np.resize(Q.batch("mixed", N, 13), (4099, 13))
    ix = _index(13)
    try:
        assert _check(ix, q, Q.benign(1, 13, 2)[0], 1, 4, 0.1, 5, "n=4099", oracle_rows=(4095, 4096, 4098))[0] == capi.OK
    finally:
        ix.close()


@pytest.mark.parametrize("sim", [0, 1, 2])
def test_errors_are_the_host_call_s(sim):
    q = Q.benign(8, 13).copy()
    ix, cen = _index(13), Q.benign(1, 13, 2)[0]
    try:
        q[0] = 0.0                                           # COSINE: the normalisation leaves zeros, nothing bad
        assert _check(ix, q, cen, sim, 4, 0.1, 5, "a zero query", oracle_rows=(0,))[0] == capi.OK
        q[2, 4], q[5, 7] = np.inf, np.nan
        rc, bad, text = _check(ix, q, cen, sim, 4, 0.1, 5, "Infinity in query 2, NaN in query 5")[:3]
        # (COSINE: the second normalisation of query 2 spreads the NaN of Infinity / Infinity to position 0)
        assert (rc, bad) == ((capi.ERR_NAN_INPUT, 2) if sim == 1 else (capi.ERR_INF_INPUT, 2)) and ("位置 0 " if sim == 1 else "位置 4 ") in text
    finally:
        ix.close()


def test_option_changes_no_byte_of_a_raw_batch():
    rng = np.random.default_rng(9100)
    base, queries = rng.standard_normal((600, 64)).astype(np.float32), rng.standard_normal((70, 64)).astype(np.float32)
    codes, corr, cen = B.quantize_vectors(base, 1)
    ix = B.Index(codes, corr, 64, B.centroid_dp(cen))
    try:
        for nq in (3, 70):
            ix.set_option("device_queries", 0)
            want = ix.search_raw_batch(queries[:nq], cen, 1, 4, 10, want_quantized=True)
            ix.set_option("device_queries", 1)
            got = ix.search_raw_batch(queries[:nq], cen, 1, 4, 10, want_quantized=True)
            assert (want[2] == 10).all()
            for a, b in zip(got, want):
                assert a.dtype == b.dtype and a.tobytes() == b.tobytes(), "nq=%d" % nq
        with pytest.raises(B.BBQError) as e:
            ix.set_option("device_queries", 2)
        assert e.value.code == capi.ERR_INVALID_ARG
        ix.set_option("device_queries", -1)
    finally:
        ix.close()


def test_refused_handles_and_sizes():
    dim = 15681                                              # one past what a workgroup's LDS holds (include/bbq.h)
    ix = _index(dim)
    try:
        with pytest.raises(B.BBQError) as e:
            ix.quantize_queries(np.ones((2, dim), np.float32), np.zeros(dim, np.float32), 1)
        assert e.value.code == capi.ERR_UNSUPPORTED and "15680" in str(e.value)
    finally:
        ix.close()
    ix = _index(15680)
    try:
        assert _check(ix, Q.benign(3, 15680), Q.benign(1, 15680, 2)[0], 1, 4, 0.1, 5, "the widest query", oracle_rows=(2,))[0] == capi.OK
    finally:
        ix.close()
    if B.device_count() > 1:
        mx = B.Index.create_multi(np.zeros((128, 2), np.uint8), np.zeros((128, 4)), 13, 0.0, [0, 1])
        try:
            with pytest.raises(B.BBQError) as e:
                mx.quantize_queries(Q.benign(2, 13), Q.benign(1, 13, 2)[0], 1)
            assert e.value.code == capi.ERR_UNSUPPORTED
        finally:
            mx.close()
