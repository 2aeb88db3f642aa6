"""GPU: scoring and ranking chosen rows - bbq_score_ords, bbq_score_ords_batch, bbq_search_ords_batch - against the golden per-row
arrays and the oracle.  Bit-exact: every list entry carries the integer qcDist, the f64 score and its f32 rounding of the row it names,
whatever the order of the list; the search returns what the reference's heap returns when it visits the list in the order given."""
import functools
import itertools

import numpy as np
import pytest

import orclib as O
from bbqlib import bbq_amd as B, capi

pytestmark = pytest.mark.gpu

FIXTURES = (["c1_1000x128_cos_qb4"]                                                            # w16 1, two chunks, a partial last tile
            + ["m_768d_%s_qb%d" % (s, q) for s in ("cos", "euc", "max") for q in (1, 4)]        # compiled width 6
            + ["m_1024d_max_qb8", "m_1024d_cos_qb4", "m_1024d_euc_qb1"]                        # width 8 at 8, 4 and 1 planes
            + ["m_%s_%s_qb%d" % (d, s, q) for d in ("100d", "72d") for s in ("cos", "euc", "max") for q in (1, 4)]  # w16 1 with a ragged last chunk
            + ["qb2_128d_cos", "qb3_96d_mip",
               "ib2_1024d_cos_qb4",                                                            # multi-bit, width 16
               "ib4_96d_euc_qb4", "ib8_64d_cos_qb4", "ib3_72d_cos_qb4",
               "edge_dim1",                                                                    # its golden scores hold NaN: delivered as NaN
               "edge_n1", "edge_zero_const"])
LENGTHS = (1, 63, 64, 65, 257)   # a list that ends inside a wave, at a wave, behind one, and one that crosses a workgroup (256 entries)


def canon64(a):
    a = np.array(a, np.float64)
    a[np.isnan(a)] = np.nan
    return a.view(np.uint64)


def canon32(a):
    a = np.array(a, np.float32)
    a[np.isnan(a)] = np.nan
    return a.view(np.uint32)


@functools.lru_cache(maxsize=None)
def _case(name):
    """the fixture's rows as the product's quantizer makes them, its quantized queries and the golden per-row results: computed once,
    shared by every test, never written to"""
    g = O.load_golden(name)
    sim = O.SIMS[g["sim"]]
    base, queries = O.golden_inputs(g)
    codes, corr, cen = B.quantize_vectors(base, sim, g["ib"], g["lambda"], g["iters"])
    assert O.sha(codes) == g["codes_sha256"]
    qs = []
    for qi, rec in enumerate(g["queries"]):
        qq, qc = B.quantize_query(queries[qi], cen, sim, g["qb"], g["lambda"], g["iters"])
        want_d, want_64 = O.dec(rec["qcdist_i32"], "<i4"), O.dec(rec["score_f64"], "<f8")
        qs.append((qq, qc, want_d, want_64, want_64.astype(np.float32)))
    for a in (codes, corr):
        a.setflags(write=False)
    return g, sim, codes, corr, B.centroid_dp(cen), qs


def _lists(n, seed):
    rng = np.random.default_rng(seed)
    out = [np.arange(n - 1, -1, -1), np.array([0, n - 1]),
           np.array(sorted({e for e in (63, 64, 511, 512, n - 1) if e < n})),       # the tile and chunk edges that exist
           rng.integers(0, n, 3 * n + 7)]                                          # a random draw: duplicates guaranteed
    out += [rng.integers(0, n, m) for m in LENGTHS]
    return [np.ascontiguousarray(a, np.int32) for a in out]


def _assert_entries(got, want, ords, msg):
    d, s64, s32 = got
    np.testing.assert_array_equal(d, want[0][ords], err_msg=msg + ": integer qcDist")
    np.testing.assert_array_equal(canon64(s64), canon64(want[1][ords]), err_msg=msg + ": f64 score")
    np.testing.assert_array_equal(canon32(s32), canon32(want[2][ords]), err_msg=msg + ": f32 score")


@pytest.mark.parametrize("compact", [True, False])
@pytest.mark.parametrize("name", FIXTURES)
def test_golden_lists(name, compact):
    g, sim, codes, corr, cdp, qs = _case(name)
    ix = B.Index(codes, corr, g["dim"], cdp, index_bits=g["ib"], corrections="compact" if compact else "inline")
    try:
        lists = _lists(g["n"], 11)
        qq, qc, *want = qs[0]
        for li, ords in enumerate(lists):            # one query, one list per call
            _assert_entries(ix.score_ords(qq, qc, g["qb"], sim, ords), want, ords, "%s list %d" % (name, li))
        # every query of the fixture in one call, each with every list (rotated, so that the queries' lists differ in length)
        nq = len(qs)
        per_query = [np.concatenate(lists[q % len(lists):] + lists[:q % len(lists)]) for q in range(nq)]
        d, s64, s32, off = ix.score_ords_batch(np.stack([q[0] for q in qs]), np.stack([q[1] for q in qs]), g["qb"], sim, per_query)
        for q in range(nq):
            sl = slice(off[q], off[q + 1])
            _assert_entries((d[sl], s64[sl], s32[sl]), qs[q][2:], per_query[q], "%s batch query %d" % (name, q))
        if name == "edge_dim1":
            assert np.isnan(s64).any() and np.isnan(s32).any()
    finally:
        ix.close()


def _explicit_sums():
    g, sim, codes, corr, cdp, qs = _case("m_64d_cos_qb4")
    corr = corr.copy()
    corr[::3, 3] += 2.0
    return g, sim, codes, corr, cdp, qs


def test_explicit_component_sums():
    """quantizedComponentSum that is not the popcount: the index stores the sums (inline records with a fourth block) and the gather reads them"""
    g, sim, codes, corr, cdp, qs = _explicit_sums()
    ix = B.Index(codes, corr, g["dim"], cdp)
    try:
        assert ix.bytes_per_row == 16 + 32
        for qq, qc, _, golden64, _ in qs:
            od, o64, o32 = O.score_all(codes, corr, g["dim"], qq, qc, g["qb"], sim, cdp)
            assert (canon64(o64) != canon64(golden64)).any()     # the edited sums matter
            for li, ords in enumerate(_lists(g["n"], 12)):
                _assert_entries(ix.score_ords(qq, qc, g["qb"], sim, ords), (od, o64, o32), ords, "explicit sums list %d" % li)
    finally:
        ix.close()


def test_batch_with_empty_lists_between():
    g, sim, codes, corr, cdp, qs = _case("c1_1000x128_cos_qb4")
    rng = np.random.default_rng(13)
    lists = [rng.integers(0, g["n"], 257), np.zeros(0, np.int64), np.array([777]), rng.integers(0, g["n"], 64), np.zeros(0, np.int64)]
    five = [qs[i % len(qs)] for i in range(5)]
    ix = B.Index(codes, corr, g["dim"], cdp)
    try:
        d, s64, s32, off = ix.score_ords_batch(np.stack([q[0] for q in five]), np.stack([q[1] for q in five]), g["qb"], sim, lists)
        np.testing.assert_array_equal(off, [0, 257, 257, 258, 322, 322])
        assert len(d) == 322
        for q in (0, 2, 3):
            sl = slice(off[q], off[q + 1])
            _assert_entries((d[sl], s64[sl], s32[sl]), five[q][2:], lists[q], "query %d" % q)
        # the same as (offsets, ords), and a search over the same lists: empty lists give no results
        d2, s2, f2, _ = ix.score_ords_batch(np.stack([q[0] for q in five]), np.stack([q[1] for q in five]), g["qb"], sim,
                                            (off, np.concatenate(lists)))
        np.testing.assert_array_equal(d2, d)
        np.testing.assert_array_equal(canon64(s2), canon64(s64))
        res = ix.search_ords_batch(np.stack([q[0] for q in five]), np.stack([q[1] for q in five]), g["qb"], sim, 10, lists)
        assert [len(r[0]) for r in res] == [10, 0, 1, 10, 0]
        for q in (0, 2, 3):
            oi, osc = O.heap_topk(five[q][4][lists[q]], 10)
            np.testing.assert_array_equal(res[q][0], lists[q][oi])
            np.testing.assert_array_equal(canon32(res[q][1]), canon32(osc))
    finally:
        ix.close()


def test_null_output_pointers():
    """every subset of the three output pointers NULL: the others are what the full call delivers"""
    g, sim, codes, corr, cdp, qs = _case("m_768d_cos_qb4")
    qq, qc, *want = qs[0]
    ords = _lists(g["n"], 14)[3]
    ix = B.Index(codes, corr, g["dim"], cdp)
    try:
        full = ix.score_ords(qq, qc, g["qb"], sim, ords)
        _assert_entries(full, want, ords, "all three")
        for mask in itertools.product((True, False), repeat=3):
            got = ix.score_ords(qq, qc, g["qb"], sim, ords, want=mask)
            for have, a, b in zip(mask, got, full):
                if have:
                    np.testing.assert_array_equal(a.view(np.uint8), b.view(np.uint8), err_msg="outputs asked for: %s" % (mask,))
                else:
                    assert a is None
    finally:
        ix.close()


def _synthetic(n, dim, seed):
    rng = np.random.default_rng(seed)
    codes = rng.integers(0, 256, size=(n, dim // 8), dtype=np.uint8)
    corr = np.empty((n, 4), np.float64)
    corr[:, 0] = -0.2 - 0.1 * rng.random(n)
    corr[:, 1] = 0.2 + 0.1 * rng.random(n)
    corr[:, 2] = 0.05 * rng.standard_normal(n)
    corr[:, 3] = np.unpackbits(codes, axis=1).sum(axis=1)
    qq = rng.integers(0, 16, dim).astype(np.uint8)
    qc = np.array([-0.7, 0.9, 0.01, float(qq.sum())])
    return codes, corr, qq, qc


def test_agrees_with_score_rows_row_by_row():
    n, dim, sim = 1100, 768, 1
    codes, corr, qq, qc = _synthetic(n, dim, 15)
    rng = np.random.default_rng(16)
    ords = np.concatenate([[0, 63, 64, 511, 512, 1023, 1024, 1087, 1088, n - 1], rng.integers(0, n, 120)]).astype(np.int32)
    for compact in (True, False):
        ix = B.Index(codes, corr, dim, 0.02, corrections="compact" if compact else "inline")
        try:
            d, s64, s32 = ix.score_ords(qq, qc, 4, sim, ords)
            for i, r in enumerate(ords):
                rd, r64, r32 = ix.score_rows(qq, qc, 4, sim, int(r), 1)
                assert d[i] == rd[0] and canon64(s64[i:i + 1])[0] == canon64(r64)[0] and canon32(s32[i:i + 1])[0] == canon32(r32)[0], "row %d" % r
        finally:
            ix.close()


def test_lists_see_updates_and_appends():
    n, dim, sim = 300, 128, 0
    codes, corr, qq, qc = _synthetic(n, dim, 17)
    new_codes, new_corr, _, _ = _synthetic(73, dim, 18)
    upd = np.array([5, 64, 299], np.int32)
    ix = B.Index(codes, corr, dim, 0.02)
    try:
        before = ix.score_ords(qq, qc, 4, sim, upd)
        ix.update_rows(upd, new_codes[:3], new_corr[:3])
        ix.append_rows(new_codes[3:], new_corr[3:])
        assert ix.n == n + 70
        allc, allr = np.concatenate([codes, new_codes[3:]]), np.concatenate([corr, new_corr[3:]])
        allc[upd], allr[upd] = new_codes[:3], new_corr[:3]
        want = O.score_all(allc, allr, dim, qq, qc, 4, sim, 0.02)
        ords = np.concatenate([upd, [n + 69, n, 4, 6, n + 35], upd[::-1]]).astype(np.int32)
        got = ix.score_ords(qq, qc, 4, sim, ords)
        _assert_entries(got, want, ords, "after update and append")
        assert (got[0][:3] != before[0]).any() or (canon64(got[1][:3]) != canon64(before[1])).any()
    finally:
        ix.close()


def test_multi_device_handle():
    """three shards on device 0: every list is split by shard on the host and scattered back to list positions"""
    n, dim, sim = 2000, 128, 1
    codes, corr, qq, qc = _synthetic(n, dim, 19)
    rng = np.random.default_rng(20)
    crossing = np.array([e for b in (512, 1024, 1536) for e in (b - 1, b, b + 1, b, b - 1)] + [n - 1, 0, 1025, 3, 1999, 1023])
    lists = [crossing, np.arange(n - 1, -1, -1), rng.integers(0, n, 700), np.zeros(0, np.int64)]
    qqs, qcs = np.stack([qq] * 4), np.stack([qc] * 4)
    one = B.Index(codes, corr, dim, 0.02)
    mx = B.Index.create_multi(codes, corr, dim, 0.02, [0, 0, 0], pilot_rows=512)
    try:
        assert mx.shards >= 2
        want = one.score_ords_batch(qqs, qcs, 4, sim, lists)
        got = mx.score_ords_batch(qqs, qcs, 4, sim, lists)
        np.testing.assert_array_equal(got[0], want[0])
        np.testing.assert_array_equal(canon64(got[1]), canon64(want[1]))
        np.testing.assert_array_equal(canon32(got[2]), canon32(want[2]))
        od, o64, o32 = O.score_all(codes, corr, dim, qq, qc, 4, sim, 0.02)
        _assert_entries(mx.score_ords(qq, qc, 4, sim, crossing), (od, o64, o32), crossing, "crossing list")
        for a, b in zip(mx.search_ords_batch(qqs, qcs, 4, sim, 25, lists), one.search_ords_batch(qqs, qcs, 4, sim, 25, lists)):
            np.testing.assert_array_equal(a[0], b[0])
            np.testing.assert_array_equal(canon32(a[1]), canon32(b[1]))
        with pytest.raises(B.BBQError) as e:
            mx.score_ords(qq, qc, 4, sim, [5, n, -1])
        assert e.value.code == capi.ERR_INVALID_ARG and "向量索引 %d 不存在" % n in str(e.value)
    finally:
        one.close()
        mx.close()


@functools.lru_cache(maxsize=None)
def _ties_case(name):
    g = O.load_golden(name)
    sim = O.SIMS[g["sim"]]
    base, queries = O.golden_inputs(g)
    codes, corr, cen = B.quantize_vectors(base, sim, g["ib"], g["lambda"], g["iters"])
    assert O.sha(codes) == g["codes_sha256"]
    cdp = B.centroid_dp(cen)
    qs = []
    for qi in range(len(queries)):
        qq, qc = B.quantize_query(queries[qi], cen, sim, g["qb"], g["lambda"], g["iters"])
        _, _, s32 = O.score_all(codes, corr, g["dim"], qq, qc, g["qb"], sim, cdp, g["ib"])
        qs.append((qq, qc, s32))
    return g, sim, codes, corr, cdp, qs


@pytest.mark.parametrize("name", ["ties_cos_qb4", "ties_euc_qb4", "ib2_ties_cos_qb4"])
def test_search_ords_matches_the_reference_heap(name):
    """equal scores everywhere: which of them the heap keeps, and in which order it returns them, depends on the order of the visit"""
    g, sim, codes, corr, cdp, qs = _ties_case(name)
    n = g["n"]
    rng = np.random.default_rng(21)
    lists = [np.arange(n), np.arange(n - 1, -1, -1), rng.integers(0, n, 1500)]
    ix = B.Index(codes, corr, g["dim"], cdp, index_bits=g["ib"])
    try:
        ks = sorted({0, 1, 10, 5000} | {len(l) + e for l in lists for e in (0, 5)})
        for qi, (qq, qc, s32) in enumerate(qs):
            qqs, qcs = np.stack([qq] * len(lists)), np.stack([qc] * len(lists))
            for k in ks:
                res = ix.search_ords_batch(qqs, qcs, g["qb"], sim, k, lists)
                for li, ords in enumerate(lists):
                    oi, osc = O.heap_topk(s32[ords], k)
                    np.testing.assert_array_equal(res[li][0], ords[oi], err_msg="%s q%d k=%d list %d" % (name, qi, k, li))
                    np.testing.assert_array_equal(canon32(res[li][1]), canon32(osc))
                if 0 < k <= 5000:      # an ascending list of all rows is the search itself
                    idx, sc = ix.search(qq, qc, g["qb"], sim, k)
                    np.testing.assert_array_equal(res[0][0], idx)
                    np.testing.assert_array_equal(canon32(res[0][1]), canon32(sc))
    finally:
        ix.close()


def test_errors_launch_nothing():
    g, sim, codes, corr, cdp, qs = _case("c1_1000x128_cos_qb4")
    qq, qc, *_ = qs[0]
    n = g["n"]
    L = capi.lib()
    ix = B.Index(codes, corr, g["dim"], cdp)
    try:
        def raw_score(offsets, ords, q=qq, bits=g["qb"]):
            off, o = np.ascontiguousarray(offsets, np.int64), np.ascontiguousarray(ords, np.int32)
            d, s64, s32 = np.full(len(o), -7, np.int32), np.full(len(o), -7.0), np.full(len(o), -7.0, np.float32)
            rc = L.bbq_score_ords_batch(ix._h, len(off) - 1, q.ctypes.data, qc.ctypes.data, bits, sim, off.ctypes.data, o.ctypes.data,
                                        d.ctypes.data, s64.ctypes.data, s32.ctypes.data)
            untouched = (d == -7).all() and (s64 == -7.0).all() and (s32 == -7.0).all()
            return rc, L.bbq_last_error().decode("utf-8"), untouched

        launches = ix.stats()["total_scan_launches"]
        # the first offending entry in list order names the error
        for ords, bad in (([3, -1, n, 5], -1), ([3, n, -1], n), ([0, 1, n + 9], n + 9)):
            rc, msg, untouched = raw_score([0, len(ords)], ords)
            assert rc == capi.ERR_INVALID_ARG and msg == "向量索引 %d 不存在" % bad and untouched
        rc, msg, untouched = raw_score([0, 3, 2], [1, 2, 3])                         # descending offsets
        assert rc == capi.ERR_INVALID_ARG and untouched
        rc, msg, untouched = raw_score([1, 3], [1, 2, 3])                            # offsets[0] != 0
        assert rc == capi.ERR_INVALID_ARG and untouched
        rc, msg, untouched = raw_score([0, 3], [1, 2, 3], bits=1)                     # 4-bit values handed over as a 1-bit query
        assert rc == capi.ERR_INVALID_ARG and msg == "1位量化值必须为0或1" and untouched
        with pytest.raises(B.BBQError) as e:                                          # ... exactly as bbq_score_rows refuses it
            ix.score_rows(qq, qc, 1, sim, 0, 3)
        assert e.value.code == capi.ERR_INVALID_ARG and str(e.value) == msg
        rc, msg, untouched = raw_score([0, 3], [1, 2, 3], bits=9)
        assert rc == capi.ERR_INVALID_ARG and untouched
        rc, msg, untouched = raw_score([0, 0], [])                                    # nothing to score: fine, and nothing written
        assert rc == capi.OK and untouched
        assert L.bbq_score_ords_batch(ix._h, 0, None, None, 4, sim, None, None, None, None, None) == capi.OK
        assert L.bbq_score_ords(ix._h, qq.ctypes.data, qc.ctypes.data, 4, sim, None, -1, None, None, None) == capi.ERR_INVALID_ARG
        with pytest.raises(B.BBQError) as e:
            ix.search_ords_batch(qq[None, :], qc[None, :], g["qb"], sim, -1, [np.arange(5)])
        assert e.value.code == capi.ERR_NEGATIVE_K and "k值不能为负数" in str(e.value)
        with pytest.raises(B.BBQError) as e:                                          # an ord that names no row is an error whatever k is
            ix.search_ords_batch(qq[None, :], qc[None, :], g["qb"], sim, 0, [np.array([1, n])])
        assert e.value.code == capi.ERR_INVALID_ARG and "向量索引 %d 不存在" % n in str(e.value)
        assert [len(r[0]) for r in ix.search_ords_batch(qq[None, :], qc[None, :], g["qb"], sim, 0, [np.arange(5)])] == [0]
        assert ix.stats()["total_scan_launches"] == launches
    finally:
        ix.close()


def test_python_mirror():
    """api.py: computeBatchQuantizedScores scores the rows named; searchNearestNeighborsInOrds is the reference loop over them"""
    g, sim, codes, corr, cdp, qs = _case("c1_1000x128_cos_qb4")
    base, queries = O.golden_inputs(g)
    n = g["n"]
    f = B.createBinaryQuantizationFormat({"queryBits": 4, "indexBits": 1, "quantizer": {"similarityFunction": "COSINE", "lambda": 0.1, "iters": 5}})
    tv = f.quantizeVectors(list(base))["quantizedVectors"]
    # the scorer's own call shape: a query quantized by quantizeQueryVector, a plain list of ords
    qz = f.quantizeQueryVector(queries[0], tv.getCentroid())
    c = qz["queryCorrections"]
    qc = np.array([c["lowerInterval"], c["upperInterval"], c["additionalCorrection"], c["quantizedComponentSum"]])
    od, o64, _ = O.score_all(codes, corr, g["dim"], qz["quantizedQuery"], qc, 4, sim, cdp)
    ords = [n - 1, 0, 17, 17]
    out = f.computeBatchQuantizedScores(qz["quantizedQuery"], c, tv, ords, 4)
    assert [o["bitDotProduct"] for o in out] == [int(od[r]) for r in ords]
    np.testing.assert_array_equal(canon64([o["score"] for o in out]), canon64(o64[ords]))
    assert f.computeBatchQuantizedScores(qz["quantizedQuery"], c, tv, [], 4) == []
    # the search over a list: the oracle's heap over the list's scores, with the query as searchNearestNeighbors prepares it
    s32 = qs[0][4]
    rng = np.random.default_rng(22)
    some = rng.integers(0, n, 90)
    oi, osc = O.heap_topk(s32[some], 7)
    got = f.searchNearestNeighborsInOrds(queries[0], tv, some, 7)
    assert [r["index"] for r in got] == [int(v) for v in some[oi]]
    np.testing.assert_array_equal(canon32([r["score"] for r in got]), canon32(osc))
    assert f.searchNearestNeighborsInOrds(queries[0], tv, list(range(n)), 10) == f.searchNearestNeighbors(queries[0], tv, 10)
    assert f.searchNearestNeighborsInOrds(queries[0], tv, some, 0) == [] and f.searchNearestNeighborsInOrds(queries[0], tv, [], 3) == []
    with pytest.raises(Exception) as e:
        f.searchNearestNeighborsInOrds(queries[0], tv, [1, n], 5)
    assert "向量索引 %d 不存在" % n in str(e.value)
