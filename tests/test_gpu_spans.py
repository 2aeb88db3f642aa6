"""GPU: span search - bbq_search_spans_batch - against the golden per-row scores and the oracle's heap.  Bit-exact: a query's answer is
what the reference's loop returns when it visits exactly the rows of its spans, ascending - indices, score bits and order, ties and NaN
scores included - and out_status says which path answered, by the rule tests/test_spans_cpu.py restates: 0 (the device selected) exactly
when L > k, 1 <= k <= 4096, no NaN and no two of the k + 1 largest visited scores equal."""
import functools

import numpy as np
import pytest

import orclib as O
import append_recipe as R
import test_gpu_score_ords as SO          # its fixtures and per-row golden arrays (_case: computed once, shared, never written to)
import test_spans_cpu as SC               # the rule, the expansion and the span sets, shared with the CPU checks
from test_gpu_score_ords import canon32
from bbqlib import bbq_amd as B, capi

pytestmark = pytest.mark.gpu


def assert_spans(ix, qqs, qcs, qb, sim, k, span_lists, scores, msg):
    """one call: every query's answer equals the oracle's heap over the scores of its visited rows, mapped back to ords, and its status
    equals the rule.  scores[q] = the f32 score of every row of the index for query q.  Returns the statuses"""
    res, status = ix.search_spans_batch(qqs, qcs, qb, sim, k, span_lists)
    assert len(res) == len(span_lists) == len(status)
    for q, sp in enumerate(span_lists):
        rows = SC.expand(sp)
        v = scores[q][rows]
        oi, osc = O.heap_topk(v, k)
        where = "%s: query %d k=%d spans %s" % (msg, q, k, np.asarray(sp).tolist()[:4])
        np.testing.assert_array_equal(res[q][0], rows[oi], err_msg=where)
        np.testing.assert_array_equal(canon32(res[q][1]), canon32(osc), err_msg=where + ": score bits")
        assert status[q] == SC.expected_status(v, k), "%s: status %d, the rule says %d" % (where, status[q], SC.expected_status(v, k))
    return status


def _pairs(qs, sets):
    """every (query, span set) pair as the queries of one call"""
    qqs, qcs, lists, who = [], [], [], []
    for qi, q in enumerate(qs):
        for sp in sets:
            qqs.append(q[0]), qcs.append(q[1]), lists.append(sp), who.append(qi)
    return np.stack(qqs), np.stack(qcs), lists, who


@pytest.mark.parametrize("compact", [True, False])
@pytest.mark.parametrize("name", SO.FIXTURES)
def test_golden_answers(name, compact):
    g, sim, codes, corr, cdp, qs = SO._case(name)
    sets = SC.span_sets(g["n"])
    qqs, qcs, lists, who = _pairs(qs, sets)
    scores = [qs[w][4] for w in who]
    ix = B.Index(codes, corr, g["dim"], cdp, index_bits=g["ib"], corrections="compact" if compact else "inline")
    try:
        seen = set()
        for k in SC.k_values(sets):
            seen |= set(assert_spans(ix, qqs, qcs, g["qb"], sim, k, lists, scores, name).tolist())
        if name == "edge_dim1":      # every score is NaN: never the device's selection, always the heap's answer
            assert all(np.isnan(s).all() for s in scores)
            res, status = ix.search_spans_batch(qqs, qcs, g["qb"], sim, 1, lists)
            assert all(st == 1 for st, sp in zip(status, lists) if len(SC.expand(sp)) > 0)
        elif g["n"] > 12:
            assert seen == {0, 1}    # both paths answered
    finally:
        ix.close()


@pytest.mark.parametrize("name", SC.TIE_FIXTURES)
def test_tie_fixtures(name):
    """equal scores everywhere: which of them the heap keeps, and in which order it returns them, depends on the visit"""
    g, sim, codes, corr, cdp, qs = SO._ties_case(name)
    sets = SC.tie_span_sets(g["n"])
    qqs, qcs, lists, who = _pairs(qs, sets)
    scores = [qs[w][2] for w in who]
    ix = B.Index(codes, corr, g["dim"], cdp, index_bits=g["ib"])
    try:
        because_of_ties = 0
        for k in SC.TIE_KS + (g["n"] // 2 - 1, g["n"], g["n"] + 5):
            assert_spans(ix, qqs, qcs, g["qb"], sim, k, lists, scores, name)
            because_of_ties += sum(SC.tie_is_the_reason(s[SC.expand(sp)], k) for s, sp in zip(scores, lists))
        assert because_of_ties >= 1
    finally:
        ix.close()


N_KEYS, DIM_KEYS = 13000, 64
KEY_SPANS = [[(0, 12288)], [(711, 13000)], [(0, 13000)]]       # 12288 = the LDS key buffer, 12289 and 13000: the radix select over global memory
KEY_KS = (1, 100, 1024, 4096, 4097)


@functools.lru_cache(maxsize=None)
def _keys_case():
    """a seeded index of 13 000 rows, quantized by the product's quantizer, scored by the oracle; the seed is the first for which the
    4097 largest scores of query 0 are distinct within each of the three span sets"""
    sim, qb = 2, 4
    for seed in range(70, 100):
        rng = np.random.default_rng(seed)
        base = rng.standard_normal((N_KEYS, DIM_KEYS)).astype(np.float32)
        queries = rng.standard_normal((2, DIM_KEYS)).astype(np.float32)
        codes, corr, cen = B.quantize_vectors(base, sim)
        cdp = B.centroid_dp(cen)
        qq, qc = B.quantize_queries(queries, cen, sim, qb)
        s32 = [O.score_all(codes, corr, DIM_KEYS, qq[i], qc[i], qb, sim, cdp)[2] for i in range(2)]
        if all(SC.expected_status(s32[0][SC.expand(sp)], 4096) == 0 for sp in KEY_SPANS):
            break
    else:
        raise AssertionError("no seed with 4097 distinct largest scores")
    for a in (codes, corr):
        a.setflags(write=False)
    return sim, qb, codes, corr, cdp, qq, qc, s32


@pytest.mark.parametrize("compact", [True, False])
def test_beyond_the_lds_key_buffer(compact):
    sim, qb, codes, corr, cdp, qq, qc, s32 = _keys_case()
    assert [len(SC.expand(sp)) for sp in KEY_SPANS] == [12288, 12289, 13000]
    who = [0, 0, 0, 1, 1, 1]
    lists = [SC.spans_of(sp) for sp in KEY_SPANS] * 2
    ix = B.Index(codes, corr, DIM_KEYS, cdp, corrections="compact" if compact else "inline")
    try:
        for k in KEY_KS:
            status = assert_spans(ix, qq[who], qc[who], qb, sim, k, lists, [s32[w] for w in who], "13000 rows")
            assert list(status[:3]) == ([0, 0, 0] if k <= 4096 else [1, 1, 1])       # query 0: the device up to 4096, the host beyond
    finally:
        ix.close()


@functools.lru_cache(maxsize=None)
def _synthetic(n, dim, seed, nq=4):
    sim, qb = 1, 4
    rng = np.random.default_rng(seed)
    base = rng.standard_normal((n, dim)).astype(np.float32)
    queries = rng.standard_normal((nq, dim)).astype(np.float32)
    codes, corr, cen = B.quantize_vectors(base, sim)
    cdp = B.centroid_dp(cen)
    qq, qc = B.quantize_queries(queries, cen, sim, qb)
    s32 = [O.score_all(codes, corr, dim, qq[i], qc[i], qb, sim, cdp)[2] for i in range(nq)]
    for a in (codes, corr):
        a.setflags(write=False)
    return sim, qb, codes, corr, cdp, qq, qc, s32


def _random_spans(rng, n, m):
    """m ascending disjoint spans of an index of n rows, some of them empty, some adjacent"""
    cuts = np.sort(rng.integers(0, n + 1, 2 * m))
    return cuts.reshape(m, 2).astype(np.int64)


@pytest.mark.parametrize("compact", [True, False])
def test_equivalences(compact):
    n, dim = 2100, 64
    sim, qb, codes, corr, cdp, qq, qc, s32 = _synthetic(n, dim, 81)
    rng = np.random.default_rng(82)
    lists = [SC.spans_of([(0, n)]), _random_spans(rng, n, 1), _random_spans(rng, n, 5), _random_spans(rng, n, 40)]
    ix = B.Index(codes, corr, dim, cdp, corrections="compact" if compact else "inline")
    try:
        for k in (1, 10, 100, 3000):
            assert_spans(ix, qq, qc, qb, sim, k, lists, s32, "2100 rows")
            res, _ = ix.search_spans_batch(qq, qc, qb, sim, k, lists)
            idx, sc = ix.search(qq[0], qc[0], qb, sim, k)                               # one span over everything is the search
            np.testing.assert_array_equal(res[0][0], idx)
            np.testing.assert_array_equal(canon32(res[0][1]), canon32(sc))
            by_ords = ix.search_ords_batch(qq, qc, qb, sim, k, [SC.expand(sp).astype(np.int32) for sp in lists])
            for q, sp in enumerate(lists):
                np.testing.assert_array_equal(res[q][0], by_ords[q][0])
                np.testing.assert_array_equal(canon32(res[q][1]), canon32(by_ords[q][1]))
                mask = np.zeros(n, bool)
                mask[SC.expand(sp)] = True
                with capi.Filter(ix, mask) as flt:
                    fi, fs, fc = ix.search_filtered_batch(qq[q:q + 1], qc[q:q + 1], qb, sim, k, flt)
                np.testing.assert_array_equal(res[q][0], fi[0, :fc[0]])
                np.testing.assert_array_equal(canon32(res[q][1]), canon32(fs[0, :fc[0]]))
    finally:
        ix.close()


def test_sub_batches():
    """1025 queries - more than a sub-batch of 1024 - and 1024 queries whose scores exceed a sub-batch's 64 MiB: every query's answer
    is that of its distinct twin asked alone, and the four twins are held to the oracle"""
    n, dim, k = 17000, 64, 10
    sim, qb, codes, corr, cdp, qq, qc, s32 = _synthetic(n, dim, 83)
    small = [SC.spans_of(s) for s in ([(3, 70)], [(500, 520), (16990, 17000)], [(0, 0), (64, 128)], [(1000, 1700)])]
    whole = SC.spans_of([(0, n)])
    ix = B.Index(codes, corr, dim, cdp)
    try:
        twins_small = assert_spans(ix, qq, qc, qb, sim, k, small, s32, "twins, small spans")
        alone_small = [ix.search_spans_batch(qq[i:i + 1], qc[i:i + 1], qb, sim, k, [small[i]])[0][0] for i in range(4)]
        twins_whole = assert_spans(ix, qq, qc, qb, sim, k, [whole] * 4, s32, "twins, the whole index")
        alone_whole = [ix.search_spans_batch(qq[i:i + 1], qc[i:i + 1], qb, sim, k, [whole])[0][0] for i in range(4)]
        for nq, lists_of, alone, twins in ((1025, lambda i: small[i], alone_small, twins_small), (1024, lambda i: whole, alone_whole, twins_whole)):
            who = np.arange(nq) % 4
            assert nq > 1024 or nq * n * 4 > (64 << 20)
            res, status = ix.search_spans_batch(qq[who], qc[who], qb, sim, k, [lists_of(i) for i in who])
            np.testing.assert_array_equal(status, twins[who])
            for q in range(nq):
                np.testing.assert_array_equal(res[q][0], alone[who[q]][0], err_msg="query %d of %d" % (q, nq))
                np.testing.assert_array_equal(canon32(res[q][1]), canon32(alone[who[q]][1]))
    finally:
        ix.close()


def test_after_mutations():
    """an append, an update and a removal on one index: every answer is the oracle's heap over bbq_score_rows of the index as it then is"""
    g, sim, codes, corr, cdp, qs = SO._case("c1_1000x128_cos_qb4")
    base, _ = O.golden_inputs(g)
    cen = B.quantize_vectors(base, sim, g["ib"], g["lambda"], g["iters"])[2]
    rng = np.random.default_rng(84)
    new_codes, new_corr = R.oracle_rows(rng.standard_normal((130, g["dim"])).astype(np.float32), cen, sim, g["ib"], g["lambda"], g["iters"])
    qqs, qcs = np.stack([q[0] for q in qs]), np.stack([q[1] for q in qs])
    ix = B.Index(codes, corr, g["dim"], cdp)
    try:
        def check(label, n):
            assert ix.n == n
            now = [ix.score_rows(qq, qc, g["qb"], sim)[2] for qq, qc in zip(qqs, qcs)]
            lists = ([SC.spans_of([(0, n)]), SC.spans_of([(n - 90, n)]), SC.spans_of([(0, 1), (60, 70), (n - 3, n)])] * len(qqs))[:len(qqs)]
            for k in (5, 200):
                assert_spans(ix, qqs, qcs, g["qb"], sim, k, lists, now, label)
            return now
        before = check("as created", 1000)
        ix.append_rows(new_codes[:100], new_corr[:100])           # a new partial tile in a new chunk
        after = check("after the append", 1100)
        assert (canon32(after[0][:1000]) == canon32(before[0])).all()
        with pytest.raises(B.BBQError):                            # a span that was good before the removal below is checked against the rows of now
            ix.search_spans_batch(qqs[:1], qcs[:1], g["qb"], sim, 5, [SC.spans_of([(0, 1101)])])
        ix.update_rows(np.array([0, 511, 512, 1099], np.int32), new_codes[100:104], new_corr[100:104])
        upd = check("after the update", 1100)
        assert (canon32(upd[0]) != canon32(after[0])).any()
        ix.remove_rows(np.arange(64, 64 + 600))                    # the rows move down across tiles and a chunk goes
        check("after the removal", 500)
    finally:
        ix.close()


def test_errors_launch_nothing():
    g, sim, codes, corr, cdp, qs = SO._case("c1_1000x128_cos_qb4")
    n, k = g["n"], 5
    qqs, qcs = np.stack([q[0] for q in qs[:2]]), np.stack([q[1] for q in qs[:2]])
    L = capi.lib()
    ix = B.Index(codes, corr, g["dim"], cdp)
    multi = B.Index.create_multi(codes, corr, g["dim"], cdp, [0, 0], pilot_rows=0)
    try:
        def raw(handle, offsets, spans, k=k, qq=qqs, qc=qcs, out=True, n_out=True):
            off = np.ascontiguousarray([] if offsets is None else offsets, np.int64)
            sp = np.ascontiguousarray([] if spans is None else spans, np.int64)
            idx, sc = np.full(2 * max(k, 1), -7, np.int32), np.full(2 * max(k, 1), -7.0, np.float32)
            cnt, st = np.full(2, -7, np.int64), np.full(2, 7, np.uint8)
            rc = L.bbq_search_spans_batch(handle._h, 2, None if qq is None else qq.ctypes.data, None if qc is None else qc.ctypes.data, g["qb"], sim, k,
                                          None if offsets is None else off.ctypes.data, None if spans is None else sp.ctypes.data,
                                          idx.ctypes.data if out else None, sc.ctypes.data if out else None, cnt.ctypes.data if n_out else None, st.ctypes.data)
            untouched = (idx == -7).all() and (sc == -7.0).all() and (cnt == -7).all() and (st == 7).all()
            return rc, L.bbq_last_error().decode("utf-8"), untouched

        good = [0, 1, 3]
        rc, _, untouched = raw(ix, good, [(0, 10), (5, 9), (9, 30)])
        assert rc == capi.OK and not untouched
        for spans, where in (([(0, 10), (5, 9), (8, 30)], "query 1, span 1"),          # overlapping
                             ([(0, 10), (50, 60), (8, 30)], "query 1, span 1"),         # descending
                             ([(0, 10), (5, 9), (9, n + 1)], "query 1, span 1"),        # beyond the index
                             ([(-1, 10), (5, 9), (9, 30)], "query 0, span 0"),          # in front of it
                             ([(0, 10), (9, 5), (9, 30)], "query 1, span 0"),           # begin > end
                             ([(12, 10), (5, 9), (8, 30)], "query 0, span 0")):         # two bad spans: the first in call order is named
            rc, msg, untouched = raw(ix, good, spans)
            assert rc == capi.ERR_INVALID_ARG and where in msg and untouched, (spans, msg)
        ok_spans = [(0, 10), (5, 9), (9, 30)]
        for kw in (dict(offsets=None, spans=ok_spans), dict(offsets=good, spans=None), dict(offsets=good, spans=ok_spans, qq=None),
                   dict(offsets=good, spans=ok_spans, qc=None), dict(offsets=good, spans=ok_spans, out=False), dict(offsets=good, spans=ok_spans, n_out=False),
                   dict(offsets=[0, 2, 1], spans=ok_spans), dict(offsets=[1, 2, 3], spans=ok_spans)):
            rc, msg, untouched = raw(ix, **kw)
            assert rc == capi.ERR_INVALID_ARG and msg and untouched, kw
        rc, msg, untouched = raw(ix, good, ok_spans, k=-1)
        assert rc == capi.ERR_NEGATIVE_K and untouched
        rc, msg, untouched = raw(multi, good, ok_spans)
        assert rc == capi.ERR_UNSUPPORTED and "multi-device" in msg and untouched
        # nothing to answer is no error: no queries, k == 0, empty lists - out_n and the statuses are written
        assert L.bbq_search_spans_batch(ix._h, 0, None, None, g["qb"], sim, k, None, None, None, None, None, None) == capi.OK
        res, status = ix.search_spans_batch(qqs, qcs, g["qb"], sim, 0, [SC.spans_of(ok_spans[:1]), SC.spans_of(ok_spans[1:])])
        assert all(len(r[0]) == 0 for r in res) and (status == 0).all()
        res, status = ix.search_spans_batch(qqs, qcs, g["qb"], sim, k, [SC.spans_of([]), SC.spans_of([(4, 4)])])
        assert all(len(r[0]) == 0 for r in res) and (status == 0).all()
    finally:
        ix.close()
        multi.close()


def test_python_api():
    """api.py: searchNearestNeighborsInSpans returns what searchNearestNeighbors returns, over the rows of the spans"""
    g, sim, codes, corr, cdp, qs = SO._case("c1_1000x128_cos_qb4")
    base, queries = O.golden_inputs(g)
    f = B.createBinaryQuantizationFormat({"queryBits": 4, "indexBits": 1, "quantizer": {"similarityFunction": "COSINE", "lambda": 0.1, "iters": 5}})
    tv = f.quantizeVectors(list(base))["quantizedVectors"]
    s32 = qs[0][4]
    assert f.searchNearestNeighborsInSpans(queries[0], tv, [(0, g["n"])], 10) == f.searchNearestNeighbors(queries[0], tv, 10)
    spans = [(10, 200), (200, 200), (640, 900)]
    rows = SC.expand(spans)
    oi, osc = O.heap_topk(s32[rows], 7)
    got = f.searchNearestNeighborsInSpans(queries[0], tv, spans, 7)
    assert [r["index"] for r in got] == [int(i) for i in rows[oi]]
    np.testing.assert_array_equal(canon32([r["score"] for r in got]), canon32(osc))
    assert f.searchNearestNeighborsInSpans(queries[0], tv, [], 7) == []
    for bad in (lambda: f.searchNearestNeighborsInSpans(queries[0], tv, [(5, 3)], 7), lambda: f.searchNearestNeighborsInSpans(queries[0], tv, None, 7),
                lambda: f.searchNearestNeighborsInSpans(None, tv, spans, 7), lambda: f.searchNearestNeighborsInSpans(queries[0], tv, spans, -1),
                lambda: f.searchNearestNeighborsInSpans(queries[0], tv, [(0, 10), (5, 20)], 7)):
        with pytest.raises(Exception):
            bad()
