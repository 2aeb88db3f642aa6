"""GPU: range search - bbq_count_range_batch, bbq_search_range_batch - against the golden per-row scores and the oracle.  Bit-exact:
the answer of a query is every row whose f32 score (what bbq_score_rows delivers) is >= its threshold as IEEE floats compare, no NaN
score ever, in ascending ord, each with that score; with a filter, of the accepted rows only."""
import functools

import numpy as np
import pytest

import orclib as O
import append_recipe as R
import test_gpu_score_ords as SO          # its fixtures and per-row golden arrays (_case: computed once, shared, never written to)
from test_range_key_cpu import range_answer
from bbqlib import bbq_amd as B, capi

pytestmark = pytest.mark.gpu

F = np.float32
INF = F(np.inf)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def thresholds_of(s32):
    """the thresholds every query is asked with: the ends, the zeros, its own minimum / median / maximum exactly, and their neighbours"""
    fin = np.sort(s32[~np.isnan(s32)])
    lo, med, hi = (fin[0], fin[len(fin) // 2], fin[-1]) if len(fin) else (F(0), F(0), F(0))
    with np.errstate(over="ignore"):
        return np.array([-INF, INF, -1.0, 0.0, -0.0, lo, med, hi, np.nextafter(hi, INF), np.nextafter(med, -INF)], np.float32)


EMPTY_AT = 8     # nextafter(max, +inf): no score reaches it - it stands between two thresholds that a row does reach


def assert_range(ix, qqs, qcs, qb, sim, ths, golden, msg, flt=None, mask=None):
    """one call for all the queries: idx, offsets and score bits equal the numpy restatement over the golden f32 scores"""
    idx, sc, off = ix.search_range_batch(qqs, qcs, qb, sim, ths, flt)
    cnt = ix.count_range_batch(qqs, qcs, qb, sim, ths, flt)
    want = [range_answer(g, t) for g, t in zip(golden, ths)]
    if mask is not None:
        want = [w[mask[w]] for w in want]
    np.testing.assert_array_equal(cnt, [len(w) for w in want], err_msg=msg + ": counts")
    np.testing.assert_array_equal(off, np.concatenate([[0], np.cumsum([len(w) for w in want])]), err_msg=msg + ": offsets")
    assert len(idx) == len(sc) == off[-1]
    for q, w in enumerate(want):
        sl = slice(off[q], off[q + 1])
        np.testing.assert_array_equal(idx[sl], w, err_msg="%s: query %d threshold %r" % (msg, q, ths[q]))
        np.testing.assert_array_equal(bits(sc[sl]), bits(golden[q][w]), err_msg="%s: query %d threshold %r: score bits" % (msg, q, ths[q]))
    return want


def _all_pairs(qs, golden):
    """every (query, threshold) pair of a fixture as the queries of ONE call"""
    qqs, qcs, ths, gold = [], [], [], []
    for (qq, qc), g in zip(qs, golden):
        for t in thresholds_of(g):
            qqs.append(qq), qcs.append(qc), ths.append(t), gold.append(g)
    return np.stack(qqs), np.stack(qcs), np.array(ths, np.float32), gold


@pytest.mark.parametrize("compact", [True, False])
@pytest.mark.parametrize("name", SO.FIXTURES)
def test_golden_answers(name, compact):
    g, sim, codes, corr, cdp, qs = SO._case(name)
    golden = [q[4] for q in qs]
    ix = B.Index(codes, corr, g["dim"], cdp, index_bits=g["ib"], corrections="compact" if compact else "inline")
    try:
        qqs, qcs, ths, gold = _all_pairs([(q[0], q[1]) for q in qs], golden)
        want = assert_range(ix, qqs, qcs, g["qb"], sim, ths, gold, name)
        per = len(ths) // len(qs)
        for q in range(len(qs)):
            w = want[q * per:(q + 1) * per]
            assert len(w[EMPTY_AT]) == 0 and len(w[1]) == 0                      # above the maximum; +inf (no golden score is +inf)
            np.testing.assert_array_equal(w[3], w[4])                            # +0.0 and -0.0
            np.testing.assert_array_equal(w[0], np.flatnonzero(~np.isnan(golden[q])))   # -inf: every row whose score is no NaN
            if name == "edge_dim1":
                assert np.isnan(golden[q]).all() and all(len(x) == 0 for x in w)
            else:
                assert len(w[EMPTY_AT - 1]) > 0 and len(w[EMPTY_AT + 1]) > 0        # a zero-length answer between two others
                # a threshold equal to a score returns every holder of that score
                for j in (5, 6, 7):
                    assert (golden[q][w[j]] == ths[q * per + j]).sum() == (golden[q] == ths[q * per + j]).sum() > 0
        if name == "ib4_96d_euc_qb4":     # the tie case: 172 and 125 of its 200 scores are exactly 0.0
            assert sorted((gg == 0.0).sum() for gg in golden) == [125, 172]
    finally:
        ix.close()


def test_explicit_component_sums():
    g, sim, codes, corr, cdp, qs = SO._explicit_sums()
    golden = [O.score_all(codes, corr, g["dim"], qq, qc, g["qb"], sim, cdp)[2] for qq, qc, *_ in qs]
    assert any((bits(a) != bits(q[4])).any() for a, q in zip(golden, qs))         # the edited sums matter
    ix = B.Index(codes, corr, g["dim"], cdp)
    try:
        assert ix.bytes_per_row == 16 + 32
        qqs, qcs, ths, gold = _all_pairs([(q[0], q[1]) for q in qs], golden)
        assert_range(ix, qqs, qcs, g["qb"], sim, ths, gold, "explicit sums")
    finally:
        ix.close()


N_BIG, DIM_BIG, CHUNK = 2100, 64, 512     # four full chunks and a 52-row tail


@functools.lru_cache(maxsize=None)
def _big():
    """a seeded index of 2100 rows, quantized by the product's quantizer, scored by the oracle; the seed is the first whose three best
    rows of query 0 lie in more than one chunk"""
    sim, qb = 1, 4
    for seed in range(50, 60):
        rng = np.random.default_rng(seed)
        base = rng.standard_normal((N_BIG, DIM_BIG)).astype(np.float32)
        queries = rng.standard_normal((2, DIM_BIG)).astype(np.float32)
        codes, corr, cen = B.quantize_vectors(base, sim)
        cdp = B.centroid_dp(cen)
        qq, qc = B.quantize_queries(queries, cen, sim, qb)
        s32 = [O.score_all(codes, corr, DIM_BIG, qq[i], qc[i], qb, sim, cdp)[2] for i in range(2)]
        top3 = np.argsort(-s32[0], kind="stable")[:3]
        if len(set(top3 // CHUNK)) >= 2 and np.sort(s32[0])[-3] > np.sort(s32[0])[-4]:
            break
    for a in (codes, corr):
        a.setflags(write=False)
    return sim, qb, codes, corr, cdp, qq, qc, s32


def _kth(s32, k):
    return np.sort(s32)[-k]


@pytest.mark.parametrize("compact", [True, False])
def test_several_chunks(compact):
    sim, qb, codes, corr, cdp, qq, qc, s32 = _big()
    ths = np.array([-INF, _kth(s32[0], 3), _kth(s32[0], 300), _kth(s32[1], 3), -INF, _kth(s32[1], 300)], np.float32)
    who = [0, 0, 0, 1, 1, 1]
    # from the oracle: the 3rd-largest threshold leaves at least two chunks without a hit and at least two with one
    hit_chunks = set(range_answer(s32[0], ths[1]) // CHUNK)
    assert len(hit_chunks) >= 2 and 5 - len(hit_chunks) >= 2
    ix = B.Index(codes, corr, DIM_BIG, cdp, corrections="compact" if compact else "inline")
    try:
        want = assert_range(ix, qq[who], qc[who], qb, sim, ths, [s32[w] for w in who], "2100 rows")
        assert len(want[0]) == N_BIG and want[0][-1] == N_BIG - 1 and len(want[1]) == 3 and len(want[2]) >= 300
    finally:
        ix.close()


def _accept_sets(n, seed):
    rng = np.random.default_rng(seed)
    none, every = np.zeros(n, bool), np.ones(n, bool)
    one_per_tile = np.zeros(n, bool)
    one_per_tile[np.minimum(np.arange(0, n, 64) + rng.integers(0, 64, (n + 63) // 64), n - 1)] = True
    tiles_cleared = np.ones(n, bool)
    for t in (0, 3, 8, (n - 1) // 64):       # a whole chunk's first tile, an inner tile, the second chunk's first, the last (partial) tile
        tiles_cleared[t * 64:(t + 1) * 64] = False
    last = np.zeros(n, bool)
    last[n - 1] = True
    return {"none": none, "all": every, "one row per tile": one_per_tile, "whole tiles cleared": tiles_cleared, "only the last row": last,
            "a random half": rng.random(n) < 0.5}


@pytest.mark.parametrize("compact", [True, False])
def test_filtered_2100_rows(compact):
    sim, qb, codes, corr, cdp, qq, qc, s32 = _big()
    ths = np.array([-INF, _kth(s32[1], 300), _kth(s32[0], 3), _kth(s32[1], 3)], np.float32)
    who = [0, 1, 0, 1]
    ix = B.Index(codes, corr, DIM_BIG, cdp, corrections="compact" if compact else "inline")
    try:
        for label, mask in _accept_sets(N_BIG, 61).items():
            with capi.Filter(ix, mask) as flt:
                want = assert_range(ix, qq[who], qc[who], qb, sim, ths, [s32[w] for w in who], "2100 rows, " + label, flt, mask)
                assert len(want[0]) == mask.sum()
    finally:
        ix.close()


@pytest.mark.parametrize("compact", [True, False])
def test_filtered_fixture(compact):
    name = "c1_1000x128_cos_qb4"
    g, sim, codes, corr, cdp, qs = SO._case(name)
    golden = [q[4] for q in qs]
    ths = np.array([-INF, _kth(golden[1], 300), _kth(golden[2], 3)], np.float32)
    qqs, qcs = np.stack([q[0] for q in qs]), np.stack([q[1] for q in qs])
    ix = B.Index(codes, corr, g["dim"], cdp, corrections="compact" if compact else "inline")
    other = B.Index(codes[:900], corr[:900], g["dim"], cdp)
    try:
        for label, mask in _accept_sets(g["n"], 62).items():
            with capi.Filter(ix, mask) as flt:
                assert_range(ix, qqs, qcs, g["qb"], sim, ths, golden, name + ", " + label, flt, mask)
        with capi.Filter(other, np.ones(900, bool)) as flt:      # a filter of another index's size
            for call in (ix.count_range_batch, ix.search_range_batch):
                with pytest.raises(B.BBQError) as e:
                    call(qqs, qcs, g["qb"], sim, ths, flt)
                assert e.value.code == capi.ERR_INVALID_ARG
    finally:
        ix.close()
        other.close()


def test_launch_bounds():
    """1100 copies of a query at -inf: more than a sub-batch of 1024 queries, and 1.1 M entries - more than a fill launch of 2^20"""
    g, sim, codes, corr, cdp, qs = SO._case("c1_1000x128_cos_qb4")
    qq, qc, _, _, s32 = qs[0]
    nq, n = 1100, g["n"]
    qqs, qcs, ths = np.repeat(qq[None, :], nq, 0), np.repeat(qc[None, :], nq, 0), np.full(nq, -INF, np.float32)
    ix = B.Index(codes, corr, g["dim"], cdp)
    try:
        idx, sc, off = ix.search_range_batch(qqs, qcs, g["qb"], sim, ths)
        np.testing.assert_array_equal(off, np.arange(nq + 1) * n)
        assert (idx.reshape(nq, n) == np.arange(n)).all()
        assert (bits(sc).reshape(nq, n) == bits(s32)).all()
        # one entry short: the offsets are written, the entries are not
        L = capi.lib()
        total = nq * n
        o2, i2, s2 = np.full(nq + 1, -7, np.int64), np.full(total - 1, -7, np.int32), np.full(total - 1, -7.0, np.float32)
        rc = L.bbq_search_range_batch(ix._h, None, nq, qqs.ctypes.data, qcs.ctypes.data, g["qb"], sim, ths.ctypes.data, total - 1,
                                      o2.ctypes.data, i2.ctypes.data, s2.ctypes.data)
        assert rc == capi.ERR_INVALID_ARG
        np.testing.assert_array_equal(o2, off)
        assert (i2 == -7).all() and (s2 == -7.0).all()
    finally:
        ix.close()


def test_agrees_with_top_k():
    g, sim, codes, corr, cdp, qs = SO._case("c1_1000x128_cos_qb4")
    ix = B.Index(codes, corr, g["dim"], cdp)
    try:
        for qq, qc, _, _, s32 in qs:
            for k in (1, 10, 100):
                top, tsc = ix.search(qq, qc, g["qb"], sim, k)
                t = tsc[k - 1]
                idx, sc, _ = ix.search_range_batch(qq[None, :], qc[None, :], g["qb"], sim, [t])
                assert set(top) <= set(idx)
                np.testing.assert_array_equal(idx, range_answer(s32, t))
                np.testing.assert_array_equal(bits(sc), bits(s32[idx]))
    finally:
        ix.close()


def test_after_mutations():
    """an append, an update and a removal on one index: every answer is the restatement over bbq_score_rows of the index as it then is"""
    g, sim, codes, corr, cdp, qs = SO._case("c1_1000x128_cos_qb4")
    base, _ = O.golden_inputs(g)
    cen = B.quantize_vectors(base, sim, g["ib"], g["lambda"], g["iters"])[2]
    rng = np.random.default_rng(63)
    new_codes, new_corr = R.oracle_rows(rng.standard_normal((130, g["dim"])).astype(np.float32), cen, sim, g["ib"], g["lambda"], g["iters"])
    qqs, qcs = np.stack([q[0] for q in qs]), np.stack([q[1] for q in qs])
    ix = B.Index(codes, corr, g["dim"], cdp)
    try:
        def check(label, n):
            assert ix.n == n
            now = [ix.score_rows(qq, qc, g["qb"], sim)[2] for qq, qc in zip(qqs, qcs)]
            ths = np.array([_kth(now[0], 5), -INF, _kth(now[2], 200)], np.float32)
            want = assert_range(ix, qqs, qcs, g["qb"], sim, ths, now, label)
            assert len(want[1]) == n
            return now
        before = check("as created", 1000)
        ix.append_rows(new_codes[:100], new_corr[:100])           # a new partial tile in a new chunk
        after = check("after the append", 1100)
        assert (bits(after[0][:1000]) == bits(before[0])).all()
        ix.update_rows(np.array([0, 511, 512, 1099], np.int32), new_codes[100:104], new_corr[100:104])
        upd = check("after the update", 1100)
        assert (bits(upd[0]) != bits(after[0])).any()
        ix.remove_rows(np.arange(64, 64 + 600))                    # the rows move down across tiles and a chunk goes
        check("after the removal", 500)
    finally:
        ix.close()


def test_arguments_and_handles():
    g, sim, codes, corr, cdp, qs = SO._case("c1_1000x128_cos_qb4")
    n = g["n"]
    qqs, qcs = np.stack([q[0] for q in qs]), np.stack([q[1] for q in qs])
    L = capi.lib()
    ix = B.Index(codes, corr, g["dim"], cdp)
    multi = B.Index.create_multi(codes, corr, g["dim"], cdp, [0, 0], pilot_rows=0)
    shard = B.Index(codes[512:], corr[512:], g["dim"], cdp, row_base=512, pilot_codes=codes[:512], pilot_corr=corr[:512])
    try:
        # a NaN threshold in the middle of the batch: refused before anything is launched or written
        ths = np.array([0.5, np.nan, 0.5], np.float32)
        off, idx, sc, cnt = np.full(4, -7, np.int64), np.full(3 * n, -7, np.int32), np.full(3 * n, -7.0, np.float32), np.full(3, -7, np.int64)
        rc = L.bbq_search_range_batch(ix._h, None, 3, qqs.ctypes.data, qcs.ctypes.data, g["qb"], sim, ths.ctypes.data, 3 * n, off.ctypes.data,
                                      idx.ctypes.data, sc.ctypes.data)
        assert rc == capi.ERR_INVALID_ARG and b"NaN" in L.bbq_last_error()
        assert L.bbq_count_range_batch(ix._h, None, 3, qqs.ctypes.data, qcs.ctypes.data, g["qb"], sim, ths.ctypes.data, cnt.ctypes.data) == capi.ERR_INVALID_ARG
        assert (off == -7).all() and (idx == -7).all() and (sc == -7.0).all() and (cnt == -7).all()
        # no queries: fine
        assert L.bbq_search_range_batch(ix._h, None, 0, None, None, g["qb"], sim, None, 0, None, None, None) == capi.OK
        assert L.bbq_count_range_batch(ix._h, None, 0, None, None, g["qb"], sim, None, None) == capi.OK
        e_idx, e_sc, e_off = ix.search_range_batch(qqs[:0], qcs[:0], g["qb"], sim, [])
        assert len(e_idx) == 0 and len(e_sc) == 0 and list(e_off) == [0]
        # cap 0 with null outputs: the offsets alone
        good = np.array([0.5, 0.6, 0.7], np.float32)
        rc = L.bbq_search_range_batch(ix._h, None, 3, qqs.ctypes.data, qcs.ctypes.data, g["qb"], sim, good.ctypes.data, 0, off.ctypes.data, None, None)
        np.testing.assert_array_equal(np.diff(off), ix.count_range_batch(qqs, qcs, g["qb"], sim, good))
        assert rc == (capi.OK if off[3] == 0 else capi.ERR_INVALID_ARG)
        # 4-bit values handed over as a 1-bit query: refused as bbq_score_rows refuses it
        with pytest.raises(B.BBQError) as e:
            ix.count_range_batch(qqs, qcs, 1, sim, good)
        assert e.value.code == capi.ERR_INVALID_ARG and str(e.value) == "1位量化值必须为0或1"
        # handles out of scope, with and without a filter
        with capi.Filter(ix, np.ones(n, bool)) as flt:
            for handle, word in ((multi, "multi-device"), (shard, "shard")):
                for f in (None, flt):
                    for call in (handle.count_range_batch, handle.search_range_batch):
                        with pytest.raises(B.BBQError) as e:
                            call(qqs, qcs, g["qb"], sim, good, f)
                        assert e.value.code == capi.ERR_UNSUPPORTED and word in str(e.value)
        # an empty filter: zeros
        with capi.Filter(ix, np.zeros(n, bool)) as flt:
            assert (ix.count_range_batch(qqs, qcs, g["qb"], sim, np.full(3, -INF), flt) == 0).all()
    finally:
        ix.close()
        multi.close()
        shard.close()


def test_python_api():
    """api.py: searchRange in ascending ord is the C answer; order="score" is that answer stably sorted by descending score"""
    g, sim, codes, corr, cdp, qs = SO._case("c1_1000x128_cos_qb4")
    base, queries = O.golden_inputs(g)
    n = g["n"]
    f = B.createBinaryQuantizationFormat({"queryBits": 4, "indexBits": 1, "quantizer": {"similarityFunction": "COSINE", "lambda": 0.1, "iters": 5}})
    tv = f.quantizeVectors(list(base))["quantizedVectors"]
    s32 = qs[0][4]
    t = float(_kth(s32, 200))
    want = range_answer(s32, t)
    by_ord = f.searchRange(queries[0], tv, t)
    assert [r["index"] for r in by_ord] == [int(i) for i in want]
    np.testing.assert_array_equal(bits([r["score"] for r in by_ord]), bits(s32[want]))
    by_score = f.searchRange(queries[0], tv, t, order="score")
    assert by_score == sorted(by_ord, key=lambda r: -r["score"])                 # sorted() is stable: ties stay in ascending ord
    assert by_score[0]["score"] == float(s32.max()) and by_score != by_ord
    mask = np.random.default_rng(64).random(n) < 0.5
    flt = B.createRowFilter(tv, mask)
    try:
        got = f.searchRange(queries[0], tv, t, rowFilter=flt)
        assert [r["index"] for r in got] == [int(i) for i in want[mask[want]]]
        assert f.searchRange(queries[0], tv, -np.inf, flt, "score") == sorted(f.searchRange(queries[0], tv, -np.inf, flt), key=lambda r: -r["score"])
    finally:
        flt.close()
    assert f.searchRange(queries[0], tv, np.inf) == []
    for bad in (lambda: f.searchRange(queries[0], tv, float("nan")), lambda: f.searchRange(None, tv, 0.5), lambda: f.searchRange(queries[0], None, 0.5),
                lambda: f.searchRange(queries[0][:5], tv, 0.5), lambda: f.searchRange(queries[0], tv, 0.5, order="best")):
        with pytest.raises(Exception):
            bad()
