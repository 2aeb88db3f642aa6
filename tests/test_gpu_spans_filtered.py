"""GPU: filtered span search - bbq_search_spans_filtered_batch - against the golden per-row scores and the oracle's heap.  Bit-exact: a
query's answer is what the reference's loop returns when it visits exactly the rows of its spans that the filter accepts, ascending -
indices (original ords), score bits and order, ties and NaN scores included - and out_status says which path answered, by the rule
tests/test_spans_filtered_cpu.py restates: 0 (the device selected) exactly when A > k, 1 <= k <= 4096, no accepted score is NaN and no
two of the k + 1 largest accepted scores are equal."""
import functools

import numpy as np
import pytest

import orclib as O
import append_recipe as R
import test_gpu_score_ords as SO          # its fixtures and per-row golden arrays (_case: computed once, shared, never written to)
import test_gpu_spans as GS               # its seeded indexes (_keys_case, _synthetic: computed once, shared, never written to)
import test_spans_cpu as SC
import test_spans_filtered_cpu as FC      # the masks, the k sets and the rule, shared with the CPU checks
from test_gpu_score_ords import canon32
from bbqlib import bbq_amd as B, capi

pytestmark = pytest.mark.gpu


def assert_filtered(ix, flt, mask, qqs, qcs, qb, sim, k, span_lists, scores, msg):
    """one call: every query's answer equals the oracle's heap over the scores of its accepted visited rows, mapped back to ords, and its
    status equals the rule.  scores[q] = the f32 score of every row of the index for query q.  Returns the answers and the statuses"""
    res, status = ix.search_spans_filtered_batch(qqs, qcs, qb, sim, k, span_lists, flt)
    assert len(res) == len(span_lists) == len(status)
    for q, sp in enumerate(span_lists):
        rows = FC.accepted(mask, sp)
        v = scores[q][rows]
        oi, osc = O.heap_topk(v, k)
        where = "%s: query %d k=%d spans %s" % (msg, q, k, np.asarray(sp).tolist()[:4])
        np.testing.assert_array_equal(res[q][0], rows[oi], err_msg=where)
        np.testing.assert_array_equal(canon32(res[q][1]), canon32(osc), err_msg=where + ": score bits")
        assert status[q] == SC.expected_status(v, k), "%s: status %d, the rule says %d" % (where, status[q], SC.expected_status(v, k))
    return res, status


def assert_same(a, b, msg=""):
    """two answers of search_spans*_batch / search_ords_batch: the same ords and score bits"""
    assert len(a) == len(b)
    for q, (x, y) in enumerate(zip(a, b)):
        np.testing.assert_array_equal(x[0], y[0], err_msg="%s query %d" % (msg, q))
        np.testing.assert_array_equal(canon32(x[1]), canon32(y[1]), err_msg="%s query %d: score bits" % (msg, q))


@pytest.mark.parametrize("compact", [True, False])
@pytest.mark.parametrize("name", SO.FIXTURES)
def test_golden_answers(name, compact):
    """every query with every span set in one call, per mask and k.  The span sets carry the edges: (63, 65), (511, 513) and (64, 128)
    against tile_out_and_ends' rejected tile 1, one-row spans every 7 rows against drop_every_third, the partial last tile, and
    A in {k - 1, k, k + 1} from the mask's k set"""
    g, sim, codes, corr, cdp, qs = SO._case(name)
    n = g["n"]
    sets = SC.span_sets(n)
    qqs, qcs, lists, who = GS._pairs(qs, sets)
    scores = [qs[w][4] for w in who]
    ix = B.Index(codes, corr, g["dim"], cdp, index_bits=g["ib"], corrections="compact" if compact else "inline")
    try:
        seen = set()
        for mname, mask in FC.masks(n).items():
            with capi.Filter(ix, mask) as flt:
                assert flt.count == mask.sum()
                for k in FC.k_values(mask, sets):
                    res, status = assert_filtered(ix, flt, mask, qqs, qcs, g["qb"], sim, k, lists, scores, "%s %s" % (name, mname))
                    seen |= set(status.tolist())
                    if mname == "none":
                        assert all(len(r[0]) == 0 for r in res) and (status == 0).all()
                if name == "edge_dim1" and mname != "none":   # every score is NaN: never the device's selection, always the heap's answer
                    assert all(np.isnan(s).all() for s in scores)
                    res, status = ix.search_spans_filtered_batch(qqs, qcs, g["qb"], sim, 1, lists, flt)
                    assert all(st == (1 if len(FC.accepted(mask, sp)) > 0 else 0) for st, sp in zip(status, lists))
        if name != "edge_dim1" and n > 12:
            assert seen == {0, 1}    # both paths answered
    finally:
        ix.close()


N_NAN, DIM_NAN, NAN_ROW = 200, 64, 77
NAN_LISTS = [SC.spans_of(s) for s in ([(0, N_NAN)], [(64, 128)], [(10, 78), (150, 190)])]               # each holds row 77
NAN_KS = (1, 5, 10)
NAN_REJECTED = np.ones(N_NAN, bool)       # row 77 and every fifth row are rejected ...
NAN_REJECTED[NAN_ROW] = False
NAN_REJECTED[3::5] = False
NAN_ACCEPTED = ~NAN_REJECTED              # ... and here they are the accepted ones


@functools.lru_cache(maxsize=None)
def _nan_case():
    """200 x 64 rows as bbq_index_create takes them, row 77's additive correction set to NaN: exactly that row scores NaN.  The seed is
    the first for which the rule gives status 0 for every query, list and k of the test once that row is rejected"""
    sim, qb = 1, 4
    for seed in range(300, 330):
        rng = np.random.default_rng(seed)
        base = rng.standard_normal((N_NAN, DIM_NAN)).astype(np.float32)
        queries = rng.standard_normal((3, DIM_NAN)).astype(np.float32)
        codes, corr, cen = B.quantize_vectors(base, sim)
        corr = corr.copy()
        corr[NAN_ROW, 2] = np.nan
        cdp = B.centroid_dp(cen)
        qq, qc = B.quantize_queries(queries, cen, sim, qb)
        s32 = [O.score_all(codes, corr, DIM_NAN, qq[i], qc[i], qb, sim, cdp)[2] for i in range(3)]
        if all(FC.expected_status(s, NAN_REJECTED, sp, k) == 0 for s in s32 for sp in NAN_LISTS for k in NAN_KS):
            break
    else:
        raise AssertionError("no seed without equal scores among the largest")
    for s in s32:
        assert np.isnan(s[NAN_ROW]) and np.isnan(s).sum() == 1
    for a in (codes, corr):
        a.setflags(write=False)
    return sim, qb, codes, corr, cdp, qq, qc, s32


@pytest.mark.parametrize("compact", [True, False])
def test_nan_and_the_filter(compact):
    """a NaN score on a rejected row changes nothing - the device selects, status 0; on an accepted row it sends the query to the heap,
    status 1.  Creation accepts a row with a NaN correction in both layouts (nothing checks the corrections), so both run"""
    sim, qb, codes, corr, cdp, qq, qc, s32 = _nan_case()
    assert NAN_ACCEPTED[NAN_ROW] and not NAN_REJECTED[NAN_ROW] and all(NAN_ROW in SC.expand(sp) for sp in NAN_LISTS)
    ix = B.Index(codes, corr, DIM_NAN, cdp, corrections="compact" if compact else "inline")
    try:
        assert np.isnan(ix.score_rows(qq[0], qc[0], qb, sim)[2]).nonzero()[0].tolist() == [NAN_ROW]
        for mask, want in ((NAN_REJECTED, 0), (NAN_ACCEPTED, 1), (np.ones(N_NAN, bool), 1)):
            with capi.Filter(ix, mask) as flt:
                for k in NAN_KS:
                    _, status = assert_filtered(ix, flt, mask, qq, qc, qb, sim, k, NAN_LISTS, s32, "NaN row, expected status %d" % want)
                    assert (status == want).all()
    finally:
        ix.close()


@pytest.mark.parametrize("compact", [True, False])
def test_equivalences(compact):
    n, dim = 2100, 64
    sim, qb, codes, corr, cdp, qq, qc, s32 = GS._synthetic(n, dim, 81)
    rng = np.random.default_rng(85)
    lists = [SC.spans_of([(0, n)]), GS._random_spans(rng, n, 1), GS._random_spans(rng, n, 5), GS._random_spans(rng, n, 40)]
    masks = FC.masks(n)
    ix = B.Index(codes, corr, dim, cdp, corrections="compact" if compact else "inline")
    try:
        with capi.Filter(ix, masks["all"]) as all_rows:
            for k in (1, 10, 100, 3000):
                plain, plain_status = ix.search_spans_batch(qq, qc, qb, sim, k, lists)
                for flt in (all_rows, None):                                  # every row accepted, and no filter: the span search
                    res, status = ix.search_spans_filtered_batch(qq, qc, qb, sim, k, lists, flt)
                    assert_same(res, plain, "all rows")
                    np.testing.assert_array_equal(status, plain_status)
                for mname in ("random_half", "sparse_61"):
                    mask = masks[mname]
                    with capi.Filter(ix, mask) as flt:
                        res, _ = assert_filtered(ix, flt, mask, qq, qc, qb, sim, k, lists, s32, "2100 rows %s" % mname)
                    by_ords = ix.search_ords_batch(qq, qc, qb, sim, k, [FC.accepted(mask, sp).astype(np.int32) for sp in lists])
                    assert_same(res, by_ords, "search_ords_batch")
                    for q, sp in enumerate(lists):
                        both = np.zeros(n, bool)
                        both[FC.accepted(mask, sp)] = True                   # mask AND the span union
                        with capi.Filter(ix, both) as flt:
                            fi, fs, fc = ix.search_filtered_batch(qq[q:q + 1], qc[q:q + 1], qb, sim, k, flt)
                        assert_same([res[q]], [(fi[0, :fc[0]], fs[0, :fc[0]])], "search_filtered_batch")
    finally:
        ix.close()


KEY_KS = (1, 100, 1024, 4096, 4097)
KEY_COUNTS = (12288, 12289, 12900)        # 12288 = the LDS key buffer; beyond it the radix select over global memory
KEY_SEEDS = range(400, 430)


@functools.lru_cache(maxsize=None)
def _key_masks():
    """masks of the 13 000-row index accepting exactly 12 288, 12 289 and 12 900 rows: the first rows of a seeded random permutation.
    The seed is the first of KEY_SEEDS for which the rule gives status 0 at k = 4096 for query 0 under all three"""
    s32 = GS._keys_case()[7]
    for seed in KEY_SEEDS:
        perm = np.random.default_rng(seed).permutation(GS.N_KEYS)
        masks = []
        for c in KEY_COUNTS:
            m = np.zeros(GS.N_KEYS, bool)
            m[perm[:c]] = True
            masks.append(m)
        if all(SC.expected_status(s32[0][m], 4096) == 0 for m in masks):
            return seed, masks
    raise AssertionError("no seed in %r leaves 4097 distinct largest scores under all three masks" % (KEY_SEEDS,))


@pytest.mark.parametrize("compact", [True, False])
def test_beyond_the_lds_key_buffer(compact):
    sim, qb, codes, corr, cdp, qq, qc, s32 = GS._keys_case()
    _, masks = _key_masks()
    assert [int(m.sum()) for m in masks] == list(KEY_COUNTS)
    whole = [SC.spans_of([(0, GS.N_KEYS)])] * 2
    ix = B.Index(codes, corr, GS.DIM_KEYS, cdp, corrections="compact" if compact else "inline")
    try:
        for mask in masks:
            with capi.Filter(ix, mask) as flt:
                for k in KEY_KS:
                    _, status = assert_filtered(ix, flt, mask, qq, qc, qb, sim, k, whole, s32, "13000 rows, %d accepted" % mask.sum())
                    assert status[0] == (0 if k <= 4096 else 1)               # query 0: the device up to 4096, the host beyond
    finally:
        ix.close()


def test_sub_batches():
    """1025 queries - more than a sub-batch of 1024 - and 1024 queries whose scores and ords exceed a sub-batch's 64 MiB: every query's
    answer and status is that of its distinct twin asked alone, and the four twins are held to the oracle"""
    n, dim, k = 17000, 64, 10
    sim, qb, codes, corr, cdp, qq, qc, s32 = GS._synthetic(n, dim, 83)
    small = [SC.spans_of(s) for s in ([(3, 70)], [(500, 520), (16990, 17000)], [(0, 0), (64, 128)], [(1000, 1700)])]
    whole = SC.spans_of([(0, n)])
    mask = np.random.default_rng(86).random(n) < 0.9
    A = int(mask.sum())
    ix = B.Index(codes, corr, dim, cdp)
    try:
        with capi.Filter(ix, mask) as flt:
            _, twins_small = assert_filtered(ix, flt, mask, qq, qc, qb, sim, k, small, s32, "twins, small spans")
            alone_small = [ix.search_spans_filtered_batch(qq[i:i + 1], qc[i:i + 1], qb, sim, k, [small[i]], flt)[0][0] for i in range(4)]
            _, twins_whole = assert_filtered(ix, flt, mask, qq, qc, qb, sim, k, [whole] * 4, s32, "twins, the whole index")
            alone_whole = [ix.search_spans_filtered_batch(qq[i:i + 1], qc[i:i + 1], qb, sim, k, [whole], flt)[0][0] for i in range(4)]
            for nq, lists_of, alone, twins in ((1025, lambda i: small[i], alone_small, twins_small), (1024, lambda i: whole, alone_whole, twins_whole)):
                who = np.arange(nq) % 4
                assert nq > 1024 or nq * A * 8 > (64 << 20)
                res, status = ix.search_spans_filtered_batch(qq[who], qc[who], qb, sim, k, [lists_of(i) for i in who], flt)
                np.testing.assert_array_equal(status, twins[who])
                assert_same(res, [alone[w] for w in who], "%d queries" % nq)
    finally:
        ix.close()


def test_sparse_filter():
    """one accepted row in 17 000 under whole-index spans: that row for every k >= 1, from the one work item that is launched; one
    accepted row per chunk of 512 rows: the oracle's answer"""
    n, dim = 17000, 64
    sim, qb, codes, corr, cdp, qq, qc, s32 = GS._synthetic(n, dim, 83)
    whole = [SC.spans_of([(0, n)])] * len(qq)
    rng = np.random.default_rng(87)
    per_chunk = np.zeros(n, bool)
    per_chunk[np.arange(0, n, 512) + rng.integers(0, n % 512, (n + 511) // 512)] = True        # (the last chunk has n % 512 rows)
    assert per_chunk.sum() == 34
    ix = B.Index(codes, corr, dim, cdp)
    try:
        for row in (0, 8191, 8192, 12345, n - 1):
            one = np.zeros(n, bool)
            one[row] = True
            with capi.Filter(ix, one) as flt:
                for k in (1, 10, 5000):
                    res, status = assert_filtered(ix, flt, one, qq, qc, qb, sim, k, whole, s32, "one accepted row")
                    assert all(r[0].tolist() == [row] for r in res) and (status == 1).all()      # A == 1 <= k: the heap's answer
        with capi.Filter(ix, per_chunk) as flt:
            for k in (1, 10, 33, 34, 40):
                assert_filtered(ix, flt, per_chunk, qq, qc, qb, sim, k, whole[:3] + [SC.spans_of([(300, 9000), (9100, 16999)])], s32, "one row per chunk")
    finally:
        ix.close()


def _raw(L, handle, flt, g, sim, qq, qc, k, offsets, spans, out=True, n_out=True):
    """the C entry point with prefilled outputs: (rc, message, outputs untouched)"""
    off = np.ascontiguousarray([] if offsets is None else offsets, np.int64)
    sp = np.ascontiguousarray([] if spans is None else spans, np.int64)
    idx, sc = np.full(2 * max(k, 1), -7, np.int32), np.full(2 * max(k, 1), -7.0, np.float32)
    cnt, st = np.full(2, -7, np.int64), np.full(2, 7, np.uint8)
    rc = L.bbq_search_spans_filtered_batch(handle._h, None if flt is None else flt._h, 2, None if qq is None else qq.ctypes.data,
                                           None if qc is None else qc.ctypes.data, g["qb"], sim, k,
                                           None if offsets is None else off.ctypes.data, None if spans is None else sp.ctypes.data,
                                           idx.ctypes.data if out else None, sc.ctypes.data if out else None, cnt.ctypes.data if n_out else None, st.ctypes.data)
    untouched = (idx == -7).all() and (sc == -7.0).all() and (cnt == -7).all() and (st == 7).all()
    return rc, L.bbq_last_error().decode("utf-8"), untouched


def test_after_mutations():
    """a filter made before an update still serves and the answers follow bbq_score_rows of the index as it then is; after an append or a
    removal the old filter is refused with nothing written and a new one serves"""
    g, sim, codes, corr, cdp, qs = SO._case("c1_1000x128_cos_qb4")
    base, _ = O.golden_inputs(g)
    cen = B.quantize_vectors(base, sim, g["ib"], g["lambda"], g["iters"])[2]
    rng = np.random.default_rng(88)
    new_codes, new_corr = R.oracle_rows(rng.standard_normal((130, g["dim"])).astype(np.float32), cen, sim, g["ib"], g["lambda"], g["iters"])
    qqs, qcs = np.stack([q[0] for q in qs]), np.stack([q[1] for q in qs])
    L = capi.lib()
    ix = B.Index(codes, corr, g["dim"], cdp)
    try:
        def check(label, flt, mask):
            n = ix.n
            assert len(mask) == n
            now = [ix.score_rows(qq, qc, g["qb"], sim)[2] for qq, qc in zip(qqs, qcs)]
            lists = ([SC.spans_of([(0, n)]), SC.spans_of([(n - 90, n)]), SC.spans_of([(0, 1), (60, 70), (n - 3, n)])] * len(qqs))[:len(qqs)]
            for k in (5, 200):
                assert_filtered(ix, flt, mask, qqs, qcs, g["qb"], sim, k, lists, now, label)
            return now

        def refused(flt):
            rc, msg, untouched = _raw(L, ix, flt, g, sim, qqs[:2], qcs[:2], 5, [0, 1, 2], [(0, 10), (5, 9)])
            assert rc == capi.ERR_INVALID_ARG and "filter" in msg and untouched, msg

        mask = FC.masks(1000)["random_half"]
        old = capi.Filter(ix, mask)
        before = check("as created", old, mask)
        ix.update_rows(np.array([0, 511, 512, 999], np.int32), new_codes[100:104], new_corr[100:104])
        upd = check("after the update, the filter made before it", old, mask)
        assert (canon32(upd[0]) != canon32(before[0])).any()
        ix.append_rows(new_codes[:100], new_corr[:100])                # a new partial tile in a new chunk
        assert ix.n == 1100
        refused(old)
        mask2 = np.concatenate([mask, np.arange(100) % 2 == 0])
        with capi.Filter(ix, mask2) as flt2:
            check("after the append", flt2, mask2)
            ix.remove_rows(np.arange(64, 64 + 600))                     # the rows move down across tiles and a chunk goes
            assert ix.n == 500
            refused(flt2)
        refused(old)
        old.close()
        mask3 = FC.masks(500)["drop_every_third"]
        with capi.Filter(ix, mask3) as flt3:
            check("after the removal", flt3, mask3)
    finally:
        ix.close()


def test_errors_launch_nothing():
    g, sim, codes, corr, cdp, qs = SO._case("c1_1000x128_cos_qb4")
    n, k = g["n"], 5
    qqs, qcs = np.stack([q[0] for q in qs[:2]]), np.stack([q[1] for q in qs[:2]])
    L = capi.lib()
    ix = B.Index(codes, corr, g["dim"], cdp)
    other = B.Index(codes[:900], corr[:900], g["dim"], cdp)
    multi = B.Index.create_multi(codes, corr, g["dim"], cdp, [0, 0], pilot_rows=0)
    flt = capi.Filter(ix, FC.masks(n)["random_half"])
    flt_other = capi.Filter(other, FC.masks(900)["random_half"])
    try:
        def raw(handle, offsets, spans, k=k, qq=qqs, qc=qcs, f=flt, **kw):
            return _raw(L, handle, f, g, sim, qq, qc, k, offsets, spans, **kw)

        good = [0, 1, 3]
        rc, _, untouched = raw(ix, good, [(0, 10), (5, 9), (9, 30)])
        assert rc == capi.OK and not untouched
        for spans, where in (([(0, 10), (5, 9), (8, 30)], "query 1, span 1"),          # overlapping
                             ([(0, 10), (50, 60), (8, 30)], "query 1, span 1"),         # descending
                             ([(0, 10), (5, 9), (9, n + 1)], "query 1, span 1"),        # beyond the index
                             ([(-1, 10), (5, 9), (9, 30)], "query 0, span 0"),          # in front of it
                             ([(0, 10), (9, 5), (9, 30)], "query 1, span 0"),           # begin > end
                             ([(12, 10), (5, 9), (8, 30)], "query 0, span 0")):         # two bad spans: the first in call order is named
            for f in (flt, None):
                rc, msg, untouched = raw(ix, good, spans, f=f)
                assert rc == capi.ERR_INVALID_ARG and where in msg and "bbq_search_spans_filtered_batch" in msg and untouched, (spans, msg)
        ok_spans = [(0, 10), (5, 9), (9, 30)]
        for kw in (dict(offsets=None, spans=ok_spans), dict(offsets=good, spans=None), dict(offsets=good, spans=ok_spans, qq=None),
                   dict(offsets=good, spans=ok_spans, qc=None), dict(offsets=good, spans=ok_spans, out=False), dict(offsets=good, spans=ok_spans, n_out=False),
                   dict(offsets=[0, 2, 1], spans=ok_spans), dict(offsets=[1, 2, 3], spans=ok_spans)):
            rc, msg, untouched = raw(ix, **kw)
            assert rc == capi.ERR_INVALID_ARG and msg and untouched, kw
        rc, msg, untouched = raw(ix, good, ok_spans, k=-1)
        assert rc == capi.ERR_NEGATIVE_K and untouched
        rc, msg, untouched = raw(ix, good, ok_spans, f=flt_other)                      # a filter of an index of another size
        assert rc == capi.ERR_INVALID_ARG and "900" in msg and untouched, msg
        for f in (flt, None):
            rc, msg, untouched = raw(multi, good, ok_spans, f=f)
            assert rc == capi.ERR_UNSUPPORTED and "multi-device" in msg and untouched
        # nothing to answer is no error: no queries, k == 0, empty lists, nothing accepted - out_n and the statuses are written
        assert L.bbq_search_spans_filtered_batch(ix._h, flt._h, 0, None, None, g["qb"], sim, k, None, None, None, None, None, None) == capi.OK
        res, status = ix.search_spans_filtered_batch(qqs, qcs, g["qb"], sim, 0, [SC.spans_of(ok_spans[:1]), SC.spans_of(ok_spans[1:])], flt)
        assert all(len(r[0]) == 0 for r in res) and (status == 0).all()
        res, status = ix.search_spans_filtered_batch(qqs, qcs, g["qb"], sim, k, [SC.spans_of([]), SC.spans_of([(4, 4)])], flt)
        assert all(len(r[0]) == 0 for r in res) and (status == 0).all()
        with capi.Filter(ix, np.zeros(n, bool)) as nothing:
            rc, _, untouched = raw(ix, good, ok_spans, f=nothing)
            assert rc == capi.OK and not untouched
            res, status = ix.search_spans_filtered_batch(qqs, qcs, g["qb"], sim, k, [SC.spans_of(ok_spans[:1]), SC.spans_of(ok_spans[1:])], nothing)
            assert all(len(r[0]) == 0 for r in res) and (status == 0).all()
    finally:
        flt.close()
        flt_other.close()
        ix.close()
        other.close()
        multi.close()


def test_python_api():
    """api.py: searchNearestNeighborsInSpansFiltered returns what searchNearestNeighbors returns, over the accepted rows of the spans"""
    g, sim, codes, corr, cdp, qs = SO._case("c1_1000x128_cos_qb4")
    base, queries = O.golden_inputs(g)
    f = B.createBinaryQuantizationFormat({"queryBits": 4, "indexBits": 1, "quantizer": {"similarityFunction": "COSINE", "lambda": 0.1, "iters": 5}})
    tv = f.quantizeVectors(list(base))["quantizedVectors"]
    s32 = qs[0][4]
    mask = FC.masks(g["n"])["drop_every_third"]
    spans = [(10, 200), (200, 200), (640, 900)]
    with B.createRowFilter(tv, mask) as flt:
        assert f.searchNearestNeighborsInSpansFiltered(queries[0], tv, [(0, g["n"])], flt, 10) == f.searchNearestNeighborsFiltered(queries[0], tv, flt, 10)
        rows = FC.accepted(mask, spans)
        oi, osc = O.heap_topk(s32[rows], 7)
        got = f.searchNearestNeighborsInSpansFiltered(queries[0], tv, spans, flt, 7)
        assert [r["index"] for r in got] == [int(i) for i in rows[oi]]
        np.testing.assert_array_equal(canon32([r["score"] for r in got]), canon32(osc))
        assert f.searchNearestNeighborsInSpansFiltered(queries[0], tv, [], flt, 7) == []
        assert f.searchNearestNeighborsInSpansFiltered(queries[0], tv, spans, flt, 0) == []
        for bad in (lambda: f.searchNearestNeighborsInSpansFiltered(queries[0], tv, [(5, 3)], flt, 7),
                    lambda: f.searchNearestNeighborsInSpansFiltered(queries[0], tv, None, flt, 7),
                    lambda: f.searchNearestNeighborsInSpansFiltered(queries[0], tv, spans, None, 7),
                    lambda: f.searchNearestNeighborsInSpansFiltered(None, tv, spans, flt, 7),
                    lambda: f.searchNearestNeighborsInSpansFiltered(queries[0], tv, spans, flt, -1),
                    lambda: f.searchNearestNeighborsInSpansFiltered(queries[0], tv, [(0, 10), (5, 20)], flt, 7)):
            with pytest.raises(Exception):
                bad()
