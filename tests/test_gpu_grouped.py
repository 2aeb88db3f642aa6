"""GPU: grouped search - bbq_groups_*, bbq_search_grouped_batch - against the golden per-row scores, the model of
tests/test_groups_cpu.py and the oracle's heap.  Bit-exact: a query's answer is what the reference's loop returns when it visits exactly
the representatives of the live groups, ascending - indices (original ords), score bits, order and groups, ties and NaN included - and
out_status says which path answered, by the span search's rule over the representatives' scores."""
import functools

import numpy as np
import pytest

import orclib as O
import append_recipe as R
import test_gpu_score_ords as SO          # its fixtures and per-row golden arrays (_case: computed once, shared, never written to)
import test_gpu_spans as GS               # its seeded indexes (_synthetic: computed once per call, never written to)
import test_spans_cpu as SC
import test_spans_filtered_cpu as FC      # the masks
import test_groups_cpu as GC              # the layouts and the model
from test_gpu_score_ords import canon32
from bbqlib import bbq_amd as B, capi

pytestmark = pytest.mark.gpu


def assert_grouped(ix, groups, offsets, mask, qqs, qcs, qb, sim, k, scores, msg):
    """one call: every query's answer equals the oracle's heap over the scores of the model's representatives, mapped back to ords and
    groups, and its status equals the rule.  scores[q] = the f32 score of every row of the index for query q.  Returns the answers and
    the statuses"""
    res, status = ix.search_grouped_batch(qqs, qcs, qb, sim, k, groups)
    assert len(res) == len(scores) == len(status)
    for q, s32 in enumerate(scores):
        ords, grp = _reps(s32, offsets, mask)
        assert groups.live == len(ords)
        v = s32[ords]
        oi, osc = O.heap_topk(v, k)
        where = "%s: query %d k=%d" % (msg, q, k)
        np.testing.assert_array_equal(res[q][0], ords[oi], err_msg=where)
        np.testing.assert_array_equal(canon32(res[q][1]), canon32(osc), err_msg=where + ": score bits")
        np.testing.assert_array_equal(res[q][2], grp[oi], err_msg=where + ": groups")
        assert status[q] == SC.expected_status(v, k), "%s: status %d, the rule says %d" % (where, status[q], SC.expected_status(v, k))
    return res, status


_rep_cache = {}


def _reps(s32, offsets, mask):
    """the model's representatives, computed once per (scores, layout, mask) and shared between the calls of a test; read-only"""
    key = (id(s32), id(offsets), id(mask))
    hit = _rep_cache.get(key)
    if hit is None or hit[0] is not s32 or hit[1] is not offsets or hit[2] is not mask:
        hit = (s32, offsets, mask) + GC.representatives(s32, offsets, mask)
        _rep_cache[key] = hit
    return hit[3], hit[4]


def _ks(L):
    return sorted({k for k in (1, L - 1, L, L + 1) if k >= 0})


def _open(ix, offsets, mask):
    """(filter or None, group set): no filter at all where the mask accepts every row"""
    flt = None if mask.all() else capi.Filter(ix, mask)
    try:
        return flt, capi.Groups(ix, offsets, flt)
    except Exception:
        if flt is not None:
            flt.close()
        raise


def _sweep(ix, n, lays, masks, qqs, qcs, qb, sim, scores, name, ks_of=_ks):
    """every layout x mask x k in one index; returns the set of statuses seen"""
    seen = set()
    for lname, off in lays.items():
        for mname, mask in masks.items():
            flt, groups = _open(ix, off, mask)
            try:
                assert groups.count == len(off) - 1 and groups.live == GC.plan(off, mask)[1]
                if flt is not None:
                    flt.close()                                   # the group set keeps its own copy of the filter's words
                    flt = None
                for k in ks_of(groups.live):
                    res, status = assert_grouped(ix, groups, off, mask, qqs, qcs, qb, sim, k, scores, "%s %s %s" % (name, lname, mname))
                    seen |= set(status.tolist())
                    if groups.live == 0:
                        assert all(len(r[0]) == 0 for r in res) and (status == 0).all()
            finally:
                groups.close()
                if flt is not None:
                    flt.close()
    return seen


@pytest.mark.parametrize("compact", [True, False])
@pytest.mark.parametrize("name", SO.FIXTURES)
def test_golden_answers(name, compact):
    """every query of the fixture with every layout and mask that fits its n, k in {1, L - 1, L, L + 1}"""
    g, sim, codes, corr, cdp, qs = SO._case(name)
    n = g["n"]
    qqs, qcs = np.stack([q[0] for q in qs]), np.stack([q[1] for q in qs])
    scores = [q[4] for q in qs]
    ix = B.Index(codes, corr, g["dim"], cdp, index_bits=g["ib"], corrections="compact" if compact else "inline")
    try:
        seen = _sweep(ix, n, GC.layouts(n), FC.masks(n), qqs, qcs, g["qb"], sim, scores, name)
        if name != "edge_dim1" and n > 12:
            assert seen == {0, 1}    # both paths answered
    finally:
        ix.close()


@pytest.mark.parametrize("dim,seed", [(64, 81), (768, 91)])
@pytest.mark.parametrize("compact", [True, False])
def test_chunk_edges(dim, seed, compact):
    """2 100 rows - four chunks and a partial tile - with groups that end at, begin at and cross the chunks' edges, a group over two
    edges and the layouts of the goldens: the segments that leave a tile are merged in LDS, those that leave a chunk by the atomic"""
    n = 2100
    sim, qb, codes, corr, cdp, qq, qc, s32 = GS._synthetic(n, dim, seed)
    lays = dict(GC.chunk_edge_layouts(n))
    lays.update({k: v for k, v in GC.layouts(n).items() if k in ("big_mid_tile", "groups_of_513", "groups_of_65", "random_1_20", "empty_groups", "one_group")})
    masks = {k: v for k, v in FC.masks(n).items() if k in ("all", "random_half", "tile_out_and_ends", "sparse_61")}
    ix = B.Index(codes, corr, dim, cdp, corrections="compact" if compact else "inline")
    try:
        seen = _sweep(ix, n, lays, masks, qq, qc, qb, sim, s32, "2100 x %d" % dim, ks_of=lambda L: sorted({k for k in (1, 3, L - 1, L + 1) if k >= 0}))
        assert seen == {0, 1}
    finally:
        ix.close()


def test_host_path_and_sub_batches():
    """5 000 singletons: k = 4 500 is beyond what the device selects, k = 4 096 is its limit; and 70 queries under 1 MiB of scratch - three
    sub-batches - answer like the same queries under the default"""
    n, dim = 5000, 64
    sim, qb, codes, corr, cdp, qq, qc, s32 = GS._synthetic(n, dim, 83)
    off, mask = GC.layouts(n)["singletons"], FC.masks(n)["all"]
    ix = B.Index(codes, corr, dim, cdp)
    try:
        with capi.Groups(ix, off) as groups:
            assert groups.live == n
            _, status = assert_grouped(ix, groups, off, mask, qq, qc, qb, sim, 4500, s32, "5000 singletons")
            assert (status == 1).all()
            assert_grouped(ix, groups, off, mask, qq, qc, qb, sim, 4096, s32, "5000 singletons")
            who = np.arange(70) % len(qq)
            want, want_status = ix.search_grouped_batch(qq[who], qc[who], qb, sim, 10, groups)
            ix.set_option("group_scratch_mb", 1)
            assert 70 * n * 16 > 2 * (1 << 20)
            got, got_status = ix.search_grouped_batch(qq[who], qc[who], qb, sim, 10, groups)
            ix.set_option("group_scratch_mb", 256)
            np.testing.assert_array_equal(got_status, want_status)
            for a, b, w in zip(got, want, who):
                for x, y in zip(a, b):
                    assert x.tobytes() == y.tobytes()
                oi, osc = O.heap_topk(s32[w], 10)
                np.testing.assert_array_equal(a[0], oi)
    finally:
        ix.close()


@pytest.mark.parametrize("compact", [True, False])
def test_cross_checks(compact):
    """all singletons is the span search over [0, n), under a filter the filtered span search - answers and statuses; one group of all
    rows returns one row, the lowest ord among the best"""
    n, dim = 2100, 64
    sim, qb, codes, corr, cdp, qq, qc, s32 = GS._synthetic(n, dim, 81)
    whole = [SC.spans_of([(0, n)])] * len(qq)
    single = GC.layouts(n)["singletons"]
    ix = B.Index(codes, corr, dim, cdp, corrections="compact" if compact else "inline")
    try:
        with capi.Groups(ix, single) as groups:
            for k in (1, 10, 100, 2099, 2100, 3000):
                res, status = ix.search_grouped_batch(qq, qc, qb, sim, k, groups)
                plain, plain_status = ix.search_spans_batch(qq, qc, qb, sim, k, whole)
                np.testing.assert_array_equal(status, plain_status)
                for q in range(len(qq)):
                    np.testing.assert_array_equal(res[q][0], plain[q][0])
                    np.testing.assert_array_equal(canon32(res[q][1]), canon32(plain[q][1]))
                    np.testing.assert_array_equal(res[q][2], res[q][0])           # a singleton's group is its row
        for mname in ("random_half", "sparse_61", "none"):
            mask = FC.masks(n)[mname]
            with capi.Filter(ix, mask) as flt, capi.Groups(ix, single, flt) as groups:
                for k in (1, 10, 35, 1500):
                    res, status = ix.search_grouped_batch(qq, qc, qb, sim, k, groups)
                    plain, plain_status = ix.search_spans_filtered_batch(qq, qc, qb, sim, k, whole, flt)
                    np.testing.assert_array_equal(status, plain_status)
                    for q in range(len(qq)):
                        np.testing.assert_array_equal(res[q][0], plain[q][0])
                        np.testing.assert_array_equal(canon32(res[q][1]), canon32(plain[q][1]))
        with capi.Groups(ix, [0, n]) as groups:
            assert groups.count == 1 and groups.live == 1
            for k in (1, 5):
                res, status = ix.search_grouped_batch(qq, qc, qb, sim, k, groups)
                assert (status == 1).all()                                        # L <= k
                for q in range(len(qq)):
                    best = int(np.flatnonzero(s32[q] == s32[q].max())[0])
                    assert res[q][0].tolist() == [best] and res[q][2].tolist() == [0]
                    assert canon32(res[q][1])[0] == canon32(s32[q][best:best + 1])[0]
    finally:
        ix.close()


@functools.lru_cache(maxsize=None)
def _tie_case():
    """2 100 x 64 rows with duplicated rows: the rows [90, 140) are copies of row 100, and the rows [200, 210) and [700, 710) are copies
    of query 0's best row"""
    n, dim = 2100, 64
    sim, qb, codes, corr, cdp, qq, qc, s32 = GS._synthetic(n, dim, 84)
    codes, corr = codes.copy(), corr.copy()
    best = int(np.argmax(s32[0]))
    assert not (90 <= best < 140)
    codes[90:140], corr[90:140] = codes[100], corr[100]
    for b in (200, 700):
        codes[b:b + 10], corr[b:b + 10] = codes[best], corr[best]
    s32 = [O.score_all(codes, corr, dim, qq[i], qc[i], qb, sim, cdp)[2] for i in range(len(qq))]
    for a in (codes, corr):
        a.setflags(write=False)
    return n, dim, sim, qb, codes, corr, cdp, qq, qc, s32, best


@pytest.mark.parametrize("compact", [True, False])
def test_ties(compact):
    n, dim, sim, qb, codes, corr, cdp, qq, qc, s32, best = _tie_case()
    everything = FC.masks(n)["all"]
    inside = np.array([0, 64, 90, 140, 200, 210, 700, 710, n], np.int64)           # each run of copies is one group
    ix = B.Index(codes, corr, dim, cdp, corrections="compact" if compact else "inline")
    try:
        with capi.Groups(ix, inside) as groups:
            for k in (1, 2, 3, 8):
                res, status = assert_grouped(ix, groups, inside, everything, qq, qc, qb, sim, k, s32, "ties")
                assert status[0] == 1                                              # query 0: the two best representatives are equal
                assert canon32(res[0][1][:1])[0] == canon32(s32[0][best:best + 1])[0]
            res, _ = ix.search_grouped_batch(qq, qc, qb, sim, 8, groups)
            for q in range(len(qq)):                                               # the lowest ord of a group of equal rows represents it
                rows = dict(zip(res[q][2].tolist(), res[q][0].tolist()))
                assert rows[2] == 90 and rows[4] == 200 and rows[6] == 700
        with capi.Filter(ix, FC.masks(n)["drop_every_third"]) as flt, capi.Groups(ix, inside, flt) as groups:
            res, _ = assert_grouped(ix, groups, inside, FC.masks(n)["drop_every_third"], qq, qc, qb, sim, 8, s32, "ties, filtered")
            rows = dict(zip(res[1][2].tolist(), res[1][0].tolist()))
            assert rows[2] == 90 and rows[4] == 200 and rows[6] == 701             # the rows 1, 4, 7, ... are rejected: 700 is one of them
    finally:
        ix.close()


N_NAN, DIM_NAN, NAN_ROW = 200, 64, 77
NAN_KS = (1, 5, 10)
NAN_TENS = np.arange(0, N_NAN + 1, 10, dtype=np.int64)        # row 77 lies in the group [70, 80)
NAN_SINGLE = np.arange(N_NAN + 1, dtype=np.int64)
NAN_EVERYTHING = np.ones(N_NAN, bool)


@functools.lru_cache(maxsize=None)
def _nan_case():
    """200 x 64 rows as bbq_index_create takes them, row 77's additive correction set to NaN: exactly that row scores NaN.  The seed is
    the first for which the rule gives status 0 for every query and k of the test over the representatives of the groups of ten"""
    sim, qb = 1, 4
    for seed in range(500, 540):
        rng = np.random.default_rng(seed)
        base = rng.standard_normal((N_NAN, DIM_NAN)).astype(np.float32)
        queries = rng.standard_normal((3, DIM_NAN)).astype(np.float32)
        codes, corr, cen = B.quantize_vectors(base, sim)
        corr = corr.copy()
        corr[NAN_ROW, 2] = np.nan
        cdp = B.centroid_dp(cen)
        qq, qc = B.quantize_queries(queries, cen, sim, qb)
        s32 = [O.score_all(codes, corr, DIM_NAN, qq[i], qc[i], qb, sim, cdp)[2] for i in range(3)]
        if all(SC.expected_status(s[GC.representatives(s, NAN_TENS, NAN_EVERYTHING)[0]], k) == 0 for s in s32 for k in NAN_KS):
            break
    else:
        raise AssertionError("no seed without equal scores among the largest representatives")
    for s in s32:
        assert np.isnan(s[NAN_ROW]) and np.isnan(s).sum() == 1
    for a in (codes, corr):
        a.setflags(write=False)
    return sim, qb, codes, corr, cdp, qq, qc, s32


@pytest.mark.parametrize("compact", [True, False])
def test_nan(compact):
    """a NaN score inside a larger group never represents and changes no status; as a singleton group it represents with NaN and sends
    its query to the heap"""
    sim, qb, codes, corr, cdp, qq, qc, s32 = _nan_case()
    ix = B.Index(codes, corr, DIM_NAN, cdp, corrections="compact" if compact else "inline")
    try:
        with capi.Groups(ix, NAN_TENS) as tens, capi.Groups(ix, NAN_SINGLE) as single:
            for k in NAN_KS:
                res, status = assert_grouped(ix, tens, NAN_TENS, NAN_EVERYTHING, qq, qc, qb, sim, k, s32, "NaN inside a group")
                assert (status == 0).all() and all(NAN_ROW not in r[0] for r in res)
                _, status = assert_grouped(ix, single, NAN_SINGLE, NAN_EVERYTHING, qq, qc, qb, sim, k, s32, "NaN as a group")
                assert (status == 1).all()
            res, _ = assert_grouped(ix, tens, NAN_TENS, NAN_EVERYTHING, qq, qc, qb, sim, 20, s32, "every group of ten")
            assert all(NAN_ROW not in r[0] and 7 in r[2] for r in res)
            res, _ = assert_grouped(ix, single, NAN_SINGLE, NAN_EVERYTHING, qq, qc, qb, sim, N_NAN, s32, "every row")
            assert all(NAN_ROW in r[0] for r in res)
        only = np.zeros(N_NAN, bool)
        only[[NAN_ROW, 150]] = True                               # the group [70, 80) has the NaN row alone: it represents, with NaN
        with capi.Filter(ix, only) as flt, capi.Groups(ix, NAN_TENS, flt) as groups:
            assert groups.live == 2
            res, status = assert_grouped(ix, groups, NAN_TENS, only, qq, qc, qb, sim, 1, s32, "a group of NaN alone")
            assert (status == 1).all()
            res, _ = assert_grouped(ix, groups, NAN_TENS, only, qq, qc, qb, sim, 2, s32, "a group of NaN alone")
            assert all(sorted(r[0].tolist()) == [NAN_ROW, 150] for r in res)
    finally:
        ix.close()


def test_two_calls_give_identical_bytes():
    n, dim = 2100, 64
    sim, qb, codes, corr, cdp, qq, qc, s32 = GS._synthetic(n, dim, 81)
    off = GC.chunk_edge_layouts(n)["around_chunk_edges"]
    ix = B.Index(codes, corr, dim, cdp)
    try:
        with capi.Filter(ix, FC.masks(n)["random_half"]) as flt, capi.Groups(ix, off, flt) as groups:
            for k in (3, 40):
                a, sa = ix.search_grouped_batch(qq, qc, qb, sim, k, groups)
                b, sb = ix.search_grouped_batch(qq, qc, qb, sim, k, groups)
                assert sa.tobytes() == sb.tobytes()
                for x, y in zip(a, b):
                    assert all(u.tobytes() == v.tobytes() for u, v in zip(x, y))
    finally:
        ix.close()


def _raw(L, handle, groups, g, sim, qq, qc, k):
    """the C entry point with prefilled outputs: (rc, message, outputs untouched)"""
    idx, grp, sc = np.full(2 * max(k, 1), -7, np.int32), np.full(2 * max(k, 1), -7, np.int32), np.full(2 * max(k, 1), -7.0, np.float32)
    cnt, st = np.full(2, -7, np.int64), np.full(2, 7, np.uint8)
    rc = L.bbq_search_grouped_batch(handle._h, None if groups is None else groups._h, 2, qq.ctypes.data, qc.ctypes.data, g["qb"], sim, k,
                                    idx.ctypes.data, grp.ctypes.data, sc.ctypes.data, cnt.ctypes.data, st.ctypes.data)
    untouched = (idx == -7).all() and (grp == -7).all() and (sc == -7.0).all() and (cnt == -7).all() and (st == 7).all()
    return rc, L.bbq_last_error().decode("utf-8"), untouched


def test_refusals_and_mutations():
    g, sim, codes, corr, cdp, qs = SO._case("c1_1000x128_cos_qb4")
    n = g["n"]
    base, _ = O.golden_inputs(g)
    cen = B.quantize_vectors(base, sim, g["ib"], g["lambda"], g["iters"])[2]
    rng = np.random.default_rng(89)
    new_codes, new_corr = R.oracle_rows(rng.standard_normal((104, g["dim"])).astype(np.float32), cen, sim, g["ib"], g["lambda"], g["iters"])
    qqs, qcs = np.stack([q[0] for q in qs[:2]]), np.stack([q[1] for q in qs[:2]])
    off = GC.layouts(n)["random_1_20"]
    everything = FC.masks(n)["all"]
    L = capi.lib()
    ix = B.Index(codes, corr, g["dim"], cdp)
    other = B.Index(codes[:900], corr[:900], g["dim"], cdp)
    multi = B.Index.create_multi(codes, corr, g["dim"], cdp, [0, 0], pilot_rows=0)
    groups = capi.Groups(ix, off)
    try:
        rc, _, untouched = _raw(L, ix, groups, g, sim, qqs, qcs, 5)
        assert rc == capi.OK and not untouched
        rc, msg, untouched = _raw(L, ix, groups, g, sim, qqs, qcs, -1)
        assert rc == capi.ERR_NEGATIVE_K and untouched
        rc, msg, untouched = _raw(L, ix, None, g, sim, qqs, qcs, 5)
        assert rc == capi.ERR_INVALID_ARG and untouched
        rc, msg, untouched = _raw(L, other, groups, g, sim, qqs, qcs, 5)               # a group set of an index of another size
        assert rc == capi.ERR_INVALID_ARG and "1000" in msg and "900" in msg and untouched, msg
        rc, msg, untouched = _raw(L, multi, groups, g, sim, qqs, qcs, 5)
        assert rc == capi.ERR_UNSUPPORTED and "multi-device" in msg and untouched
        with pytest.raises(capi.BBQError) as e:
            capi.Groups(multi, off)
        assert e.value.code == capi.ERR_UNSUPPORTED
        for bad in ([1, 500, n], [0, 600, 500, n], [0, 500, n - 1], [0, 500, n + 1], [0, 500]):
            with pytest.raises(capi.BBQError) as e:
                capi.Groups(ix, bad)
            assert e.value.code == capi.ERR_INVALID_ARG and "bbq_groups_create" in str(e.value)
        with capi.Filter(other, FC.masks(900)["random_half"]) as flt_other, pytest.raises(capi.BBQError) as e:
            capi.Groups(ix, off, flt_other)
        assert e.value.code == capi.ERR_INVALID_ARG and "filter" in str(e.value)
        # nothing to answer is no error: no queries, k == 0, no live group
        assert L.bbq_search_grouped_batch(ix._h, groups._h, 0, None, None, g["qb"], sim, 5, None, None, None, None, None) == capi.OK
        res, status = ix.search_grouped_batch(qqs, qcs, g["qb"], sim, 0, groups)
        assert all(len(r[0]) == 0 for r in res) and (status == 0).all()
        with capi.Filter(ix, np.zeros(n, bool)) as nothing, capi.Groups(ix, off, nothing) as dead:
            assert dead.live == 0 and dead.count == len(off) - 1
            res, status = ix.search_grouped_batch(qqs, qcs, g["qb"], sim, 5, dead)
            assert all(len(r[0]) == 0 for r in res) and (status == 0).all()
        # out_group may be null
        idx, sc, cnt = np.zeros(10, np.int32), np.zeros(10, np.float32), np.zeros(2, np.int64)
        assert L.bbq_search_grouped_batch(ix._h, groups._h, 2, qqs.ctypes.data, qcs.ctypes.data, g["qb"], sim, 5, idx.ctypes.data, None, sc.ctypes.data,
                                          cnt.ctypes.data, None) == capi.OK
        want, _ = ix.search_grouped_batch(qqs, qcs, g["qb"], sim, 5, groups)
        assert cnt.tolist() == [5, 5] and idx[:5].tolist() == want[0][0].tolist() and idx[5:].tolist() == want[1][0].tolist()

        # an update in place: the group set still serves and the answers follow the rows as they then are
        ix.update_rows(np.array([0, 511, 512, 999], np.int32), new_codes[100:104], new_corr[100:104])
        now = [ix.score_rows(qq, qc, g["qb"], sim)[2] for qq, qc in zip(qqs, qcs)]
        assert_grouped(ix, groups, off, everything, qqs, qcs, g["qb"], sim, 7, now, "after the update")
        # an append: refused with nothing written, and a new group set serves
        ix.append_rows(new_codes[:100], new_corr[:100])
        assert ix.n == 1100
        rc, msg, untouched = _raw(L, ix, groups, g, sim, qqs, qcs, 5)
        assert rc == capi.ERR_INVALID_ARG and "group set" in msg and untouched, msg
        off2 = np.concatenate([off, [1040, 1100]]).astype(np.int64)
        now = [ix.score_rows(qq, qc, g["qb"], sim)[2] for qq, qc in zip(qqs, qcs)]
        with capi.Groups(ix, off2) as groups2:
            assert_grouped(ix, groups2, off2, np.ones(1100, bool), qqs, qcs, g["qb"], sim, 7, now, "after the append")
    finally:
        groups.close()
        ix.close()
        other.close()
        multi.close()


def test_python_api():
    """api.py: createRowGroups and searchNearestNeighborsGrouped"""
    g, sim, codes, corr, cdp, qs = SO._case("c1_1000x128_cos_qb4")
    base, queries = O.golden_inputs(g)
    f = B.createBinaryQuantizationFormat({"queryBits": 4, "indexBits": 1, "quantizer": {"similarityFunction": "COSINE", "lambda": 0.1, "iters": 5}})
    tv = f.quantizeVectors(list(base))["quantizedVectors"]
    s32 = qs[0][4]
    n = g["n"]
    off = GC.layouts(n)["random_1_20"]
    mask = FC.masks(n)["drop_every_third"]
    with B.createRowFilter(tv, mask) as flt, B.createRowGroups(tv, off, flt) as groups, B.createRowGroups(tv, off) as unfiltered:
        assert groups.count == len(off) - 1 and groups.live == GC.plan(off, mask)[1] and unfiltered.live == len(off) - 1
        for grp, m in ((groups, mask), (unfiltered, FC.masks(n)["all"])):
            ords, gids = GC.representatives(s32, off, m)
            oi, osc = O.heap_topk(s32[ords], 7)
            got = f.searchNearestNeighborsGrouped(queries[0], tv, grp, 7)
            assert [r["index"] for r in got] == [int(i) for i in ords[oi]] and [r["group"] for r in got] == [int(i) for i in gids[oi]]
            np.testing.assert_array_equal(canon32([r["score"] for r in got]), canon32(osc))
        assert f.searchNearestNeighborsGrouped(queries[0], tv, groups, 0) == []
        for bad in (lambda: f.searchNearestNeighborsGrouped(queries[0], tv, None, 7),
                    lambda: f.searchNearestNeighborsGrouped(None, tv, groups, 7),
                    lambda: f.searchNearestNeighborsGrouped(queries[0], tv, groups, -1),
                    lambda: f.searchNearestNeighborsGrouped(queries[0][:5], tv, groups, 7),
                    lambda: B.createRowGroups(tv, [0, 5, 3, n]),
                    lambda: B.createRowGroups(tv, None)):
            with pytest.raises(Exception):
                bad()
