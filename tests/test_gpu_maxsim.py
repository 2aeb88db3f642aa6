"""GPU: MaxSim search - bbq_search_maxsim_batch - against the model of tests/maxsim_model.py, bit for bit: a query's answer is what the
reference's loop returns when it visits the live groups, ascending, each with the ordered f64 sum of its per-token representatives'
scores - group numbers, score bits, order, out_n - and out_status is the span search's rule over the sums.  Every case runs under both
values of maxsim_fused: at 768 dimensions 1 is the fused kernel, at 64 both are the grouped search's score kernel."""
import functools

import numpy as np
import pytest

import orclib as O
import append_recipe as R
import maxsim_model as M
import test_gpu_score_ords as SO          # its fixtures and per-row golden arrays (_case: computed once, shared, never written to)
import test_gpu_spans as GS               # its seeded indexes (_synthetic: computed once per call, never written to)
import test_spans_filtered_cpu as FC      # the masks
import test_groups_cpu as GC              # the layouts
from test_gpu_score_ords import canon32
from bbqlib import bbq_amd as B, capi

pytestmark = pytest.mark.gpu

N = 1300                                  # three chunks of 512 rows, the last tile partial
FUSED = (0, 1)


@functools.lru_cache(maxsize=None)
def _tb():
    return capi.maxsim_token_block()


def _token_counts():
    tb = _tb()
    return (1, 2, tb - 1, tb, tb + 1, 2 * tb + 3)


@functools.lru_cache(maxsize=None)
def _vectors(dim):
    """1 300 rows and as many token vectors as one query of every token count needs, with every vector's per-row oracle scores"""
    return GS._synthetic(N, dim, 93 if dim == 64 else 97, nq=sum(_token_counts()))


def _queries(counts):
    """queries of `counts` token vectors each, cut from the front of the vectors: [(first, last)]"""
    cuts = np.concatenate([[0], np.cumsum(counts)])
    return [(int(a), int(b)) for a, b in zip(cuts[:-1], cuts[1:])]


def _layouts():
    lays = {k: v for k, v in GC.layouts(N).items() if k in ("singletons", "one_group", "groups_of_64", "groups_of_65", "random_1_20", "empty_groups")}
    lays.update(GC.chunk_edge_layouts(N))          # across_two_edges: [500, 1300) - a whole chunk and both its neighbours
    return lays


_rep_cache = {}


def _reps(tag, s32, off, mask, lname, mname):
    """the model's representative scores [vectors, L] and live groups of one (index, layout, mask): computed once, read-only"""
    key = (tag, lname, mname)
    if key not in _rep_cache:
        rep, groups = M.rep_scores(s32, off, mask)
        rep.setflags(write=False)
        _rep_cache[key] = (rep, groups)
    return _rep_cache[key]


def _want(rep, groups, spans, k):
    out = []
    for a, b in spans:
        S = M.reduce(rep[a:b]) if len(groups) else np.zeros(0, np.float32)
        oi, osc = O.heap_topk(S, k)
        out.append((groups[oi].astype(np.int32), osc, M.SC.expected_status(S, k)))
    return out


def _call(ix, groups, qq, qc, spans, qb, sim, k):
    return ix.search_maxsim_batch([(qq[a:b], qc[a:b]) for a, b in spans], qb, sim, k, groups)


def assert_maxsim(ix, groups, rep, live_groups, qq, qc, spans, qb, sim, k, msg):
    """one call under each value of maxsim_fused: every query's groups, score bits, order and count equal the model's and its status the
    rule's; the two values give the same bytes.  Returns the answers and the statuses"""
    want = _want(rep, live_groups, spans, k)
    assert groups.live == len(live_groups)
    seen = []
    for fused in FUSED:
        ix.set_option("maxsim_fused", fused)
        res, status = _call(ix, groups, qq, qc, spans, qb, sim, k)
        assert len(res) == len(want) == len(status)
        for q, (wg, ws, wst) in enumerate(want):
            where = "%s: fused=%d query %d (%d tokens) k=%d" % (msg, fused, q, spans[q][1] - spans[q][0], k)
            np.testing.assert_array_equal(res[q][0], wg, err_msg=where + ": groups")
            np.testing.assert_array_equal(canon32(res[q][1]), canon32(ws), err_msg=where + ": score bits")
            assert status[q] == wst, "%s: status %d, the rule says %d" % (where, status[q], wst)
        seen.append((res, status))
    ix.set_option("maxsim_fused", -1)
    (a, sa), (b, sb) = seen
    assert sa.tobytes() == sb.tobytes()
    for x, y in zip(a, b):
        assert all(u.tobytes() == v.tobytes() for u, v in zip(x, y)), msg + ": the two score paths differ"
    return seen[0]


def _open(ix, off, mask):
    if mask.all():
        return capi.Groups(ix, off)
    with capi.Filter(ix, mask) as flt:            # the group set keeps its own copy of the filter's words
        return capi.Groups(ix, off, flt)


@pytest.mark.parametrize("dim", [64, 768])
@pytest.mark.parametrize("compact", [True, False])
def test_edges_filters_and_token_counts(dim, compact):
    """every layout without a filter, three of them under a random half and under a mask that rejects a whole tile - rows 64..127, which
    is all of group 1 of groups_of_64 - and a whole singleton group; one call holds a query of every token count"""
    sim, qb, codes, corr, cdp, qq, qc, s32 = _vectors(dim)
    spans = _queries(_token_counts())
    masks = FC.masks(N)
    cases = [(l, "all") for l in _layouts()] + [(l, m) for l in ("groups_of_64", "singletons", "around_chunk_edges") for m in ("random_half", "tile_out_and_ends")]
    ix = B.Index(codes, corr, dim, cdp, corrections="compact" if compact else "inline")
    statuses = set()
    try:
        for lname, mname in cases:
            off, mask = _layouts()[lname], masks[mname]
            rep, live = _reps(dim, s32, off, mask, lname, mname)
            with _open(ix, off, mask) as groups:
                for k in (3, 40):
                    _, st = assert_maxsim(ix, groups, rep, live, qq, qc, spans, qb, sim, k, "%d %s %s" % (dim, lname, mname))
                    statuses |= set(st.tolist())
        assert statuses == {0, 1}                 # both paths answered
    finally:
        ix.close()


@pytest.mark.parametrize("dim", [64, 768])
def test_each_token_count_alone(dim):
    sim, qb, codes, corr, cdp, qq, qc, s32 = _vectors(dim)
    off, mask = _layouts()["around_chunk_edges"], FC.masks(N)["all"]
    rep, live = _reps(dim, s32, off, mask, "around_chunk_edges", "all")
    ix = B.Index(codes, corr, dim, cdp)
    try:
        with capi.Groups(ix, off) as groups:
            for T in _token_counts():
                assert_maxsim(ix, groups, rep, live, qq, qc, [(0, T)], qb, sim, 4, "%d alone T=%d" % (dim, T))
    finally:
        ix.close()


@pytest.mark.parametrize("dim", [64, 768])
@pytest.mark.parametrize("compact", [True, False])
def test_one_token_is_the_grouped_search(dim, compact):
    sim, qb, codes, corr, cdp, qq, qc, s32 = _vectors(dim)
    masks = FC.masks(N)
    ix = B.Index(codes, corr, dim, cdp, corrections="compact" if compact else "inline")
    try:
        for lname, mname in (("random_1_20", "all"), ("around_chunk_edges", "random_half"), ("one_group", "all")):
            with _open(ix, _layouts()[lname], masks[mname]) as groups:
                for k in (1, 5, groups.live, groups.live + 1):
                    want, want_status = ix.search_grouped_batch(qq[:6], qc[:6], qb, sim, k, groups)
                    for fused in FUSED:
                        ix.set_option("maxsim_fused", fused)
                        got, status = _call(ix, groups, qq, qc, [(i, i + 1) for i in range(6)], qb, sim, k)
                        np.testing.assert_array_equal(status, want_status)
                        for q in range(6):
                            np.testing.assert_array_equal(got[q][0], want[q][2])
                            assert got[q][1].tobytes() == want[q][1].tobytes()
                    ix.set_option("maxsim_fused", -1)
    finally:
        ix.close()


@functools.lru_cache(maxsize=None)
def _tie_case(dim):
    """the rows [200, 210) and [700, 710) are copies of one row, as in test_gpu_grouped._tie_case: the groups that are exactly those
    runs have equal representatives for every token, and so equal sums"""
    sim, qb, codes, corr, cdp, qq, qc, _ = _vectors(dim)
    codes, corr = codes.copy(), corr.copy()
    best = int(np.argmax(_vectors(dim)[7][0]))
    for b in (200, 700):
        codes[b:b + 10], corr[b:b + 10] = codes[best], corr[best]
    s32 = [O.score_all(codes, corr, dim, qq[i], qc[i], qb, sim, cdp)[2] for i in range(5)]
    for a in (codes, corr):
        a.setflags(write=False)
    return codes, corr, s32


@pytest.mark.parametrize("dim", [64, 768])
def test_ties(dim):
    sim, qb, _, _, cdp, qq, qc, _ = _vectors(dim)
    codes, corr, s32 = _tie_case(dim)
    off = np.array([0, 64, 200, 210, 700, 710, N], np.int64)              # each run of copies is one group: 2 and 4
    rep, live = M.rep_scores(s32, off, np.ones(N, bool))
    S = M.reduce(rep)
    assert S[2].tobytes() == S[4].tobytes()
    ix = B.Index(codes, corr, dim, cdp)
    try:
        with capi.Groups(ix, off) as groups:
            for k in (1, 2, 5):
                res, status = assert_maxsim(ix, groups, rep, live, qq, qc, [(0, 5), (0, 1)], qb, sim, k, "ties %d" % dim)
                assert status[1] == 1                                      # one token, the duplicated row its best: the two best sums are equal
            res, status = assert_maxsim(ix, groups, rep, live, qq, qc, [(0, 5)], qb, sim, 5, "ties %d, all but one" % dim)
            assert status[0] == 1                                          # k + 1 = L: the equal pair is among them; the order is the model's heap's
    finally:
        ix.close()


@functools.lru_cache(maxsize=None)
def _nan_case(dim):
    """row 77's additive correction set to NaN, as in test_gpu_grouped._nan_case: exactly that row scores NaN, for every token"""
    sim, qb, codes, corr, cdp, qq, qc, _ = _vectors(dim)
    corr = corr.copy()
    corr[77, 2] = np.nan
    s32 = [O.score_all(codes, corr, dim, qq[i], qc[i], qb, sim, cdp)[2] for i in range(4)]
    for s in s32:
        assert np.isnan(s[77]) and np.isnan(s).sum() == 1
    corr.setflags(write=False)
    return corr, s32


@pytest.mark.parametrize("dim", [64, 768])
@pytest.mark.parametrize("compact", [True, False])
def test_nan(dim, compact):
    """a NaN row inside a larger group never represents: no sum is NaN; as a singleton - or the only accepted row of its group - its
    group's sum is NaN, the query goes to the heap and the group stands where the reference puts it"""
    sim, qb, codes, _, cdp, qq, qc, _ = _vectors(dim)
    corr, s32 = _nan_case(dim)
    everything = np.ones(N, bool)
    tens, single = GC._tiled(N, 10), GC.layouts(N)["singletons"]
    ix = B.Index(codes, corr, dim, cdp, corrections="compact" if compact else "inline")
    try:
        with capi.Groups(ix, tens) as groups:
            rep, live = M.rep_scores(s32, tens, everything)
            assert not np.isnan(M.reduce(rep)).any()
            for k in (1, 10, len(live)):
                assert_maxsim(ix, groups, rep, live, qq, qc, [(0, 4), (1, 2)], qb, sim, k, "NaN inside a group")
        with capi.Groups(ix, single) as groups:
            rep, live = M.rep_scores(s32, single, everything)
            assert np.isnan(M.reduce(rep)).sum() == 1
            for k in (1, 10, N):
                res, status = assert_maxsim(ix, groups, rep, live, qq, qc, [(0, 4), (1, 2)], qb, sim, k, "NaN as a group")
                assert (status == 1).all()
            assert all(77 in r[0] for r in res)
        only = np.zeros(N, bool)
        only[[77, 150, 900]] = True                                         # the group [70, 80) has the NaN row alone
        with capi.Filter(ix, only) as flt, capi.Groups(ix, tens, flt) as groups:
            rep, live = M.rep_scores(s32, tens, only)
            assert groups.live == 3 and np.isnan(M.reduce(rep)).sum() == 1
            for k in (1, 2, 3):
                res, status = assert_maxsim(ix, groups, rep, live, qq, qc, [(0, 4)], qb, sim, k, "a group of NaN alone")
                assert (status == 1).all()
    finally:
        ix.close()


@pytest.mark.parametrize("dim", [64, 768])
def test_k(dim):
    sim, qb, codes, corr, cdp, qq, qc, s32 = _vectors(dim)
    off, mask = _layouts()["random_1_20"], FC.masks(N)["all"]
    rep, live = _reps(dim, s32, off, mask, "random_1_20", "all")
    L = len(live)
    ix = B.Index(codes, corr, dim, cdp)
    try:
        with capi.Groups(ix, off) as groups:
            for k in (0, 1, L - 1, L, L + 1, 4097):
                res, status = assert_maxsim(ix, groups, rep, live, qq, qc, [(0, 3), (3, 4)], qb, sim, k, "k")
                assert all(len(r[0]) == min(k, L) for r in res)
                if k == 0:
                    assert (status == 0).all()
            with pytest.raises(capi.BBQError) as e:
                _call(ix, groups, qq, qc, [(0, 3)], qb, sim, -1)
            assert e.value.code == capi.ERR_NEGATIVE_K
    finally:
        ix.close()


def test_sub_batches_and_token_blocks():
    """1 300 singletons under 1 MiB of scratch: two queries per sub-batch, and the longest query takes three token blocks; the same
    bytes as under the default"""
    dim = 768
    sim, qb, codes, corr, cdp, qq, qc, s32 = _vectors(dim)
    off = GC.layouts(N)["singletons"]
    spans = _queries(_token_counts())
    assert 3 * (8 * _tb() + 16) * N > (1 << 20) >= 2 * (8 * _tb() + 16) * N and len(spans) > 4
    ix = B.Index(codes, corr, dim, cdp)
    try:
        with capi.Groups(ix, off) as groups:
            for fused in FUSED:
                ix.set_option("maxsim_fused", fused)
                want, want_status = _call(ix, groups, qq, qc, spans, qb, sim, 10)
                ix.set_option("group_scratch_mb", 1)
                got, got_status = _call(ix, groups, qq, qc, spans, qb, sim, 10)
                ix.set_option("group_scratch_mb", 256)
                assert got_status.tobytes() == want_status.tobytes()
                for a, b in zip(got, want):
                    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
            rep, live = _reps(dim, s32, off, FC.masks(N)["all"], "singletons", "all")
            ix.set_option("group_scratch_mb", 1)
            assert_maxsim(ix, groups, rep, live, qq, qc, spans, qb, sim, 10, "1 MiB of scratch")
    finally:
        ix.close()


@pytest.mark.parametrize("dim", [64, 768])
def test_two_calls_give_identical_bytes(dim):
    sim, qb, codes, corr, cdp, qq, qc, s32 = _vectors(dim)
    spans = _queries(_token_counts())
    ix = B.Index(codes, corr, dim, cdp)
    try:
        with capi.Filter(ix, FC.masks(N)["random_half"]) as flt, capi.Groups(ix, _layouts()["around_chunk_edges"], flt) as groups:
            for k in (3, 8):
                runs = []
                for fused in (0, 0, 1, 1):
                    ix.set_option("maxsim_fused", fused)
                    res, st = _call(ix, groups, qq, qc, spans, qb, sim, k)
                    runs.append(st.tobytes() + b"".join(x.tobytes() for r in res for x in r))
                assert runs[0] == runs[1] == runs[2] == runs[3]
    finally:
        ix.close()


def _raw(L, handle, groups, off, qq, qc, qb, sim, k):
    """the C entry point with prefilled outputs: (rc, message, outputs untouched)"""
    off = np.ascontiguousarray(off, np.int64)
    nq = len(off) - 1
    grp, sc = np.full(nq * max(k, 1), -7, np.int32), np.full(nq * max(k, 1), -7.0, np.float32)
    cnt, st = np.full(nq, -7, np.int64), np.full(nq, 7, np.uint8)
    rc = L.bbq_search_maxsim_batch(handle._h, None if groups is None else groups._h, nq, off.ctypes.data, qq.ctypes.data, qc.ctypes.data, qb, sim, k,
                                   grp.ctypes.data, sc.ctypes.data, cnt.ctypes.data, st.ctypes.data)
    untouched = (grp == -7).all() and (sc == -7.0).all() and (cnt == -7).all() and (st == 7).all()
    return rc, L.bbq_last_error().decode("utf-8"), untouched


def test_refusals():
    g, sim, codes, corr, cdp, qs = SO._case("c1_1000x128_cos_qb4")
    n, qb = g["n"], g["qb"]
    base, _ = O.golden_inputs(g)
    cen = B.quantize_vectors(base, sim, g["ib"], g["lambda"], g["iters"])[2]
    rng = np.random.default_rng(89)
    new_codes, new_corr = R.oracle_rows(rng.standard_normal((100, g["dim"])).astype(np.float32), cen, sim, g["ib"], g["lambda"], g["iters"])
    reps = [qs[i % len(qs)] for i in range(6)]
    qq, qc = np.ascontiguousarray(np.stack([q[0] for q in reps])), np.ascontiguousarray(np.stack([q[1] for q in reps]))
    off = GC.layouts(n)["random_1_20"]
    L = capi.lib()
    ix = B.Index(codes, corr, g["dim"], cdp)
    multi = B.Index.create_multi(codes, corr, g["dim"], cdp, [0, 0], pilot_rows=0)
    groups = capi.Groups(ix, off)
    try:
        rc, _, untouched = _raw(L, ix, groups, [0, 2, 6], qq, qc, qb, sim, 5)
        assert rc == capi.OK and not untouched
        for bad, word in (([1, 2, 6], "query 0"),          # not starting at 0
                          ([0, 4, 2, 6], "query 1"),       # descending
                          ([0, 2, 2, 6], "query 1"),       # a query without vectors
                          ([0, 2, 6, 6], "query 2")):
            rc, msg, untouched = _raw(L, ix, groups, bad, qq, qc, qb, sim, 5)
            assert rc == capi.ERR_INVALID_ARG and word in msg and untouched, (bad, msg)
        rc, msg, untouched = _raw(L, ix, groups, [0, 2, 6], qq, qc, qb, sim, -1)
        assert rc == capi.ERR_NEGATIVE_K and untouched
        rc, msg, untouched = _raw(L, ix, None, [0, 2, 6], qq, qc, qb, sim, 5)
        assert rc == capi.ERR_INVALID_ARG and untouched
        rc, msg, untouched = _raw(L, multi, groups, [0, 2, 6], qq, qc, qb, sim, 5)
        assert rc == capi.ERR_UNSUPPORTED and "multi-device" in msg and untouched
        # nothing to answer is no error: no queries, k == 0
        assert L.bbq_search_maxsim_batch(ix._h, groups._h, 0, None, None, None, qb, sim, 5, None, None, None, None) == capi.OK
        res, status = ix.search_maxsim_batch([(qq[:2], qc[:2])], qb, sim, 0, groups)
        assert len(res[0][0]) == 0 and (status == 0).all()
        with capi.Filter(ix, np.zeros(n, bool)) as nothing, capi.Groups(ix, off, nothing) as dead:
            res, status = ix.search_maxsim_batch([(qq[:2], qc[:2])], qb, sim, 5, dead)
            assert len(res[0][0]) == 0 and (status == 0).all()
        # an append: refused with nothing written
        ix.append_rows(new_codes, new_corr)
        rc, msg, untouched = _raw(L, ix, groups, [0, 2, 6], qq, qc, qb, sim, 5)
        assert rc == capi.ERR_INVALID_ARG and "group set" in msg and untouched, msg
    finally:
        groups.close()
        ix.close()
        multi.close()


def test_python_api():
    """api.py: searchNearestNeighborsMaxSim on the README-sized case"""
    g, sim, codes, corr, cdp, qs = SO._case("c1_1000x128_cos_qb4")
    base, queries = O.golden_inputs(g)
    f = B.createBinaryQuantizationFormat({"queryBits": 4, "indexBits": 1, "quantizer": {"similarityFunction": "COSINE", "lambda": 0.1, "iters": 5}})
    tv = f.quantizeVectors(list(base))["quantizedVectors"]
    n = g["n"]
    T = min(len(qs), 5)
    s32 = [qs[i][4] for i in range(T)]
    off = GC.layouts(n)["random_1_20"]
    mask = FC.masks(n)["drop_every_third"]
    with B.createRowFilter(tv, mask) as flt, B.createRowGroups(tv, off, flt) as groups, B.createRowGroups(tv, off) as unfiltered:
        for grp, m in ((groups, mask), (unfiltered, FC.masks(n)["all"])):
            wg, ws, _, _ = M.answer(s32, off, m, 7)
            got = f.searchNearestNeighborsMaxSim([queries[i] for i in range(T)], tv, grp, 7)
            assert [r["group"] for r in got] == [int(i) for i in wg]
            np.testing.assert_array_equal(canon32([r["score"] for r in got]), canon32(ws))
        assert f.searchNearestNeighborsMaxSim([queries[0]], tv, groups, 0) == []
        one = f.searchNearestNeighborsMaxSim([queries[0]], tv, groups, 7)
        same = f.searchNearestNeighborsGrouped(queries[0], tv, groups, 7)
        assert [(r["group"], r["score"]) for r in one] == [(r["group"], r["score"]) for r in same]
        for bad in (lambda: f.searchNearestNeighborsMaxSim([queries[0]], tv, None, 7),
                    lambda: f.searchNearestNeighborsMaxSim(None, tv, groups, 7),
                    lambda: f.searchNearestNeighborsMaxSim([], tv, groups, 7),
                    lambda: f.searchNearestNeighborsMaxSim([queries[0]], tv, groups, -1),
                    lambda: f.searchNearestNeighborsMaxSim([queries[0][:5]], tv, groups, 7)):
            with pytest.raises(Exception):
                bad()
