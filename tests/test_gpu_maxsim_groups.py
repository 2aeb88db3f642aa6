"""GPU: MaxSim over chosen groups - bbq_score_maxsim_groups_batch, bbq_search_maxsim_groups_batch - against the model of
tests/maxsim_groups_model.py, bit for bit: every candidate's score is the sum the MaxSim search defines for its group, and a query's
answer is what the reference's loop returns when it visits the query's candidates in the order given - group numbers, score bits, order,
out_n.  The fixtures are test_gpu_maxsim's: 1 300 rows, 64 and 768 dimensions, both corrections layouts."""
import numpy as np
import pytest

import orclib as O
import append_recipe as R
import maxsim_model as M
import maxsim_groups_model as MG
import test_gpu_maxsim as GM              # its vectors, layouts, cached representatives, tie and NaN cases (read-only)
import test_gpu_score_ords as SO
import test_maxsim_groups_cpu as TC       # the tie lists
import test_spans_filtered_cpu as FC      # the masks
import test_groups_cpu as GC              # the layouts
from test_gpu_score_ords import canon32
from bbqlib import bbq_amd as B, capi

pytestmark = pytest.mark.gpu

N = GM.N


def _tokens(qq, qc, spans):
    return [(qq[a:b], qc[a:b]) for a, b in spans]


def assert_lists(ix, groups, rep, live, qq, qc, spans, lists, qb, sim, msg, ks=(3, 40, None)):
    """one score call and one search call per k (None: longer than the longest list): every candidate's score bits, and every query's
    groups, score bits, order and count, equal the model's.  Returns the calls' bytes"""
    assert len(spans) == len(lists)
    tok = _tokens(qq, qc, spans)
    got, coff = ix.score_maxsim_groups_batch(tok, qb, sim, groups, lists)
    seen = [got.tobytes()]
    assert coff.tolist() == np.concatenate([[0], np.cumsum([len(l) for l in lists])]).tolist()
    for q, ((a, b), lst) in enumerate(zip(spans, lists)):
        want = MG.scores(rep[a:b], live, lst)
        np.testing.assert_array_equal(canon32(got[coff[q]:coff[q + 1]]), canon32(want),
                                      err_msg="%s: query %d (%d tokens, %d candidates): score bits" % (msg, q, b - a, len(lst)))
    for k in ks:
        k = max(len(l) for l in lists) + 1 if k is None else k
        res = ix.search_maxsim_groups_batch(tok, qb, sim, k, groups, lists)
        assert len(res) == len(lists)
        for q, ((a, b), lst) in enumerate(zip(spans, lists)):
            wg, ws = MG.answer(rep[a:b], live, lst, k)
            where = "%s: query %d (%d tokens, %d candidates) k=%d" % (msg, q, b - a, len(lst), k)
            assert len(res[q][0]) == min(k, len(lst)), where + ": out_n"
            np.testing.assert_array_equal(res[q][0], wg, err_msg=where + ": groups")
            np.testing.assert_array_equal(canon32(res[q][1]), canon32(ws), err_msg=where + ": score bits")
        seen.append(b"".join(x.tobytes() for r in res for x in r))
    return seen


def _calls(lists, nq):
    """the named lists dealt to calls of nq queries, a different list per query; the last call is filled up from the front"""
    names = list(lists)
    out = []
    for i in range(0, len(names), nq):
        out.append([names[(i + j) % len(names)] for j in range(nq)])
    return out


@pytest.mark.parametrize("dim", [64, 768])
@pytest.mark.parametrize("compact", [True, False])
def test_layouts_filters_lists_and_token_counts(dim, compact):
    """every layout without a filter, three of them under a random half and under a mask that rejects a whole tile; per (layout, mask)
    every list of the model - ascending, reversed, a subset with duplicates, one candidate, none, and the lists of exactly 64, 65, 256
    and 257 expanded rows where the layout can make them - dealt to calls that hold a query of every token count, a different list
    each.  one_group is a single candidate of 1 300 rows: every wave merges through the atomic maximum"""
    sim, qb, codes, corr, cdp, qq, qc, s32 = GM._vectors(dim)
    spans = GM._queries(GM._token_counts())
    masks = FC.masks(N)
    cases = [(l, "all") for l in GM._layouts()] + [(l, m) for l in ("groups_of_64", "singletons", "around_chunk_edges") for m in ("random_half", "tile_out_and_ends")]
    ix = B.Index(codes, corr, dim, cdp, corrections="compact" if compact else "inline")
    try:
        for lname, mname in cases:
            off, mask = GM._layouts()[lname], masks[mname]
            rep, live = GM._reps(dim, s32, off, mask, lname, mname)
            lists = MG.candidate_lists(off, live)
            with GM._open(ix, off, mask) as groups:
                for names in _calls(lists, len(spans)):
                    assert_lists(ix, groups, rep, live, qq, qc, spans, [lists[n] for n in names], qb, sim, "%d %s %s %s" % (dim, lname, mname, names))
                # every live group, ascending: the MaxSim search's own answer, in the same process
                tok = _tokens(qq, qc, spans)
                for k in (3, 40):
                    want, _ = ix.search_maxsim_batch(tok, qb, sim, k, groups)
                    got = ix.search_maxsim_groups_batch(tok, qb, sim, k, groups, [live] * len(spans))
                    for q in range(len(spans)):
                        np.testing.assert_array_equal(got[q][0], want[q][0])
                        assert got[q][1].tobytes() == want[q][1].tobytes(), "%d %s %s query %d k=%d" % (dim, lname, mname, q, k)
    finally:
        ix.close()


@pytest.mark.parametrize("dim", [64, 768])
def test_ties(dim):
    """groups 2 and 4 are copies of one row and score equal sums: the answer is the heap's over the list in its order, which is not the
    stable sort's for at least one of the lists"""
    sim, qb, _, _, cdp, qq, qc, _ = GM._vectors(dim)
    codes, corr, s32 = GM._tie_case(dim)
    off = np.array([0, 64, 200, 210, 700, 710, N], np.int64)
    rep, live = M.rep_scores(s32, off, np.ones(N, bool))
    differs = 0
    ix = B.Index(codes, corr, dim, cdp)
    try:
        with capi.Groups(ix, off) as groups:
            for lst, k in TC.TIE_LISTS:
                lst = np.array(lst, np.int64)
                for span in ((0, 5), (0, 1)):
                    differs += MG.answer(rep[span[0]:span[1]], live, lst, k)[0].tolist() != MG.sorted_answer(rep[span[0]:span[1]], live, lst, k)[0].tolist()
                assert_lists(ix, groups, rep, live, qq, qc, [(0, 5), (0, 1)], [lst, lst[::-1].copy()], qb, sim, "ties %d %s" % (dim, lst), ks=(k, 1, 2))
        assert differs > 0
    finally:
        ix.close()


@pytest.mark.parametrize("dim", [64, 768])
@pytest.mark.parametrize("compact", [True, False])
def test_nan(dim, compact):
    """row 77 scores NaN for every token: inside a larger group it never represents, as a singleton candidate - or the only accepted row
    of its group - its sum is NaN and stands where the reference's heap puts it"""
    sim, qb, codes, _, cdp, qq, qc, _ = GM._vectors(dim)
    corr, s32 = GM._nan_case(dim)
    everything = np.ones(N, bool)
    tens, single = GC._tiled(N, 10), GC.layouts(N)["singletons"]
    spans = [(0, 4), (1, 2)]
    ix = B.Index(codes, corr, dim, cdp, corrections="compact" if compact else "inline")
    try:
        with capi.Groups(ix, tens) as groups:
            rep, live = M.rep_scores(s32, tens, everything)
            lists = [np.array([9, 7, 3, 7, 120], np.int64), np.array([7], np.int64)]
            assert not np.isnan(MG.scores(rep, live, lists[0])).any()
            assert_lists(ix, groups, rep, live, qq, qc, spans, lists, qb, sim, "NaN inside a group", ks=(1, 3, 10))
        with capi.Groups(ix, single) as groups:
            rep, live = M.rep_scores(s32, single, everything)
            lists = [np.array([76, 77, 78, 5, 77, 1299], np.int64), np.array([77], np.int64)]
            assert np.isnan(MG.scores(rep, live, lists[0])).sum() == 2
            assert_lists(ix, groups, rep, live, qq, qc, spans, lists, qb, sim, "NaN as a candidate", ks=(1, 3, 10))
            assert_lists(ix, groups, rep, live, qq, qc, spans, [l[::-1].copy() for l in lists], qb, sim, "NaN as a candidate, reversed", ks=(1, 3, 10))
        only = np.zeros(N, bool)
        only[[77, 150, 900]] = True                                         # the group [70, 80) has the NaN row alone
        with capi.Filter(ix, only) as flt, capi.Groups(ix, tens, flt) as groups:
            rep, live = M.rep_scores(s32, tens, only)
            assert live.tolist() == [7, 15, 90]
            lists = [np.array([90, 7, 15], np.int64), np.array([7, 7], np.int64)]
            assert np.isnan(MG.scores(rep, live, lists[0])).sum() == 1
            assert_lists(ix, groups, rep, live, qq, qc, spans, lists, qb, sim, "a group of NaN alone", ks=(1, 2, 3))
    finally:
        ix.close()


def test_two_runs_and_sub_batches_give_identical_bytes():
    """1 300 singleton candidates per query under 1 MiB of scratch: three queries per sub-batch, so the call of six takes two, and the
    longest query three token blocks; the same bytes as under the default, and as a second run"""
    dim = 768
    sim, qb, codes, corr, cdp, qq, qc, s32 = GM._vectors(dim)
    off = GC.layouts(N)["singletons"]
    spans = GM._queries(GM._token_counts())
    per_query = (8 * GM._tb() + 12) * N
    assert 4 * per_query > (1 << 20) >= 3 * per_query and len(spans) == 6
    rep, live = GM._reps(dim, s32, off, FC.masks(N)["all"], "singletons", "all")
    rng = np.random.default_rng(31)
    lists = [rng.permutation(live) for _ in spans]
    ix = B.Index(codes, corr, dim, cdp)
    try:
        with capi.Groups(ix, off) as groups:
            first = assert_lists(ix, groups, rep, live, qq, qc, spans, lists, qb, sim, "default scratch", ks=(10,))
            again = assert_lists(ix, groups, rep, live, qq, qc, spans, lists, qb, sim, "second run", ks=(10,))
            ix.set_option("group_scratch_mb", 1)
            small = assert_lists(ix, groups, rep, live, qq, qc, spans, lists, qb, sim, "1 MiB of scratch", ks=(10,))
            ix.set_option("group_scratch_mb", 256)
            assert first == again == small
    finally:
        ix.close()


def _raw(L, handle, groups, voff, qq, qc, qb, sim, k, coff, cand, null_out=False):
    """both C entry points with prefilled outputs: [(rc, message, outputs untouched)] - the score call first (k is the search's)"""
    voff, coff = np.ascontiguousarray(voff, np.int64), np.ascontiguousarray(coff, np.int64)
    cand = np.ascontiguousarray(cand, np.int32)
    nq = len(voff) - 1
    gh = None if groups is None else groups._h
    out = np.full(max(len(cand), 1), -7.0, np.float32)
    rc = L.bbq_score_maxsim_groups_batch(handle._h, gh, nq, voff.ctypes.data, qq.ctypes.data, qc.ctypes.data, qb, sim, coff.ctypes.data, cand.ctypes.data,
                                         None if null_out else out.ctypes.data)
    res = [(rc, L.bbq_last_error().decode("utf-8"), bool((out == -7.0).all()))]
    grp, sc = np.full(nq * max(k, 1), -7, np.int32), np.full(nq * max(k, 1), -7.0, np.float32)
    cnt = np.full(nq, -7, np.int64)
    rc = L.bbq_search_maxsim_groups_batch(handle._h, gh, nq, voff.ctypes.data, qq.ctypes.data, qc.ctypes.data, qb, sim, k, coff.ctypes.data, cand.ctypes.data,
                                          None if null_out else grp.ctypes.data, sc.ctypes.data, cnt.ctypes.data)
    res.append((rc, L.bbq_last_error().decode("utf-8"), bool((grp == -7).all() and (sc == -7.0).all() and (cnt == -7).all())))
    return res


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
    ng = len(off) - 1
    voff, coff = [0, 2, 6], [0, 3, 7]
    L = capi.lib()
    ix = B.Index(codes, corr, g["dim"], cdp)
    multi = B.Index.create_multi(codes, corr, g["dim"], cdp, [0, 0], pilot_rows=0)
    groups = capi.Groups(ix, off)
    try:
        for rc, msg, untouched in _raw(L, ix, groups, voff, qq, qc, qb, sim, 5, coff, [5, 1, 5, 0, ng - 1, 2, 3]):
            assert rc == capi.OK and not untouched, msg
        # a group number that is no group of the set: the first one in call order is named
        for cand, word in (([5, 1, 5, 0, -1, ng, 3], "query 1, position 1: group -1"), ([5, 1, ng, 0, -1, 2, 3], "query 0, position 2: group %d" % ng)):
            for rc, msg, untouched in _raw(L, ix, groups, voff, qq, qc, qb, sim, 5, coff, cand):
                assert rc == capi.ERR_INVALID_ARG and word in msg and untouched, msg
        # an empty group (empty_groups: group 0 is [0, 0)), and a group the filter empties (row 0, a singleton)
        with capi.Groups(ix, GC.layouts(n)["empty_groups"]) as holes:
            for rc, msg, untouched in _raw(L, ix, holes, voff, qq, qc, qb, sim, 5, coff, [1, 2, 1, 6, 6, 0, 2]):
                assert rc == capi.ERR_INVALID_ARG and "query 1, position 2: group 0" in msg and "not live" in msg and untouched, msg
        with capi.Filter(ix, FC.masks(n)["tile_out_and_ends"]) as flt, capi.Groups(ix, GC.layouts(n)["singletons"], flt) as some:
            for rc, msg, untouched in _raw(L, ix, some, voff, qq, qc, qb, sim, 5, coff, [1, 2, 0, 5, 5, 70, 2]):
                assert rc == capi.ERR_INVALID_ARG and "query 0, position 2: group 0" in msg and "not live" in msg and untouched, msg
            for rc, msg, untouched in _raw(L, ix, some, voff, qq, qc, qb, sim, 5, coff, [1, 2, 3, 5, 5, 70, 2]):
                assert rc == capi.ERR_INVALID_ARG and "query 1, position 2: group 70" in msg and untouched, msg
            for rc, msg, untouched in _raw(L, ix, some, voff, qq, qc, qb, sim, 0, coff, [1, 2, 3, 5, 5, 70, 2])[1:]:
                assert rc == capi.ERR_INVALID_ARG and untouched, msg          # whatever k is
        for bad, word in (([1, 3, 7], "cand_offsets[0]"), ([0, 4, 3], "query 1")):
            for rc, msg, untouched in _raw(L, ix, groups, voff, qq, qc, qb, sim, 5, bad, [5, 1, 5, 0, 4, 2, 3]):
                assert rc == capi.ERR_INVALID_ARG and word in msg and untouched, msg
        for bad, word in (([1, 2, 6], "query 0"), ([0, 2, 2], "query 1")):
            for rc, msg, untouched in _raw(L, ix, groups, bad, qq, qc, qb, sim, 5, coff, [5, 1, 5, 0, 4, 2, 3]):
                assert rc == capi.ERR_INVALID_ARG and word in msg and untouched, msg
        for rc, msg, untouched in _raw(L, ix, groups, voff, qq, qc, qb, sim, 5, coff, [5, 1, 5, 0, 4, 2, 3], null_out=True):
            assert rc == capi.ERR_INVALID_ARG and "null output" in msg and untouched, msg
        rc, msg, untouched = _raw(L, ix, groups, voff, qq, qc, qb, sim, -1, coff, [5, 1, 5, 0, 4, 2, 3])[1]
        assert rc == capi.ERR_NEGATIVE_K and untouched
        for rc, msg, untouched in _raw(L, ix, None, voff, qq, qc, qb, sim, 5, coff, [5, 1, 5, 0, 4, 2, 3]):
            assert rc == capi.ERR_INVALID_ARG and untouched
        for rc, msg, untouched in _raw(L, multi, groups, voff, qq, qc, qb, sim, 5, coff, [5, 1, 5, 0, 4, 2, 3]):
            assert rc == capi.ERR_UNSUPPORTED and "multi-device" in msg and untouched
        # nothing to answer is no error: no queries, no candidates (the search call still writes out_n), k == 0
        assert L.bbq_score_maxsim_groups_batch(ix._h, groups._h, 0, None, None, None, qb, sim, None, None, None) == capi.OK
        assert L.bbq_search_maxsim_groups_batch(ix._h, groups._h, 0, None, None, None, qb, sim, 5, None, None, None, None, None) == capi.OK
        tok = [(qq[:2], qc[:2]), (qq[2:6], qc[2:6])]
        sc, co = ix.score_maxsim_groups_batch(tok, qb, sim, groups, [[], []])
        assert len(sc) == 0 and co.tolist() == [0, 0, 0]
        assert [len(r[0]) for r in ix.search_maxsim_groups_batch(tok, qb, sim, 5, groups, [[], []])] == [0, 0]
        assert [len(r[0]) for r in ix.search_maxsim_groups_batch(tok, qb, sim, 0, groups, [[1, 2], [3]])] == [0, 0]
        assert [len(r[0]) for r in ix.search_maxsim_groups_batch(tok, qb, sim, 5, groups, [[], [3, 3]])] == [0, 2]
        # an in-place update: the set still serves.  An append: refused with nothing written
        ix.update_rows(np.array([3], np.int32), new_codes[:1], new_corr[:1])
        for rc, msg, untouched in _raw(L, ix, groups, voff, qq, qc, qb, sim, 5, coff, [5, 1, 5, 0, 4, 2, 3]):
            assert rc == capi.OK and not untouched, msg
        ix.append_rows(new_codes, new_corr)
        for rc, msg, untouched in _raw(L, ix, groups, voff, qq, qc, qb, sim, 5, coff, [5, 1, 5, 0, 4, 2, 3]):
            assert rc == capi.ERR_INVALID_ARG and "group set" in msg and untouched, msg
    finally:
        groups.close()
        ix.close()
        multi.close()


def test_python_api():
    """api.py: searchNearestNeighborsMaxSimInGroups on the README-sized case"""
    g, sim, codes, corr, cdp, qs = SO._case("c1_1000x128_cos_qb4")
    base, queries = O.golden_inputs(g)
    f = B.createBinaryQuantizationFormat({"queryBits": 4, "indexBits": 1, "quantizer": {"similarityFunction": "COSINE", "lambda": 0.1, "iters": 5}})
    tv = f.quantizeVectors(list(base))["quantizedVectors"]
    n = g["n"]
    T = min(len(qs), 5)
    s32 = [qs[i][4] for i in range(T)]
    off = GC.layouts(n)["random_1_20"]
    mask = FC.masks(n)["drop_every_third"]
    vecs = [queries[i] for i in range(T)]
    with B.createRowFilter(tv, mask) as flt, B.createRowGroups(tv, off, flt) as groups, B.createRowGroups(tv, off) as unfiltered:
        for grp, m in ((groups, mask), (unfiltered, FC.masks(n)["all"])):
            rep, live = M.rep_scores(s32, off, m)
            lst = np.random.default_rng(5).permutation(live)[:40]
            lst = np.concatenate([lst, lst[:2]])
            wg, ws = MG.answer(rep, live, lst, 7)
            got = f.searchNearestNeighborsMaxSimInGroups(vecs, tv, grp, [int(x) for x in lst], 7)
            assert [r["group"] for r in got] == [int(i) for i in wg]
            np.testing.assert_array_equal(canon32([r["score"] for r in got]), canon32(ws))
            same = f.searchNearestNeighborsMaxSim(vecs, tv, grp, 7)
            assert f.searchNearestNeighborsMaxSimInGroups(vecs, tv, grp, [int(x) for x in live], 7) == same
        assert f.searchNearestNeighborsMaxSimInGroups(vecs, tv, groups, [3, 4], 0) == []
        assert f.searchNearestNeighborsMaxSimInGroups(vecs, tv, groups, [], 7) == []
        for bad in (lambda: f.searchNearestNeighborsMaxSimInGroups(vecs, tv, None, [3], 7),
                    lambda: f.searchNearestNeighborsMaxSimInGroups(None, tv, groups, [3], 7),
                    lambda: f.searchNearestNeighborsMaxSimInGroups(vecs, tv, groups, None, 7),
                    lambda: f.searchNearestNeighborsMaxSimInGroups(vecs, tv, groups, [3], -1),
                    lambda: f.searchNearestNeighborsMaxSimInGroups(vecs, tv, groups, [len(off) - 1], 7),
                    lambda: f.searchNearestNeighborsMaxSimInGroups([queries[0][:5]], tv, groups, [3], 7)):
            with pytest.raises(Exception):
                bad()
