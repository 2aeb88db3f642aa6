"""GPU: the exact MaxSim rerank - bbq_rerank_maxsim_groups_batch, bbq_search_maxsim_rerank_batch - byte for byte, no tolerance, three
ways: against the model of tests/maxsim_rerank_model.py (the oracle's computeSimilarity per token and row, the maximum under the NaN and
-0.0 rule, the ordered f64 sum), against the same quantity composed from this library's own Vectors.rerank_scores per token plus
maxsim_reduce_true, and a second call against the first.  2 000 rows in groups of 1, 2, 63, 64, 65, 257 and 300 rows and empty ones, so
that candidates lie inside a wave, across a wave's edge and across several; hostile rows among them."""
import functools

import numpy as np
import pytest

import orclib as O
import maxsim_rerank_model as MR
import test_gpu_score_ords as SO
import test_groups_cpu as GC
from bbqlib import bbq_amd as B, capi

pytestmark = pytest.mark.gpu

LENS = [1, 2, 0, 63, 64, 65, 0, 0, 257, 300, 300, 0, 257, 65, 64, 63, 2, 1, 64, 64, 64, 64, 100, 140]
OFF = np.concatenate([[0], np.cumsum(LENS)]).astype(np.int64)
N = int(OFF[-1])
TOKENS = (1, 32, 33, 70)                      # on both sides of a token block of 32, and three blocks
SPANS = [(0, 1), (1, 33), (33, 66), (66, 136), (0, 1), (1, 33)]   # the tokens of the six queries among the 136 token vectors
ZERO_ROW, NAN_IN_PAIR, INF_ROW, BIG_ROWS, BOTH_INF, INF_PAIR, NAN_ALONE = 0, 1, 10, (70, 71), 140, (1501, 1502), 1503
assert N == 2000


@functools.lru_cache(maxsize=None)
def _index():
    """an index of N rows: the group sets and filters hang on it - its dimension and rows are not the rerank's"""
    rng = np.random.default_rng(11)
    base = rng.standard_normal((N, 64)).astype(np.float32)
    codes, corr, cen = B.quantize_vectors(base, 1)
    return B.Index(codes, corr, 64, B.centroid_dp(cen))


@functools.lru_cache(maxsize=None)
def _masks():
    rng = np.random.default_rng(12)
    run = np.ones(N, bool)
    run[OFF[9] + 60:OFF[9] + 200] = False       # 140 rows inside the first group of 300: a whole wave of it is rejected wherever it falls
    m = {"all": np.ones(N, bool), "random_half": rng.random(N) < 0.5, "run_out": run}
    for a in m.values():
        a.setflags(write=False)
    return m


@functools.lru_cache(maxsize=None)
def _data(dim):
    rng = np.random.default_rng(100 + dim)
    base = rng.standard_normal((N, dim)).astype(np.float32)
    base[ZERO_ROW] = 0.0                          # COSINE gives 0
    base[NAN_IN_PAIR, 0] = np.nan                 # beside an ordinary row: never the maximum
    base[INF_ROW, 0] = np.inf
    base[list(BIG_ROWS)] *= np.float32(1e30)
    base[BOTH_INF, 0], base[BOTH_INF, dim - 1] = np.inf, -np.inf     # dim 1: -Inf alone
    base[INF_PAIR[0], 0], base[INF_PAIR[1], 0] = np.inf, -np.inf
    base[NAN_ALONE, dim // 2] = np.nan            # a group of one row: every token's maximum is NaN
    tokens = rng.standard_normal((136, dim)).astype(np.float32)
    tokens[70] *= np.float32(1e30)
    tokens[40, 0] = 0.0
    tokens[3] = 0.0                               # an all-zero token: COSINE's na == 0
    base.setflags(write=False)
    tokens.setflags(write=False)
    return base, tokens


@functools.lru_cache(maxsize=None)
def _model(dim, sim):
    """c(t, r) of every token and row from the oracle, once per (dim, similarity)"""
    base, tokens = _data(dim)
    c = MR.true_scores(tokens, base, sim)
    c.setflags(write=False)
    return c


def _lists(live, seed):
    rng = np.random.default_rng(seed)
    shuffled = rng.permutation(live)
    dups = np.concatenate([rng.permutation(live), rng.choice(live, 7), live[:3]])
    single = np.array([9 if 9 in live else live[0]], np.int64)
    return [live.copy(), live[::-1].copy(), dups, shuffled, np.zeros(0, np.int64), single]


def _check(V, groups, dim, sim, mask, c_model, c_lib, seed, msg):
    _, tokens = _data(dim)
    live = MR.live_groups(OFF, mask)
    lists = _lists(live, seed)
    tok = [tokens[a:b] for a, b in SPANS]
    got, coff = V.rerank_maxsim_groups_batch(tok, groups, lists, sim)
    again, _ = V.rerank_maxsim_groups_batch(tok, groups, lists, sim)
    assert got.dtype == np.float64 and coff.tolist() == np.concatenate([[0], np.cumsum([len(l) for l in lists])]).tolist()
    assert got.tobytes() == again.tobytes(), msg + ": two calls differ"
    rep_model = MR.rep_true(c_model, OFF, mask, live)         # [136, live]
    rep_lib = MR.rep_true(c_lib, OFF, mask, live)
    where = {int(g): i for i, g in enumerate(live)}
    for q, ((a, b), lst) in enumerate(zip(SPANS, lists)):
        at = [where[int(g)] for g in lst]
        want = MR.reduce_true(rep_model[a:b])[at]
        composed = capi.maxsim_reduce_true(rep_lib[a:b])[at]
        mine = got[coff[q]:coff[q + 1]]
        w = "%s: query %d (%d tokens, %d candidates)" % (msg, q, b - a, len(lst))
        np.testing.assert_array_equal(MR.bits(mine), MR.bits(want), err_msg=w + ": against the model")
        np.testing.assert_array_equal(MR.bits(mine), MR.bits(composed), err_msg=w + ": against rerank_scores + maxsim_reduce_true")
    return got


@pytest.mark.parametrize("sim", [0, 1, 2])
@pytest.mark.parametrize("dim", [1, 31, 33, 100, 768])
def test_shapes_filters_lists_and_hostile_rows(dim, sim):
    base, tokens = _data(dim)
    c_model = _model(dim, sim)
    ix = _index()
    V = capi.Vectors(base)
    try:
        c_lib = np.stack(V.rerank_scores(tokens, [np.arange(N, dtype=np.int32)] * len(tokens), sim))
        nan_groups = 0
        for mname, mask in _masks().items():
            flt = capi.Filter(ix, mask) if mname != "all" else None
            try:
                with capi.Groups(ix, OFF, flt) as groups:
                    got = _check(V, groups, dim, sim, mask, c_model, c_lib, 7 + dim, "dim %d sim %d %s" % (dim, sim, mname))
                    nan_groups += int(np.isnan(got).sum())
            finally:
                if flt is not None:
                    flt.close()
        assert nan_groups > 0                                  # the group of the NaN row alone, at least
    finally:
        V.close()


def _raw(L, V, groups, voff, q, sim, coff, cand):
    voff, coff = np.ascontiguousarray(voff, np.int64), np.ascontiguousarray(coff, np.int64)
    cand = np.ascontiguousarray(cand, np.int32)
    out = np.full(max(len(cand), 1), -7.0, np.float64)
    rc = L.bbq_rerank_maxsim_groups_batch(V._h, groups._h, len(voff) - 1, voff.ctypes.data, q.ctypes.data, sim, coff.ctypes.data, cand.ctypes.data, out.ctypes.data)
    return rc, L.bbq_last_error().decode("utf-8"), bool((out == -7.0).all())


def test_refusals_and_update():
    dim = 33
    base, tokens = _data(dim)
    ix = _index()
    L = capi.lib()
    q = np.ascontiguousarray(tokens[:6])
    voff, coff = [0, 2, 6], [0, 3, 7]
    V, longer = capi.Vectors(base), capi.Vectors(np.concatenate([base, base[:1]]))
    try:
        with capi.Filter(ix, _masks()["run_out"]) as flt, capi.Groups(ix, OFF) as groups, capi.Groups(ix, OFF, flt) as filtered:
            rc, msg, untouched = _raw(L, V, groups, voff, q, 1, coff, [5, 1, 5, 0, 23, 9, 3])
            assert rc == capi.OK and not untouched, msg
            ng = len(OFF) - 1
            for cand, word in (([5, 1, 5, 0, -1, ng, 3], "query 1, position 1: group -1"), ([5, 1, ng, 0, -1, 9, 3], "query 0, position 2: group %d" % ng)):
                rc, msg, untouched = _raw(L, V, groups, voff, q, 1, coff, cand)
                assert rc == capi.ERR_INVALID_ARG and word in msg and "bbq_rerank_maxsim_groups_batch" in msg and untouched, msg
            rc, msg, untouched = _raw(L, V, groups, voff, q, 1, coff, [5, 1, 5, 0, 23, 2, 3])            # group 2 is empty
            assert rc == capi.ERR_INVALID_ARG and "query 1, position 2: group 2" in msg and "not live" in msg and untouched, msg
            for sim in (-1, 3):
                rc, msg, untouched = _raw(L, V, groups, voff, q, sim, coff, [5, 1, 5, 0, 23, 9, 3])
                assert rc == capi.ERR_INVALID_ARG and "不支持的相似性函数" in msg and untouched, msg
            for bad, word in (([1, 2, 6], "query 0"), ([0, 2, 2], "query 1")):
                rc, msg, untouched = _raw(L, V, groups, bad, q, 1, coff, [5, 1, 5, 0, 23, 9, 3])
                assert rc == capi.ERR_INVALID_ARG and word in msg and untouched, msg
            rc, msg, untouched = _raw(L, longer, groups, voff, q, 1, coff, [5, 1, 5, 0, 23, 9, 3])       # vectors of another size
            assert rc == capi.ERR_INVALID_ARG and "group set" in msg and untouched, msg
            # nothing to answer is no error
            assert L.bbq_rerank_maxsim_groups_batch(V._h, groups._h, 0, None, None, 1, None, None, None) == capi.OK
            sc, co = V.rerank_maxsim_groups_batch([tokens[:2], tokens[2:6]], groups, [[], []], 1)
            assert len(sc) == 0 and co.tolist() == [0, 0, 0]
            # after an update of the rows the set still serves and the scores follow the new rows
            rng = np.random.default_rng(5)
            ords = np.array([OFF[9] + 5, OFF[9] + 250, 2], np.int32)
            fresh = rng.standard_normal((3, dim)).astype(np.float32) * 3
            V.update(ords, fresh)
            base2 = base.copy()
            base2[ords] = fresh
            lst = [np.array([9, 1, 9, 4], np.int64), np.array([8, 9], np.int64)]
            tok = [tokens[0:3], tokens[66:101]]
            c2 = MR.true_scores(tokens[[0, 1, 2] + list(range(66, 101))], base2[:OFF[10]], 1)
            c2 = np.concatenate([c2, np.zeros((c2.shape[0], N - c2.shape[1]))], axis=1)
            for grp, mask in ((groups, _masks()["all"]), (filtered, _masks()["run_out"])):
                got, co = V.rerank_maxsim_groups_batch(tok, grp, lst, 1)
                np.testing.assert_array_equal(MR.bits(got[:4]), MR.bits(MR.scores(c2[:3], OFF, mask, lst[0])))
                np.testing.assert_array_equal(MR.bits(got[4:]), MR.bits(MR.scores(c2[3:], OFF, mask, lst[1])))
            # an append makes the set stale: refused with nothing written
            V.append(base[:5])
            rc, msg, untouched = _raw(L, V, groups, voff, q, 1, coff, [5, 1, 5, 0, 23, 9, 3])
            assert rc == capi.ERR_INVALID_ARG and "group set" in msg and untouched, msg
    finally:
        V.close()
        longer.close()


@pytest.mark.parametrize("lname", ["random_1_20", "groups_of_64"])
def test_the_recipe_is_the_composition(lname):
    """bbq_search_maxsim_rerank_batch for selector 0 and 1, k in {0, 1, 10}, factor in {1, 3} - groups_of_64 has 16 groups, so k x factor
    exceeds L there - equals search_maxsim_batch, the score call and the oracle's selectors, composed in Python"""
    g, sim, codes, corr, cdp, qs = SO._case("c1_1000x128_cos_qb4")
    base, queries = O.golden_inputs(g)
    n, qb = g["n"], g["qb"]
    T = min(len(qs), 5)
    spans = [(0, T), (1, 2)] if T >= 2 else [(0, 1)]
    tok = [(np.stack([qs[i][0] for i in range(a, b)]), np.stack([qs[i][1] for i in range(a, b)])) for a, b in spans]
    raw = [np.stack([queries[i] for i in range(a, b)]).astype(np.float32) for a, b in spans]
    off = GC.layouts(n)[lname]
    ix = B.Index(codes, corr, g["dim"], cdp)
    V = capi.Vectors(base)
    try:
        with capi.Groups(ix, off) as groups:
            L = groups.live
            saw_more_than_live = False
            for k in (0, 1, 10):
                for factor in (1, 3):
                    saw_more_than_live |= k * factor > L
                    first, _ = ix.search_maxsim_batch(tok, qb, sim, k * factor, groups)
                    true, coff = V.rerank_maxsim_groups_batch(raw, groups, [r[0] for r in first], 1)
                    for selector, how in ((0, "heap"), (1, "sort")):
                        got = capi.search_maxsim_rerank_batch(ix, V, groups, raw, tok, qb, sim, k, factor, selector, 1)
                        assert len(got) == len(spans)
                        for q in range(len(spans)):
                            t = true[coff[q]:coff[q + 1]]
                            pos = O.rerank_select(t, k, how) if k > 0 else np.zeros(0, np.int32)
                            w = "%s k=%d factor=%d %s query %d" % (lname, k, factor, how, q)
                            assert len(got[q][0]) == min(k, len(t)), w
                            np.testing.assert_array_equal(got[q][0], first[q][0][pos], err_msg=w + ": groups")
                            assert got[q][1].tobytes() == first[q][1][pos].tobytes(), w + ": quantized scores"
                            assert got[q][2].tobytes() == t[pos].tobytes(), w + ": true scores"
            assert saw_more_than_live == (lname == "groups_of_64")
    finally:
        V.close()
        ix.close()


def test_python_api():
    g, sim, codes, corr, cdp, qs = SO._case("c1_1000x128_cos_qb4")
    base, queries = O.golden_inputs(g)
    f = B.createBinaryQuantizationFormat({"queryBits": 4, "indexBits": 1, "quantizer": {"similarityFunction": "COSINE", "lambda": 0.1, "iters": 5}})
    tv = f.quantizeVectors(list(base))["quantizedVectors"]
    off = GC.layouts(g["n"])["random_1_20"]
    vecs = [queries[i] for i in range(min(len(qs), 4))]
    V = B.createDeviceVectors(base)
    try:
        with B.createRowGroups(tv, off) as groups:
            first = f.searchNearestNeighborsMaxSim(vecs, tv, groups, 15)
            true, _ = V.rerank_maxsim_groups_batch([np.stack(vecs)], groups, [[r["group"] for r in first]], 1)
            for selector in ("heap", "sort"):
                got = f.searchNearestNeighborsMaxSimReranked(vecs, tv, V, groups, 5, 3, selector)
                pos = O.rerank_select(true, 5, selector)
                assert [r["group"] for r in got] == [first[i]["group"] for i in pos]
                assert [r["trueScore"] for r in got] == [float(true[i]) for i in pos]
                assert [r["quantizedScore"] for r in got] == [first[i]["score"] for i in pos]
            assert f.searchNearestNeighborsMaxSimReranked(vecs, tv, V, groups, 0, 3) == []
            for bad in (lambda: f.searchNearestNeighborsMaxSimReranked(vecs, tv, None, groups, 5, 3),
                        lambda: f.searchNearestNeighborsMaxSimReranked(vecs, tv, V, None, 5, 3),
                        lambda: f.searchNearestNeighborsMaxSimReranked(vecs, tv, V, groups, -1, 3),
                        lambda: f.searchNearestNeighborsMaxSimReranked(vecs, tv, V, groups, 5, 0),
                        lambda: f.searchNearestNeighborsMaxSimReranked([queries[0][:5]], tv, V, groups, 5, 3)):
                with pytest.raises(Exception):
                    bad()
    finally:
        V.close()
