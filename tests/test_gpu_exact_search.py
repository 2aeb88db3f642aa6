"""GPU: the exact search - bbq_vectors_search_batch - byte for byte, no tolerance, against the model of tests/exact_model.py (the
oracle's computeSimilarity for every pair, its stable descending sort over the accepted rows, the first k), against
Vectors.rerank_scores of the returned rows on the same device, a second call against the first, and with exact_slab_rows 256 against
automatic slabs.  The shapes are the smallest at which the kernels take another path: widths on both sides of the 32-column stage and
one that is no multiple of 4, row counts on both sides of a wave and of a 256-row slab, query counts on both sides of the 32-query
block, k up to the 4096 the select pass holds."""
import functools
import threading

import numpy as np
import pytest

import exact_model as EM
from bbqlib import bbq_amd as B, capi

pytestmark = pytest.mark.gpu

SLABS = (256, 0)


@functools.lru_cache(maxsize=None)
def _index(n):
    """an index of n rows: filters hang on it - its dimension and rows are not the search's"""
    rng = np.random.default_rng(7 + n)
    codes, corr, cen = B.quantize_vectors(rng.standard_normal((n, 64)).astype(np.float32), 1)
    return B.Index(codes, corr, 64, B.centroid_dp(cen))


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


def _check(V, c, queries, sim, k, mask=None, msg=""):
    """one call per slab setting, each held to the model, to rerank_scores and to the other; returns the answer"""
    n = V.n
    assert c.shape == (queries.shape[0], n)
    want = [EM.topk(c[q], k, mask) for q in range(queries.shape[0])]
    flt = capi.Filter(_index(n), mask) if mask is not None else None
    first = None
    for slab in SLABS:
        V.set_option("exact_slab_rows", slab)
        idx, out, cnt = V.search_batch(queries, k, sim, flt)
        w = "%s, sim %d, %d rows, %d queries, k %d, slab %d" % (msg, sim, n, queries.shape[0], k, slab)
        assert idx.dtype == np.int32 and out.dtype == np.float64 and cnt.dtype == np.int64
        for q, (rows, bits) in enumerate(want):
            assert cnt[q] == rows.shape[0], w + ": query %d: count" % q
            assert idx[q, :cnt[q]].tolist() == rows.tolist(), w + ": query %d: rows" % q
            assert out[q, :cnt[q]].view(np.uint64).tolist() == bits.tolist(), w + ": query %d: score bits" % q
        if first is None:
            first = (idx, out, cnt)
            again = V.search_batch(queries, k, sim, flt)
            assert all(a.tobytes() == b.tobytes() for a, b in zip(first, again)), w + ": two calls differ"
            if k > 0:
                lib_scores = V.rerank_scores(queries, [idx[q, :cnt[q]] for q in range(queries.shape[0])], sim)
                for q, s in enumerate(lib_scores):
                    assert EM.canon64(s).tolist() == out[q, :cnt[q]].view(np.uint64).tolist(), w + ": query %d: against rerank_scores" % q
        else:
            assert all(a.tobytes() == b.tobytes() for a, b in zip(first, (idx, out, cnt))), w + ": the slab setting changed the answer"
    V.set_option("exact_slab_rows", 0)
    if flt is not None:
        flt.close()
    return first


# ---------------------------------------------------------------- widths, row counts, query counts, k

N_SMALL, Q_SMALL = 1000, 33


@functools.lru_cache(maxsize=None)
def _small(dim):
    rng = np.random.default_rng(5000 + dim)
    base = rng.standard_normal((N_SMALL, dim)).astype(np.float32)
    base[20:25] = base[3]          # duplicates inside a wave
    base[60:70] = base[3]          # ... and across a wave's edge
    base[250:262] = base[3]        # ... and across a slab's edge
    base[40] = 0.0                 # COSINE: 0.0
    queries = rng.standard_normal((Q_SMALL, dim)).astype(np.float32)
    queries[5] = 0.0               # COSINE's na == 0
    queries[6] = base[3]           # the duplicates lead this query's ranking under COSINE
    return _frozen(base, queries)


@functools.lru_cache(maxsize=None)
def _small_scores(dim, sim):
    base, queries = _small(dim)
    return EM.scores(queries, base, sim)


@pytest.mark.parametrize("sim", [0, 1, 2])
@pytest.mark.parametrize("dim", [1, 3, 31, 32, 33, 100, 768])
def test_widths_rows_queries_and_k(dim, sim):
    base, queries = _small(dim)
    c = _small_scores(dim, sim)
    for n in (1, 63, 64, 65, 255, 257, 1000):
        V = B.Vectors(base[:n])
        for nq in ((1, 31, 32, 33) if n == 257 else (1, 33)):
            for k in sorted({1, 10, 100, n, n + 5}):
                _check(V, c[:nq, :n], queries[:nq], sim, k, msg="dim %d" % dim)
        _check(V, c[:2, :n], queries[:2], sim, 0, msg="dim %d" % dim)
        V.close()


N_LARGE, Q_LARGE = 5000, 70


@functools.lru_cache(maxsize=None)
def _large(dim, nq):
    rng = np.random.default_rng(6000 + dim)
    base = rng.standard_normal((N_LARGE, dim)).astype(np.float32)
    base[4090:4100] = base[17]
    queries = rng.standard_normal((nq, dim)).astype(np.float32)
    return _frozen(base, queries)


@functools.lru_cache(maxsize=None)
def _large_scores(dim, nq, sim):
    base, queries = _large(dim, nq)
    return EM.scores(queries, base, sim)


@pytest.mark.parametrize("sim", [0, 1, 2])
def test_twenty_slabs_every_query_block_edge_and_k_4096(sim):
    base, queries = _large(100, Q_LARGE)
    c = _large_scores(100, Q_LARGE, sim)
    V = B.Vectors(base)
    for nq in (1, 31, 32, 33, 70):
        for k in ((10, 4096) if nq in (1, 70) else (100,)):
            _check(V, c[:nq], queries[:nq], sim, k, msg="dim 100")
    V.close()


def test_twenty_slabs_at_768_columns():
    base, queries = _large(768, 33)
    c = _large_scores(768, 33, 1)
    V = B.Vectors(base)
    for k in (10, 4096):
        _check(V, c, queries, 1, k, msg="dim 768")
    V.close()


# ---------------------------------------------------------------- order and ties


@functools.lru_cache(maxsize=None)
def _ordered(sim):
    """5000 rows and their scores for three queries, and the order of query 0's scores"""
    rng = np.random.default_rng(7000)
    base = rng.standard_normal((N_LARGE, 32)).astype(np.float32)
    queries = rng.standard_normal((3, 32)).astype(np.float32)
    c = EM.scores(queries, base, sim)
    order = np.argsort(c[0], kind="stable")
    return _frozen(base, queries) + (c, order)


@pytest.mark.parametrize("sim", [0, 1, 2])
@pytest.mark.parametrize("direction", ["ascending", "descending"])
def test_rows_stored_by_score(direction, sim):
    """ascending: every row beats the list so far, the select pass's flood; descending: nothing behind the first k passes its test"""
    base, queries, c, order = _ordered(sim)
    perm = order if direction == "ascending" else order[::-1]
    V = B.Vectors(base[perm])
    cp = np.ascontiguousarray(c[:, perm])
    assert (np.diff(cp[0]) >= 0).all() if direction == "ascending" else (np.diff(cp[0]) <= 0).all()
    for k in (1, 10, 100, 4096):
        got = _check(V, cp, queries, sim, k, msg=direction)
        if direction == "descending":
            assert sorted(got[0][0, :k].tolist()) == list(range(k))
    V.close()


@pytest.mark.parametrize("sim", [0, 1, 2])
def test_duplicated_rows_across_a_slab_edge_and_the_kth_place(sim):
    base, queries, c, order = _ordered(sim)
    rows, cc = base.copy(), c.copy()
    fifth = int(order[-5])                    # the row in fifth place for query 0: 13 copies of it take places 5 .. 17 (and more)
    for lo, hi in ((250, 263), (3000, 3005), (4990, 5000)):
        rows[lo:hi] = base[fifth]
        cc[:, lo:hi] = c[:, fifth:fifth + 1]
    V = B.Vectors(rows)
    for k in (4, 5, 10, 17, 40, 4096):
        got = _check(V, cc, queries, sim, k, msg="duplicates")
    assert set(range(250, 263)) <= set(got[0][0, :40].tolist())
    V.close()


@pytest.mark.parametrize("sim", [0, 1, 2])
def test_all_rows_identical(sim):
    base, queries, _, _ = _ordered(sim)
    rows = np.repeat(base[9:10], 600, axis=0)
    c = np.repeat(EM.scores(queries, base[9:10], sim), 600, axis=1)
    V = B.Vectors(rows)
    for k in (1, 100, 256, 257, 600, 700):
        got = _check(V, c, queries, sim, k, msg="identical rows")
        assert got[0][1, :got[2][1]].tolist() == list(range(min(k, 600)))
    V.close()


# ---------------------------------------------------------------- hostile values

N_HOSTILE = 600


@functools.lru_cache(maxsize=None)
def _hostile():
    rng = np.random.default_rng(8000)
    dim = 33
    base = rng.standard_normal((N_HOSTILE, dim)).astype(np.float32)
    base[0, 0] = np.nan
    base[100, 32] = np.nan
    base[300] = np.nan
    base[1, 5] = np.inf
    base[2, 5] = -np.inf
    base[3, 0], base[3, 32] = np.inf, -np.inf
    base[255], base[256] = np.float32(3e38), np.float32(-3e38)
    with np.errstate(over="ignore"):
        base[400:404] *= np.float32(3e38)      # most of it overflows to an infinity
    base[500] = 0.0
    queries = rng.standard_normal((7, dim)).astype(np.float32)
    queries[1, 7] = np.nan
    queries[2, 5] = np.inf
    queries[3] = np.float32(3e38)
    queries[4] *= np.float32(1e30)
    queries[5] = 0.0
    return _frozen(base, queries)


@functools.lru_cache(maxsize=None)
def _hostile_scores(sim):
    base, queries = _hostile()
    return EM.scores(queries, base, sim)


@pytest.mark.parametrize("sim", [0, 1, 2])
def test_nan_inf_and_huge_rows_and_queries(sim):
    base, queries = _hostile()
    c = _hostile_scores(sim)
    assert np.isnan(c).any() and (sim != 2 or np.isinf(c).any())
    V = B.Vectors(base)
    for k in (1, 10, 300, N_HOSTILE, N_HOSTILE + 5):
        got = _check(V, c, queries, sim, k, msg="hostile")
    nan_bits = got[1].view(np.uint64)[np.isnan(got[1])]
    assert nan_bits.size and (nan_bits == EM.NAN_BITS).all()
    mask = np.ones(N_HOSTILE, bool)
    mask[[1, 2, 300]] = False
    _check(V, c, queries, sim, 50, mask, msg="hostile, filtered")
    V.close()


# ---------------------------------------------------------------- filters


def _filter_masks(n):
    rng = np.random.default_rng(9000)
    one = np.zeros(n, bool)
    one[n - 70] = True
    block = np.zeros(n, bool)
    block[1000:1300] = True
    waves = rng.random(n) < 0.7
    waves[64:256] = False          # three whole accept words
    waves[2048:2560] = False       # two whole slabs of 256
    waves[n - 8:] = False
    return {"half": rng.random(n) < 0.5, "one percent": rng.random(n) < 0.01, "all": np.ones(n, bool), "empty": np.zeros(n, bool), "one row": one,
            "block": block, "whole waves out": waves}


@pytest.mark.parametrize("sim", [0, 1, 2])
def test_filters(sim):
    base, queries, c, _ = _ordered(sim)
    V = B.Vectors(base)
    for name, mask in _filter_masks(N_LARGE).items():
        a = int(mask.sum())
        for k in sorted({10, min(a, 4096), a + 5 if a + 5 <= 4096 else 4096}):
            _check(V, c, queries, sim, k, mask, msg="filter " + name)
    V.close()


def test_a_filter_made_for_another_row_count_is_refused():
    base, queries, _, _ = _ordered(1)
    V = B.Vectors(base[:1000])
    with capi.Filter(_index(N_LARGE), np.ones(N_LARGE, bool)) as flt:
        with pytest.raises(B.BBQError) as e:
            V.search_batch(queries, 10, 1, flt)
    assert e.value.code == capi.ERR_INVALID_ARG and "5000 rows" in str(e.value)
    V.close()


# ---------------------------------------------------------------- mutations, refusals, threads


@pytest.mark.parametrize("sim", [0, 1, 2])
def test_after_append_update_and_compact(sim):
    base, queries, c, _ = _ordered(sim)
    V = B.Vectors(base[:700])
    _check(V, np.ascontiguousarray(c[:, :700]), queries, sim, 20, msg="before")
    V.append(base[700:1000])
    assert V.n == 1000
    _check(V, np.ascontiguousarray(c[:, :1000]), queries, sim, 20, msg="after append")
    rng = np.random.default_rng(9100)
    ords = rng.choice(1000, 60, replace=False).astype(np.int32)
    src = rng.choice(np.arange(1000, N_LARGE), 60, replace=False)
    V.update(ords, base[src])
    cu = np.ascontiguousarray(c[:, :1000])
    cu[:, ords] = c[:, src]
    _check(V, cu, queries, sim, 20, msg="after update")
    mask = rng.random(1000) < 0.6
    mask[256:512] = False
    with capi.Filter(_index(1000), mask) as flt:
        V.compact(flt)
    assert V.n == int(mask.sum())
    _check(V, np.ascontiguousarray(cu[:, mask]), queries, sim, 20, msg="after compact")
    _check(V, np.ascontiguousarray(cu[:, mask]), queries, sim, V.n, msg="after compact")
    V.close()


def test_refusals():
    base, queries, _, _ = _ordered(1)
    V = B.Vectors(base)

    def code(*a, **kw):
        with pytest.raises(B.BBQError) as e:
            V.search_batch(*a, **kw)
        return e.value.code, str(e.value)

    assert code(queries, 4097)[0] == capi.ERR_UNSUPPORTED and "bbq_rerank_scores" in code(queries, 4097)[1]
    assert code(queries, 2**40)[0] == capi.ERR_UNSUPPORTED
    assert V.search_batch(queries, 4096)[2].tolist() == [4096] * 3
    m = np.zeros(N_LARGE, bool)
    m[:4097] = True
    with capi.Filter(_index(N_LARGE), m) as flt:
        assert code(queries, 5000, 1, flt)[0] == capi.ERR_UNSUPPORTED       # min(k, |A|) = 4097
        assert V.search_batch(queries, 4096, 1, flt)[2].tolist() == [4096] * 3
    m[4096] = False
    with capi.Filter(_index(N_LARGE), m) as flt:
        assert V.search_batch(queries, 5000, 1, flt)[2].tolist() == [4096] * 3   # min(k, |A|) = 4096
    assert code(queries, -1)[0] == capi.ERR_NEGATIVE_K
    bad_sim = code(queries, 10, 3)
    assert bad_sim[0] == capi.ERR_INVALID_ARG and "不支持的相似性函数: 3" in bad_sim[1]
    idx, out, cnt = V.search_batch(queries[:0], 10)
    assert idx.shape == (0, 10) and cnt.shape == (0,)
    for name, value in (("exact_slab_rows", 100), ("exact_slab_rows", 255), ("exact_slab_rows", 257), ("exact_slab_rows", -256), ("exact_slab_rows", 2**24 + 256),
                        ("exact_slab_cols", 256), ("", 0)):
        with pytest.raises(B.BBQError) as e:
            V.set_option(name, value)
        assert e.value.code == capi.ERR_INVALID_ARG
    for value in (256, 2**24, 0):
        V.set_option("exact_slab_rows", value)
    V.close()


def test_two_threads_on_one_handle():
    base, queries, c, _ = _ordered(1)
    V = B.Vectors(base)
    want = {k: [EM.topk(c[q], k) for q in range(3)] for k in (7, 300)}
    bad = []

    def work(k, slab):
        for _ in range(10):
            V.set_option("exact_slab_rows", slab)      # the other thread may set it back: it never changes an answer
            idx, out, cnt = V.search_batch(queries, k, 1)
            for q, (rows, bits) in enumerate(want[k]):
                if cnt[q] != k or idx[q].tolist() != rows.tolist() or out[q].view(np.uint64).tolist() != bits.tolist():
                    bad.append((k, q))

    threads = [threading.Thread(target=work, args=a) for a in ((7, 256), (300, 0))]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not bad
    V.close()
