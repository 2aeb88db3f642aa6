"""GPU: the exact search behind its f32 prefilter on the matrix cores - byte for byte, no tolerance.  Every case runs with
exact_prefilter 1 against the model of tests/exact_model.py and against the same call with exact_prefilter 0, with exact_slab_rows 256
and automatic; the read-out tells pruning from falling back.  COSINE and MAXIMUM_INNER_PRODUCT: EUCLIDEAN has no prefilter."""
import functools

import numpy as np
import pytest

import exact_model as EM
from bbqlib import bbq_amd as B, capi

pytestmark = pytest.mark.gpu

SIMS = [1, 2]


@functools.lru_cache(maxsize=None)
def _index(n):
    """an index of n rows for the filters to hang on"""
    rng = np.random.default_rng(7 + n)
    codes, corr, cen = B.quantize_vectors(rng.standard_normal((n, 64)).astype(np.float32), 1)
    return B.Index(codes, corr, 64, B.centroid_dp(cen))


def _check(V, c, queries, sim, k, mask=None, msg=""):
    """prefilter 1 and 0 under both slab settings, each held to the model; returns the read-outs of prefilter 1 by slab setting"""
    want = [EM.topk(c[q], k, mask) for q in range(queries.shape[0])]
    flt = capi.Filter(_index(V.n), mask) if mask is not None else None
    stats = {}
    for slab in (256, 0):
        V.set_option("exact_slab_rows", slab)
        for pre in (1, 0):
            V.set_option("exact_prefilter", pre)
            idx, out, cnt = V.search_batch(queries, k, sim, flt)
            st = V.exact_stats()
            w = "%s, sim %d, %d rows, %d queries, k %d, slab %d, prefilter %d" % (msg, sim, V.n, queries.shape[0], k, slab, pre)
            for q, (rows, bits) in enumerate(want):
                assert cnt[q] == rows.shape[0], w + ": query %d: count" % q
                assert idx[q, :cnt[q]].tolist() == rows.tolist(), w + ": query %d: rows" % q
                assert out[q, :cnt[q]].view(np.uint64).tolist() == bits.tolist(), w + ": query %d: score bits" % q
            if pre:
                stats[slab], first = st, (idx, out, cnt)
                assert k == 0 or cnt.max() == 0 or st["prefilter_pairs"] > 0, w + ": the prefilter did not run"
            else:
                assert st["prefilter_pairs"] == 0 and st["fallbacks"] == 0, w
                assert all(a.tobytes() == b.tobytes() for a, b in zip(first, (idx, out, cnt))), w + ": the prefilter changed the answer"
    V.set_option("exact_slab_rows", 0)
    V.set_option("exact_prefilter", -1)
    if flt is not None:
        flt.close()
    return stats


@functools.lru_cache(maxsize=None)
def _small(dim):
    rng = np.random.default_rng(5000 + dim)
    base = rng.standard_normal((1000, dim)).astype(np.float32)
    base[20:25] = base[3]          # duplicates inside a wave
    base[60:70] = base[3]          # ... across a wave's edge
    base[250:262] = base[3]        # ... across a slab's edge; with query 6 they hold the k-th place too
    base[40] = 0.0
    base[101] = base[100]          # one f32 ulp apart in one component: f32 cannot tell their scores apart, the f64 bits rank them
    base[101, 0] = np.nextafter(base[100, 0], np.float32(np.inf))
    queries = rng.standard_normal((65, dim)).astype(np.float32)
    queries[5] = 0.0
    queries[6] = base[3]
    queries[7] = base[100]
    return base, queries


@functools.lru_cache(maxsize=None)
def _small_scores(dim, sim):
    return EM.scores(_small(dim)[1], _small(dim)[0], sim)


@pytest.mark.parametrize("sim", SIMS)
@pytest.mark.parametrize("dim", [1, 3, 33, 100, 768])
def test_widths_rows_queries_and_k(dim, sim):
    base, queries = _small(dim)
    c = _small_scores(dim, sim)
    for n in ((1000,) if dim == 768 else (1, 63, 65, 257, 1000)):
        V = B.Vectors(base[:n])
        for nq in ((1, 33, 65) if n in (257, 1000) else (33,)):
            for k in sorted({1, 10, n, n + 5}) if nq == 33 else (10,):
                _check(V, c[:nq, :n], queries[:nq], sim, k, msg="dim %d" % dim)
        V.close()


@pytest.mark.parametrize("sim", SIMS)
def test_hostile_rows_and_queries(sim):
    rng = np.random.default_rng(8100)
    base = (rng.standard_normal((300, 33)) * 1e-3).astype(np.float32)
    base[10], base[70], base[130] = 1e-30, 1e-40, 3e38
    base[11] *= np.float32(1e23)   # one row 1e20 among rows of 1e-3
    base[64, 5], base[65, 5], base[200, 32] = np.inf, -np.inf, np.nan
    base[256] = 0.0
    queries = rng.standard_normal((6, 33)).astype(np.float32)
    queries[1] = 0.0
    queries[2] *= np.float32(1e-30)
    queries[3, 7] = np.nan
    queries[4] = 3e38
    c = EM.scores(queries, base, sim)
    V = B.Vectors(base)
    for k in (1, 10, 300):
        _check(V, c, queries, sim, k, msg="hostile")
    V.close()


@pytest.mark.parametrize("sim", SIMS)
def test_filters_and_k_4096(sim):
    rng = np.random.default_rng(8200)
    base = rng.standard_normal((5000, 33)).astype(np.float32)
    queries = rng.standard_normal((34, 33)).astype(np.float32)
    c = EM.scores(queries, base, sim)
    V = B.Vectors(base)
    one = np.zeros(5000, bool)
    one[4321] = True
    gap = np.ones(5000, bool)
    gap[2560:2624] = False          # an empty wave in the middle
    for name, mask in (("all", np.ones(5000, bool)), ("one row", one), ("empty wave", gap), ("random 10 %", rng.random(5000) < 0.1)):
        _check(V, c, queries, sim, 10, mask, msg=name)
    _check(V, c[:2], queries[:2], sim, 4096, msg="kk 4096")
    V.close()


def test_after_append_update_and_compact():
    base, queries = (a.copy() for a in _small(33))
    extra = np.random.default_rng(8300).standard_normal((300, 33)).astype(np.float32)
    V = B.Vectors(base)
    V.append(extra)
    rows = np.concatenate([base, extra])
    _check(V, EM.scores(queries, rows, 1), queries, 1, 10, msg="append")
    V.update([3, 1299], extra[:2])
    rows[[3, 1299]] = extra[:2]
    _check(V, EM.scores(queries, rows, 1), queries, 1, 10, msg="update")
    keep = np.arange(1300) % 3 != 0
    flt = capi.Filter(_index(1300), keep)
    V.compact(flt)
    flt.close()
    _check(V, EM.scores(queries, rows[keep], 1), queries, 1, 10, msg="compact")
    V.close()


@pytest.mark.parametrize("sim", SIMS)
@pytest.mark.parametrize("dim", [33, 100, 768])
def test_the_prefilter_prunes_and_does_not_fall_back(dim, sim):
    """conditions on the read-out: at one slab a query scores at most 2 k + 16 pairs in f64, at slabs of 256 at most 625 - an eighth
    of the rows; on the CPU, with the library's bound and numpy's f32 dot products, the most were k + 4 and 406"""
    rng = np.random.default_rng(5000 + dim)
    base = rng.standard_normal((5000, dim)).astype(np.float32)
    queries = rng.standard_normal((70, dim)).astype(np.float32)
    c = EM.scores(queries, base, sim)
    V = B.Vectors(base)
    for k in (10, 100):
        st = _check(V, c, queries, sim, k, msg="read-out, dim %d" % dim)
        print("dim %d sim %d k %d: %r" % (dim, sim, k, st))
        for slab, most in ((0, 2 * k + 16), (256, 625)):
            assert st[slab]["fallbacks"] == 0 and st[slab]["prefilter_pairs"] == 70 * 5000, (slab, st[slab])
            assert k <= st[slab]["f64_pairs_max_query"] <= most and st[slab]["f64_pairs"] <= 70 * most, (slab, st[slab])
    V.close()


def test_identical_rows_fall_back_and_bad_option_values():
    rng = np.random.default_rng(8400)
    base = np.repeat(rng.standard_normal((1, 33)).astype(np.float32), 8192, axis=0)
    queries = rng.standard_normal((3, 33)).astype(np.float32)
    c = np.repeat(EM.scores(queries, base[:1], 1), 8192, axis=1)
    V = B.Vectors(base)
    st = _check(V, c, queries, 1, 10, msg="identical rows")
    assert st[0]["fallbacks"] == 1 and st[256]["fallbacks"] == 1 and st[0]["f64_pairs"] == 3 * 8192, st
    for bad in (-2, 2):
        with pytest.raises(capi.BBQError) as e:
            V.set_option("exact_prefilter", bad)
        assert e.value.code == capi.ERR_INVALID_ARG
    V.set_option("exact_prefilter", 1)
    V.search_batch(queries, 10, 0)   # EUCLIDEAN: the f64 sweep, whatever the option says
    assert V.exact_stats()["prefilter_pairs"] == 0
    V.close()
