"""GPU: option fast_bound - the compact layout's score bound as an f32 test against the threshold's z image (1, the default) or
through the f64 similarity transform (0) - changes no answer.

The criterion everywhere: search results with fast_bound 1 and 0 are identical to each other and to heap_topk of the oracle's
scores - indices, f32 score BITS and counts.  No tolerances."""
import functools

import numpy as np
import pytest

import orclib as O
from bbqlib import bbq_amd as B, capi

pytestmark = pytest.mark.gpu

CDP = 0.0009


def bits32(a):
    a = np.array(a, np.float32)
    a[np.isnan(a)] = np.nan
    return a.view(np.uint32)


def _rows(seed, n, dim, ib=1):
    """random codes and the corrections a real COSINE index shows (bench.py's synth_rows)"""
    rng = np.random.default_rng(seed)
    if ib == 1:
        codes = rng.integers(0, 256, size=(n, (dim + 7) // 8), dtype=np.uint8)
        if dim % 8:
            codes[:, -1] &= (0xFF << (8 - dim % 8)) & 0xFF
        x1 = np.unpackbits(codes, axis=1).sum(axis=1)
    else:
        codes = rng.integers(0, 1 << ib, size=(n, dim), dtype=np.uint8)
        x1 = codes.sum(axis=1)
    corr = np.empty((n, 4))
    corr[:, 0] = -0.04 * (0.9 + 0.2 * rng.random(n))
    corr[:, 1] = 0.04 * (0.9 + 0.2 * rng.random(n))
    corr[:, 2] = 1e-4 * (2 * rng.random(n) - 1)
    corr[:, 3] = x1
    return codes, corr


def _queries(seed, nq, dim, qb):
    rng = np.random.default_rng(seed)
    qq = rng.integers(0, 1 << qb, size=(nq, dim), dtype=np.uint8)
    qc = np.empty((nq, 4))
    qc[:, 0] = -0.15 * (0.9 + 0.2 * rng.random(nq))
    qc[:, 1] = 0.148 * (0.9 + 0.2 * rng.random(nq))
    qc[:, 2] = -0.0028 * rng.random(nq)
    qc[:, 3] = qq.sum(axis=1)
    return qq, qc


def _scores(codes, corr, dim, qq, qc, qb, sim, ib=1):
    out = []
    for q in range(len(qq)):
        if ib == 1:
            s32 = O.score_all(codes, corr, dim, qq[q], qc[q], qb, sim, CDP)[2]
        elif qb in (1, 4):
            s32 = O.score_all(codes, corr, dim, qq[q], qc[q], qb, sim, CDP, ib=ib)[2]
        else:   # the reference throws for this queryBits on a multi-bit index: libbbq's documented extension
            s32 = O.score_all_multibit_ext(codes, corr, dim, qq[q], qc[q], qb, sim, CDP)[2]
        out.append(s32)
    return out


def _want(s32, k, mask=None):
    if mask is None:
        return O.heap_topk(s32, k)
    acc = np.flatnonzero(mask)
    pos, sc = O.heap_topk(s32[acc], k)
    return acc[pos].astype(np.int32), sc


def _index(codes, corr, dim, ib=1):
    ix = B.Index(codes, corr, dim, CDP, index_bits=ib, corrections="compact")
    ix.set_option("first_segment_rows", 1024)   # many segments: the threshold - and its z image - is rewritten many times
    ix.set_option("segment_growth", 2)
    return ix


def _check(ix, run, want):
    """run() -> (idx [nq][k], scores, counts): fast_bound 1 equals `want`, fast_bound 0 equals fast_bound 1"""
    first = None
    for fast in (1, 0):
        ix.set_option("fast_bound", fast)
        idx, sc, cnt = run()
        if first is None:
            first = (idx, bits32(sc), cnt)
            for q, (wi, ws) in enumerate(want):
                assert cnt[q] == len(wi), "fast_bound 1, query %d" % q
                np.testing.assert_array_equal(idx[q, :cnt[q]], wi, err_msg="fast_bound 1, query %d" % q)
                np.testing.assert_array_equal(bits32(sc[q, :cnt[q]]), bits32(ws), err_msg="fast_bound 1, query %d" % q)
        else:
            np.testing.assert_array_equal(cnt, first[2], err_msg="fast_bound 0")
            np.testing.assert_array_equal(idx, first[0], err_msg="fast_bound 0")
            np.testing.assert_array_equal(bits32(sc), first[1], err_msg="fast_bound 0")
    ix.set_option("fast_bound", 1)


# 768-d (six 16-byte chunks per row: the headline kernel's instantiation) x 20 480 rows, computed once and never changed
@functools.lru_cache(maxsize=None)
def _base768():
    codes, corr = _rows(3, 20_480, 768)
    for a in (codes, corr):
        a.setflags(write=False)
    return codes, corr


@pytest.mark.parametrize("sim", [0, 1, 2])
@pytest.mark.parametrize("qb", [1, 4])
def test_768d_many_thresholds(sim, qb):
    codes, corr = _base768()
    qq, qc = _queries(10 * sim + qb, 8, 768, qb)
    want = [_want(s, 10) for s in _scores(codes, corr, 768, qq, qc, qb, sim)]
    ix = _index(codes, corr, 768)
    try:
        _check(ix, lambda: ix.search_batch(qq, qc, qb, sim, 10), want)
        assert ix.stats()["dense_fallbacks"] == 0
    finally:
        ix.close()


def test_run_time_row_width():
    codes, corr = _rows(4, 5_000, 200)
    qq, qc = _queries(41, 8, 200, 4)
    want = [_want(s, 10) for s in _scores(codes, corr, 200, qq, qc, 4, 1)]
    ix = _index(codes, corr, 200)
    try:
        _check(ix, lambda: ix.search_batch(qq, qc, 4, 1, 10), want)
    finally:
        ix.close()


def _hostile(seed, n, dim, sim):
    """corrections over 1e-12 .. 1e6, zeros, and rows whose upper interval lies below the lower"""
    rng = np.random.default_rng(seed)
    codes = rng.integers(0, 256, size=(n, dim // 8), dtype=np.uint8)
    corr = np.zeros((n, 4))
    scale = 10.0 ** rng.uniform(-12, 6, n)
    corr[:, 0] = rng.standard_normal(n) * scale
    corr[:, 1] = rng.standard_normal(n) * scale * 10.0 ** rng.uniform(-2, 2, n)
    corr[:, 2] = rng.standard_normal(n) * 10.0 ** rng.uniform(-10, 6, n)
    corr[::101, 0] = 0
    corr[::103, 1] = 0
    corr[::107, 2] = 0
    flip = np.arange(n) % 5 == 0
    lo, hi = np.minimum(corr[:, 0], corr[:, 1]), np.maximum(corr[:, 0], corr[:, 1])
    corr[flip, 0], corr[flip, 1] = hi[flip], lo[flip]      # upper < lower
    corr[:, 3] = np.unpackbits(codes, axis=1).sum(axis=1)
    return codes, corr


@pytest.mark.parametrize("sim", [0, 1, 2])
@pytest.mark.parametrize("nonfinite", [False, True])
def test_hostile_corrections(sim, nonfinite):
    """sim 0 has rows with 1 + e <= 0 (score +0 or huge), sim 2 rows with t < 0 (the reciprocal branch), sim 1 rows clamped to +0"""
    n, dim, k = 20_000, 96, 10
    codes, corr = _hostile(50 + sim, n, dim, sim)
    if nonfinite:   # rows no bound exists for: they must reach the exact path; a NaN score sends the query to the dense path
        corr[3000, 1] = np.inf
        corr[7000, 0] = -np.inf
        corr[9000, 2] = np.inf
        corr[11000, 1] = 1e300
        corr[15000, 0] = np.nan
        corr[17000, 2] = np.nan
    qq, qc = _queries(60 + sim, 8, dim, 4)
    qc[4:, 0] *= 30.0   # a second query scale
    qc[4:, 1] *= 30.0
    s32 = _scores(codes, corr, dim, qq, qc, 4, sim)
    if sim == 0 and not nonfinite:
        e = [O.score_all(codes, corr, dim, qq[0], qc[0], 4, sim, CDP)[1]]
        assert (e[0] == 0.0).any(), "EUCLIDEAN rows with 1 + e <= 0"
    ix = _index(codes, corr, dim)
    try:
        _check(ix, lambda: ix.search_batch(qq, qc, 4, sim, k), [_want(s, k) for s in s32])
    finally:
        ix.close()


def test_kth_score_is_plus_zero_under_cosine():
    """all but a few rows are clamped to +0: the threshold becomes the key of +0, whose z image is t > -1"""
    n, dim, k = 8_192, 96, 10
    codes, corr = _rows(7, n, dim)
    corr[:, 2] = -5.0                      # (1 + t) / 2 < 0 -> +0
    corr[[100, 2000, 4000, 6000, 8000], 2] = 1e-4
    qq, qc = _queries(71, 4, dim, 4)
    s32 = _scores(codes, corr, dim, qq, qc, 4, 1)
    assert all((s == 0.0).sum() == n - 5 for s in s32)
    ix = _index(codes, corr, dim)
    try:
        _check(ix, lambda: ix.search_batch(qq, qc, 4, 1, k), [_want(s, k) for s in s32])
    finally:
        ix.close()


def test_negative_mip_scores():
    """t < 0 for every row: scaleMaxInnerProductScore's reciprocal branch, thresholds below 1"""
    n, dim, k = 8_192, 96, 10
    codes, corr = _rows(8, n, dim)
    corr[:, 2] -= 3.0
    qq, qc = _queries(81, 4, dim, 4)
    s32 = _scores(codes, corr, dim, qq, qc, 4, 2)
    assert all((s < 1.0).all() for s in s32)
    ix = _index(codes, corr, dim)
    try:
        _check(ix, lambda: ix.search_batch(qq, qc, 4, 2, k), [_want(s, k) for s in s32])
    finally:
        ix.close()


@pytest.mark.parametrize("scale", [1e60, 1e-60])
@pytest.mark.parametrize("sim", [0, 1, 2])
def test_query_corrections_outside_f32(scale, sim):
    """such a query has no f32 images: it keeps the f64 bound whatever the option says"""
    codes, corr = _base768()
    codes, corr = codes[:8192], corr[:8192]
    qq, qc = _queries(90 + sim, 4, 768, 4)
    qc[:2, 0] *= scale    # two queries outside, two ordinary ones in the same launch
    qc[:2, 1] *= scale
    want = [_want(s, 10) for s in _scores(codes, corr, 768, qq, qc, 4, sim)]
    ix = _index(codes, corr, 768)
    try:
        _check(ix, lambda: ix.search_batch(qq, qc, 4, sim, 10), want)
    finally:
        ix.close()


@pytest.mark.parametrize("qb", [4, 8])
def test_two_bit_rows(qb):
    n, dim, ib = 4_096, 1024, 2
    codes, corr = _rows(9, n, dim, ib)
    qq, qc = _queries(91 + qb, 8, dim, qb)
    want = [_want(s, 10) for s in _scores(codes, corr, dim, qq, qc, qb, 1, ib)]
    ix = _index(codes, corr, dim, ib)
    try:
        _check(ix, lambda: ix.search_batch(qq, qc, qb, 1, 10), want)
    finally:
        ix.close()


@pytest.mark.parametrize("share", [4, 8])
def test_shared_sweep(share):
    codes, corr = _base768()
    qq, qc = _queries(100 + share, 8, 768, 4)
    want = [_want(s, 10) for s in _scores(codes, corr, 768, qq, qc, 4, 1)]
    ix = _index(codes, corr, 768)
    try:
        ix.set_option("sweep_share", share)
        _check(ix, lambda: ix.search_batch(qq, qc, 4, 1, 10), want)
    finally:
        ix.close()


def test_filtered_search():
    codes, corr = _base768()
    qq, qc = _queries(110, 8, 768, 4)
    mask = np.random.default_rng(111).random(len(corr)) < 0.3
    want = [_want(s, 10, mask) for s in _scores(codes, corr, 768, qq, qc, 4, 1)]
    ix = _index(codes, corr, 768)
    try:
        with capi.Filter(ix, mask) as flt:
            _check(ix, lambda: ix.search_filtered_batch(qq, qc, 4, 1, 10, flt), want)
    finally:
        ix.close()


def test_single_query_presampled_path():
    """262 144 rows: the single-query call samples its threshold from a prefix (bbq_lat_select_kernel writes it) and sweeps once"""
    n, dim, k = 262_144, 768, 10
    codes, corr = _rows(12, n, dim)
    qq, qc = _queries(121, 1, dim, 4)
    want = [_want(s, k) for s in _scores(codes, corr, dim, qq, qc, 4, 1)]
    ix = B.Index(codes, corr, dim, CDP, corrections="compact")
    try:
        _check(ix, lambda: ix.search_batch(qq, qc, 4, 1, k), want)
        ix.set_option("latency_presample", 0)   # ... and the segmented single-query chain (bbq_finalize_kernel writes the thresholds)
        _check(ix, lambda: ix.search_batch(qq, qc, 4, 1, k), want)
    finally:
        ix.close()


def test_option_validation():
    codes, corr = _base768()
    ix = B.Index(codes[:1024], corr[:1024], 768, CDP)
    try:
        for bad in (-1, 2):
            with pytest.raises(capi.BBQError) as e:
                ix.set_option("fast_bound", bad)
            assert e.value.code == capi.ERR_INVALID_ARG
        ix.set_option("fast_bound", 0)
        ix.set_option("fast_bound", 1)
    finally:
        ix.close()
