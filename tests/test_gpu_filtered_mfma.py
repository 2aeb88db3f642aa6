"""GPU: filtered search on the shared sweep on the matrix cores (sweep_share 32 + bbq_search_filtered_batch: the filtered family of
bbq_scan_mfma_kernel) against the oracle.  The contract is test_gpu_filtered.py's: the answer is the oracle's heap over the accepted
rows' scores, ascending ord, mapped back to ords - bit-exact in ords, f32 score bits and order, no tolerance anywhere.  Rows and
queries are built as test_matrix_core_sweep_hostile_rows_and_queries (test_gpu_parity.py) builds them; every index runs with
sweep_share 32, first_segment_rows 1024, segment_growth 4, and a call has 70 queries (three groups of 32, the last one partial)
unless a test says otherwise; k = 50."""
import functools

import numpy as np
import pytest

import orclib as O
from bbqlib import bbq_amd as B, capi
from test_gpu_filtered import assert_same, expected

pytestmark = pytest.mark.gpu

K, NQ, N = 50, 70, 40000


def _rows(rng, n, dim, sim, hostile):
    codes = rng.integers(0, 256, size=(n, dim // 8), dtype=np.uint8)
    pop = np.unpackbits(codes, axis=1).sum(axis=1).astype(np.float64)
    corr = np.zeros((n, 4))
    corr[:, 0] = -0.04 * (0.9 + 0.2 * rng.random(n))
    corr[:, 1] = 0.04 * (0.9 + 0.2 * rng.random(n))
    corr[:, 2] = np.abs(rng.standard_normal(n)) * 1e-2 if sim == 0 else 1e-3 * rng.standard_normal(n)
    weird = np.zeros(0, np.int64)
    if hostile:  # the recipe of the hostile test, on a tenth of the rows
        h = rng.choice(n, n // 10, replace=False)
        m = len(h) // 12
        scale = 10.0 ** rng.uniform(-6, 3, len(h))
        corr[h, 0] = -scale * rng.uniform(0.1, 1.0, len(h))
        corr[h, 1] = scale * rng.uniform(0.1, 1.0, len(h))
        corr[h[:m], 1] = corr[h[:m], 0]                                       # zero width
        corr[h[m:2 * m], 1] = corr[h[m:2 * m], 0] - 0.01                      # negative width
        corr[h[2 * m:3 * m], 1] = corr[h[2 * m:3 * m], 0] * (1 - 2.0 ** -30)  # a width lost in f32
        corr[h[3 * m:3 * m + 100], 1] = 1e300                                 # overflows f32
        corr[h[3 * m + 100:3 * m + 200], 2] = 3.0e38
        corr[h[3 * m + 200:3 * m + 300], 0] = -1e-320                         # f64 subnormal
        corr[h[3 * m + 300:4 * m + 300], 2] = rng.standard_normal(m) * 1e4
        weird = h[:3 * m + 300]
    corr[:, 3] = pop
    return codes, corr, weird


def _queries(rng, nq, dim, qb, sim):
    qq = rng.integers(0, 1 << qb, size=(nq, dim), dtype=np.uint8)
    qc = np.empty((nq, 4))
    qc[:, 0] = -0.15 * (0.9 + 0.2 * rng.random(nq))
    qc[:, 1] = 0.148 * (0.9 + 0.2 * rng.random(nq))
    qc[:, 2] = 0.7 * rng.random(nq) if sim == 0 else -0.0028 * rng.random(nq)
    qc[:, 3] = qq.sum(axis=1)
    qc[5, 3] *= 0.25                                                          # a quantizedComponentSum that is not the sum of the values
    return qq, qc


CDP = 0.02


def _scores(codes, corr, dim, qq, qc, qb, sim):
    return [O.score_all(codes, corr, dim, qq[q], qc[q], qb, sim, CDP)[2] for q in range(qq.shape[0])]


@functools.lru_cache(maxsize=2)
def _case(sim, qb, dim, n=N, nq=NQ, hostile=False):
    """rows, queries and every query's oracle scores: built once per shape and shared by the layouts (and tests) that sweep it"""
    rng = np.random.default_rng(7000 * sim + 10 * qb + dim + (1 if hostile else 0))
    codes, corr, weird = _rows(rng, n, dim, sim, hostile)
    qq, qc = _queries(rng, nq, dim, qb, sim)
    s32 = _scores(codes, corr, dim, qq, qc, qb, sim)
    for a in (codes, corr, qq, qc, *s32):
        a.setflags(write=False)
    return codes, corr, weird, qq, qc, s32


def random_tiles(rng, n):
    """each 64-row tile kept with probability 0.3, inside a kept tile each row with probability 0.5: empty tiles in front of and behind
    live ones for every wave slot"""
    tiles = (n + 63) // 64
    keep = np.repeat(rng.random(tiles) < 0.3, 64)[:n]
    return keep & (rng.random(n) < 0.5)


def _masks(n, s32, seed):
    rng = np.random.default_rng(seed)
    m = {"ones": np.ones(n, bool), "random_50": rng.random(n) < 0.5, "first_half": np.arange(n) < n // 2,
         "last_10pct": np.arange(n) >= n - n // 10, "random_tiles": random_tiles(rng, n)}
    m["not_top"] = np.ones(n, bool)   # rejected rows that beat every accepted one: every query's unfiltered top 20
    for s in s32:
        m["not_top"][O.heap_topk(s, 20)[0]] = False
    return m


def _open(codes, corr, dim, compact, **opts):
    ix = B.Index(codes, corr, dim, CDP, corrections="compact" if compact else "inline")
    for name, v in dict({"sweep_share": 32, "first_segment_rows": 1024, "segment_growth": 4}, **opts).items():
        ix.set_option(name, v)
    return ix


def _check(ix, flt, mask, qq, qc, s32, qb, sim, k, msg):
    idx, sc, cnt = ix.search_filtered_batch(qq, qc, qb, sim, k, flt)
    for q in range(qq.shape[0]):
        assert_same((idx[q, :cnt[q]], sc[q, :cnt[q]]), expected(s32[q], mask, k), "%s q%d" % (msg, q))


# every (form, W, layout) instantiation: FP (query values <= 15) and int8 at W = 1, 6, 8, 12.  The 1536-d shapes run all three
# similarities in the compact layout and one in the inline layout (their oracle scores cost the most)
SHAPES = [(4, 768), (2, 128), (4, 1024), (4, 1536), (7, 768), (7, 1536)]
GRID = [(qb, dim, sim, compact) for qb, dim in SHAPES for sim in (0, 1, 2) for compact in (True, False)
        if dim != 1536 or compact or sim == 1]


@pytest.mark.parametrize("qb,dim,sim,compact", GRID)
def test_parity_over_forms_layouts_and_masks(qb, dim, sim, compact):
    codes, corr, _, qq, qc, s32 = _case(sim, qb, dim)
    ix = _open(codes, corr, dim, compact)
    try:
        for mname, mask in _masks(N, s32, 11).items():
            with capi.Filter(ix, mask) as flt:
                _check(ix, flt, mask, qq, qc, s32, qb, sim, K, "%s qb%d %dd sim%d compact=%s" % (mname, qb, dim, sim, compact))
        assert ix.stats()["dense_fallbacks"] == 0
    finally:
        ix.close()


@pytest.mark.parametrize("compact", [True, False])
@pytest.mark.parametrize("qb,dim,sim", [(4, 768, 1), (7, 768, 0), (4, 128, 2)])
def test_hostile_rows_half_of_them_rejected(qb, dim, sim, compact):
    """zero, negative and lost widths, 1e300, 3e38, subnormal: under random_50 half of the weird rows are rejected - a rejected weird
    row gets pass_none, not pass_all, and must not show"""
    codes, corr, weird, qq, qc, s32 = _case(sim, qb, dim, hostile=True)
    assert not any(np.isnan(s).any() for s in s32)
    mask = np.random.default_rng(13).random(N) < 0.5
    assert 0 < mask[weird].sum() < len(weird)
    ix = _open(codes, corr, dim, compact)
    try:
        with capi.Filter(ix, mask) as flt:
            _check(ix, flt, mask, qq, qc, s32, qb, sim, K, "hostile qb%d %dd sim%d compact=%s" % (qb, dim, sim, compact))
    finally:
        ix.close()


@pytest.mark.parametrize("compact", [True, False])
def test_nan_rows_rejected_and_then_accepted(compact):
    """NaN in a correction of 200 rows, all of them rejected: never scored, so no flag and no dense fallback.  Then 20 of them are
    accepted: the answers are whatever the oracle's heap makes of NaN scores"""
    sim, qb, dim = 1, 4, 768
    codes, corr, _, qq, qc, _ = _case(sim, qb, dim)
    rng = np.random.default_rng(17)
    corr = corr.copy()
    nan_rows = rng.choice(np.arange(2048, N), 200, replace=False)   # behind the first segments: in tiles the matrix cores sweep
    corr[nan_rows[:100], 2] = np.nan
    corr[nan_rows[100:], 1] = np.nan
    s32 = _scores(codes, corr, dim, qq, qc, qb, sim)
    assert all(np.isnan(s[nan_rows]).all() for s in s32)
    mask = rng.random(N) < 0.5
    mask[nan_rows] = False
    ix = _open(codes, corr, dim, compact)
    try:
        with capi.Filter(ix, mask) as flt:
            _check(ix, flt, mask, qq, qc, s32, qb, sim, K, "NaN rows rejected, compact=%s" % compact)
            assert ix.stats()["dense_fallbacks"] == 0
        mask[nan_rows[:10]] = True
        mask[nan_rows[100:110]] = True
        with capi.Filter(ix, mask) as flt:
            _check(ix, flt, mask, qq, qc, s32, qb, sim, K, "20 NaN rows accepted, compact=%s" % compact)
    finally:
        ix.close()


@pytest.mark.parametrize("compact", [True, False])
def test_a_query_the_kernel_refuses(compact):
    """a query of zero interval width cannot be swept on the matrix cores (the threshold divides by it): its sub-batch falls back to
    the per-query filtered sweep, with the same answers"""
    sim, qb, dim = 1, 4, 768
    codes, corr, _, qq, qc, s32 = _case(sim, qb, dim)
    qz = qc.copy()
    qz[3, 1] = qz[3, 0]
    sz = list(s32)
    sz[3] = O.score_all(codes, corr, dim, qq[3], qz[3], qb, sim, CDP)[2]
    mask = np.random.default_rng(19).random(N) < 0.5
    ix = _open(codes, corr, dim, compact)
    try:
        with capi.Filter(ix, mask) as flt:
            _check(ix, flt, mask, qq, qz, sz, qb, sim, K, "zero-width query, compact=%s" % compact)
    finally:
        ix.close()


def test_walking_chunks_across_skipped_tiles():
    """128-d, 300 000 rows, 100 queries in one sub-batch (batch_queries 128), segment_growth 8, mask random_tiles (15 % of the rows, 70 %
    of the tiles empty).  Chunks are 512 rows, so the index has 586.  The accepted-space plan with k_dev = 51: the first segment ends
    behind 1024 accepted rows (about chunk 14), the second behind 8 x 1024 (about chunk 107), and as 8 x 8192 is beyond half of the
    45 000 accepted rows the last one takes the rest, about 479 chunks.  Its chunk slots hold cap_for(51, 8192) = 40 <= 64 entries,
    so a workgroup serves G = 2 groups; 100 queries are 4 groups, and by launch_mfma_t's rule units = chunks x ceil(groups / G) =
    479 x 2 = 958 > 512: chunks_per_block = ceil(958 / 512) = 2.  Every workgroup of the last segment walks two chunks, each wave from
    its first tile with an accepted row to the next one - across tiles without any."""
    sim, qb, dim, n, nq = 1, 4, 128, 300000, 100
    codes, corr, _, qq, qc, s32 = _case(sim, qb, dim, n, nq)
    mask = random_tiles(np.random.default_rng(23), n)
    assert (n + 511) // 512 == 586 and 40000 < mask.sum() < 50000
    ix = _open(codes, corr, dim, True, segment_growth=8, batch_queries=128)
    try:
        with capi.Filter(ix, mask) as flt:
            _check(ix, flt, mask, qq, qc, s32, qb, sim, K, "walking chunks")
        assert ix.stats()["dense_fallbacks"] == 0
    finally:
        ix.close()


def test_few_accepted_rows_and_a_rank_beyond_the_first_segment():
    """600 accepted rows, fewer than the first segment: the plan is that segment alone and nothing reaches the matrix cores.  And
    k = 1024 under random_50: the rank the device selects with lies beyond first_segment_rows, so the first segment grows to hold it
    and no later segment is swept before k_dev accepted rows have been seen.  The answers are the oracle's either way."""
    sim, qb, dim = 1, 4, 768
    codes, corr, _, qq, qc, s32 = _case(sim, qb, dim)
    rng = np.random.default_rng(29)
    few = np.zeros(N, bool)
    few[rng.choice(N, 600, replace=False)] = True
    half = rng.random(N) < 0.5
    ix = _open(codes, corr, dim, True)
    try:
        with capi.Filter(ix, few) as flt:
            _check(ix, flt, few, qq, qc, s32, qb, sim, K, "600 accepted rows")
        with capi.Filter(ix, half) as flt:
            _check(ix, flt, half, qq[:40], qc[:40], s32[:40], qb, sim, 1024, "k = 1024")
    finally:
        ix.close()


@pytest.mark.parametrize("compact", [True, False])
def test_the_filtered_call_ran_on_the_matrix_cores(compact):
    """One call of exactly 64 queries, one sub-batch, mask random_50, 768-d: the dominant launch reports the bytes of a sweep that loads
    every tile once for S = 64 (two groups per tile load) or 32 queries - 16 x 6 code bytes + 24 bytes of exact corrections per row in
    the compact layout, the tile record's bytes per row in the inline layout: 1.875 or 3.75 bytes per (row, query).  The per-query
    sweep reports bytes_per_row (100) per (row, query): that figure comes back with sweep_share 1, and is what this call reported
    before the filtered kernels existed."""
    sim, qb, dim, nq = 1, 4, 768, 64
    codes, corr, _, qq, qc, s32 = _case(sim, qb, dim)
    mask = np.random.default_rng(31).random(N) < 0.5
    ix = _open(codes, corr, dim, compact, batch_queries=64)
    try:
        row_bytes = 16 * 6 + 24 if compact else ix.bytes_per_row
        with capi.Filter(ix, mask) as flt:
            _check(ix, flt, mask, qq[:nq], qc[:nq], s32[:nq], qb, sim, K, "64 queries, compact=%s" % compact)
            st = ix.stats()
            print("sweep_share 32: last_scan_rows %d last_scan_bytes %d" % (st["last_scan_rows"], st["last_scan_bytes"]))
            assert st["last_scan_rows"] > 0 and st["last_scan_rows"] % 64 == 0
            assert st["last_scan_bytes"] in [(st["last_scan_rows"] // 64) * ((64 + S - 1) // S) * row_bytes for S in (64, 32)]
            ix.set_option("sweep_share", 1)
            _check(ix, flt, mask, qq[:nq], qc[:nq], s32[:nq], qb, sim, K, "64 queries, sweep_share 1, compact=%s" % compact)
            st = ix.stats()
            print("sweep_share 1: last_scan_rows %d last_scan_bytes %d" % (st["last_scan_rows"], st["last_scan_bytes"]))
            assert st["last_scan_bytes"] == st["last_scan_rows"] * ix.bytes_per_row
    finally:
        ix.close()
