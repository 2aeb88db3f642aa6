"""GPU: option l2_share - the per-query sweep's workgroup -> (chunk, query) map (sweep_coord, bbq_device.h) - changes no answer.

The criterion everywhere: for every l2_share in {1, 2, 4, 8, 16, 32, -1} the indices, the f32 score BITS and the counts are identical
to those of l2_share = 1, the l2_share = 1 results are heap_topk of the oracle's scores, and host_replays / dense_fallbacks do not
change between the values.  No tolerances."""
import functools

import numpy as np
import pytest

import orclib as O
from bbqlib import bbq_amd as B, capi

pytestmark = pytest.mark.gpu

SHARES = (1, 2, 4, 8, 16, 32, -1)
CDP = 0.0009


def bits32(a):
    a = np.array(a, np.float32)
    a[np.isnan(a)] = np.nan
    return a.view(np.uint32)


def _synthetic(seed, n, dim, ib, qb, nq):
    """random codes and plausible corrections, as test_cache_resident_chunks_change_no_answer builds them"""
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
    qq = rng.integers(0, 1 << qb, size=(nq, dim), dtype=np.uint8)
    qc = np.empty((nq, 4))
    qc[:, 0] = -0.15 * (0.9 + 0.2 * rng.random(nq))
    qc[:, 1] = 0.148 * (0.9 + 0.2 * rng.random(nq))
    qc[:, 2] = -0.0028 * rng.random(nq)
    qc[:, 3] = qq.sum(axis=1)
    return codes, corr, qq, qc


def _scores(codes, corr, dim, qq, qc, qb, sim, ib):
    out = []
    for q in range(len(qq)):
        if ib == 1:
            _, _, s32 = O.score_all(codes, corr, dim, qq[q], qc[q], qb, sim, CDP)
        elif qb in (1, 4):
            _, _, s32 = O.score_all(codes, corr, dim, qq[q], qc[q], qb, sim, CDP, ib=ib)
        else:   # the reference throws for this queryBits on a multi-bit index: libbbq's documented extension
            _, _, s32 = O.score_all_multibit_ext(codes, corr, dim, qq[q], qc[q], qb, sim, CDP)
        out.append(s32)
    return out


# the ragged grid: 19 044 rows = 38 chunks (four groups of 8 plus 6, the last chunk partly filled), 37 queries = one launch group of 32
# plus 5.  Computed once, shared by the tests below and never changed.
RAGGED = dict(n=19_044, dim=768, ib=1, qb=4, sim=1, nq=37, k=50)


@functools.lru_cache(maxsize=None)
def _ragged():
    c = RAGGED
    codes, corr, qq, qc = _synthetic(5, c["n"], c["dim"], c["ib"], c["qb"], c["nq"])
    s32 = _scores(codes, corr, c["dim"], qq, qc, c["qb"], c["sim"], c["ib"])
    for a in (codes, corr, qq, qc, *s32):
        a.setflags(write=False)
    return codes, corr, qq, qc, s32


def _ragged_index():
    codes, corr, qq, qc, s32 = _ragged()
    ix = B.Index(codes, corr, RAGGED["dim"], CDP, corrections="compact")
    # launches of 2, 4, 8, ... chunks, some with fewer than 8, each with its own chunk_begin
    ix.set_option("first_segment_rows", 1024)
    ix.set_option("segment_growth", 2)
    return ix


def _expected(s32, k, mask=None):
    """the oracle's heap over the (accepted) rows' scores in ascending row order"""
    if mask is None:
        return O.heap_topk(s32, k)
    acc = np.flatnonzero(mask)
    pos, sc = O.heap_topk(s32[acc], k)
    return acc[pos].astype(np.int32), sc


def _check_all_shares(ix, run, want, shares=SHARES):
    """run() -> (idx [nq][k], scores, counts) under every l2_share: the first (l2_share 1) equals `want`, the others equal the first"""
    assert shares[0] == 1
    first = first_stats = None
    for share in shares:
        ix.set_option("l2_share", share)
        ix.reset_stats()
        idx, sc, cnt = run()
        st = ix.stats()
        st = (st["host_replays"], st["dense_fallbacks"])
        if first is None:
            first, first_stats = (idx, bits32(sc), cnt), st
            for q, (wi, ws) in enumerate(want):
                assert cnt[q] == len(wi), "query %d" % q
                np.testing.assert_array_equal(idx[q, :cnt[q]], wi, err_msg="l2_share 1, query %d" % q)
                np.testing.assert_array_equal(bits32(sc[q, :cnt[q]]), bits32(ws), err_msg="l2_share 1, query %d" % q)
        else:
            np.testing.assert_array_equal(cnt, first[2], err_msg="l2_share %d" % share)
            np.testing.assert_array_equal(idx, first[0], err_msg="l2_share %d" % share)
            np.testing.assert_array_equal(bits32(sc), first[1], err_msg="l2_share %d" % share)
            assert st == first_stats, "l2_share %d: host_replays / dense_fallbacks %r, with l2_share 1 %r" % (share, st, first_stats)
    ix.set_option("l2_share", -1)
    return first_stats


def test_ragged_grid():
    codes, corr, qq, qc, s32 = _ragged()
    c = RAGGED
    ix = _ragged_index()
    try:
        want = [_expected(s, c["k"]) for s in s32]
        _check_all_shares(ix, lambda: ix.search_batch(qq, qc, c["qb"], c["sim"], c["k"]), want)
    finally:
        ix.close()


@pytest.mark.parametrize("dim,ib,qb,sim,compact", [(100, 1, 1, 0, False), (1024, 2, 8, 1, True)])
def test_other_kernels_of_the_template(dim, ib, qb, sim, compact):
    """a run-time row width with the inline layout, and config 5's multi-bit kernel"""
    n, nq, k = 5_003, 12, 50
    codes, corr, qq, qc = _synthetic(dim + qb, n, dim, ib, qb, nq)
    s32 = _scores(codes, corr, dim, qq, qc, qb, sim, ib)
    ix = B.Index(codes, corr, dim, CDP, index_bits=ib, corrections="compact" if compact else "inline")
    try:
        ix.set_option("first_segment_rows", 1024)
        ix.set_option("segment_growth", 2)
        _check_all_shares(ix, lambda: ix.search_batch(qq, qc, qb, sim, k), [_expected(s, k) for s in s32])
    finally:
        ix.close()


@pytest.mark.parametrize("which", ["random_30", "last_three_chunks"])
def test_filtered_search(which):
    codes, corr, qq, qc, s32 = _ragged()
    c = RAGGED
    n = c["n"]
    if which == "random_30":
        mask = np.random.default_rng(31).random(n) < 0.3
    else:   # every accepted row lies in the last three of the 38 chunks (the last one partly filled)
        mask = (np.arange(n) >= 35 * 512) & (np.random.default_rng(32).random(n) < 0.5)
    ix = _ragged_index()
    try:
        with capi.Filter(ix, mask) as flt:
            want = [_expected(s, c["k"], mask) for s in s32]
            _check_all_shares(ix, lambda: ix.search_filtered_batch(qq, qc, c["qb"], c["sim"], c["k"], flt), want)
    finally:
        ix.close()


def test_flood_tier():
    """rows stored cluster by cluster: the chunks of a query's own cluster hold far more rows above its threshold (derived from other
    clusters) than a chunk slot takes (cap_for: 48 entries behind 4096 rows at k 50, a chunk has 512 rows), so the count word redirects
    to the query's overflow block - under the new chunk numbering"""
    rng = np.random.default_rng(77)
    n, dim, ncl, k, sim = 40_000, 64, 20, 50, 1
    centres = rng.standard_normal((ncl, dim)).astype(np.float32)
    cid = np.sort(rng.integers(0, ncl, n))
    base = centres[cid] + 0.4 * rng.standard_normal((n, dim)).astype(np.float32)
    qcl = np.array([0, 1, 5, 13, 19, 19, 17, 9, 10])
    queries = centres[qcl] + 0.4 * rng.standard_normal((len(qcl), dim)).astype(np.float32)
    codes, corr, cen = B.quantize_vectors(base, sim)
    cdp = B.centroid_dp(cen)
    qs = [B.quantize_query(q, cen, sim, 4) for q in queries]
    qq, qc = np.stack([a for a, _ in qs]), np.stack([b for _, b in qs])
    want = [O.heap_topk(O.score_all(codes, corr, dim, qq[i], qc[i], 4, sim, cdp)[2], k) for i in range(len(qcl))]
    ix = B.Index(codes, corr, dim, cdp, corrections="compact")
    try:
        ix.set_option("replay_threads", 4)
        stats = _check_all_shares(ix, lambda: ix.search_batch(qq, qc, 4, sim, k), want)
        assert stats[1] == 0                                       # no dense fallback: the floods were parked
        ix.set_option("l2_share", 8)
        ix.reset_stats()
        ix.search_batch(qq, qc, 4, sim, k)
        assert ix.stats()["candidates"] > len(qcl) * 1000          # ... and replayed: whole chunks of candidates per query
    finally:
        ix.close()


@pytest.mark.parametrize("nq", [1, 3])
def test_few_queries(nq):
    """calls with few queries append their candidates to the lists themselves, and have fewer queries than P"""
    codes, corr, qq, qc, s32 = _ragged()
    c = RAGGED
    ix = _ragged_index()
    try:
        want = [_expected(s, c["k"]) for s in s32[:nq]]
        for fused in (1, 0):   # a single query: the three-launch latency path, then the general one (append mode through the sweep)
            ix.set_option("latency_fused", fused)
            _check_all_shares(ix, lambda: ix.search_batch(qq[:nq], qc[:nq], c["qb"], c["sim"], c["k"]), want)
    finally:
        ix.close()


def test_residency_combinations():
    codes, corr, qq, qc, s32 = _ragged()
    c = RAGGED
    ix = _ragged_index()
    try:
        want = [_expected(s, c["k"]) for s in s32]
        for mb in (0, 1, -1):
            ix.set_option("resident_mb", mb)
            _check_all_shares(ix, lambda: ix.search_batch(qq, qc, c["qb"], c["sim"], c["k"]), want, shares=(1, 8))
            assert (ix.stats()["resident_bytes"] == 0) == (mb == 0)
    finally:
        ix.close()


def test_option_validation():
    codes, corr, qq, qc, s32 = _ragged()
    ix = B.Index(codes[:1024], corr[:1024], RAGGED["dim"], CDP)
    try:
        for bad in (0, 3, 64, -2, 33):
            with pytest.raises(capi.BBQError) as e:
                ix.set_option("l2_share", bad)
            assert e.value.code == capi.ERR_INVALID_ARG
        for good in SHARES:
            ix.set_option("l2_share", good)
    finally:
        ix.close()
