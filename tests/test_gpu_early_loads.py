"""GPU: the unfiltered per-query sparse sweep of a compile-time width issues its tile's loads in front of the query staging and the first
barrier (EARLY, bbq_scan_body.h): the masks' load, the tile's loads, the LDS write and the barrier in that order, the masks' load and the LDS
write in both arms of the scalar "has this wave a tile" branch.  The order changes no answer and has no option, so there is no second value
to compare with: every case is held to the oracle exactly - indices, f32 score BITS and counts equal heap_topk of the oracle's scores.
host_replays / dense_fallbacks are printed, not compared.

What can go wrong with the order, and the smallest shapes that show it:
  waves without a tile      the staging wave and the barrier must survive waves that load nothing: 1025, 1087, 1089, 1537 rows (behind the
                            dense first segment a chunk whose wave 0 holds one row and waves 1-7 nothing, ...), 19 044 rows (38 chunks, the
                            last partly filled), 37 queries (32 + 5: padding workgroups of the reordered grid leave idle, after staging, in
                            front of the barrier) and 1 query
  staging by several waves  96 units (1-bit 1536-d, queryBits 8) and 64 (2-bit 1024-d, queryBits 8): waves 0 and 1 stage
  both load arms, both      resident_mb 0 (streamed arm, plain grid, the kernel that counts the sum), 1 (part of the 38 chunks resident) and
  grid orders               -1, each under l2_share 1 and 32
  the end of the chunk      append mode (few queries) and the flood tier behind the new order

The filtered family keeps the old order (the early one was measured slower under sparse filters, docs/dropped.md), so the filtered cases
here - a staging wave whose accept word is 0, whole chunks rejected, one row in the last tile, every row accepted, and the small row counts
1, 63, 65, 513 through a filter that accepts everything - hold the family that shares the template to the oracle on the same shapes.

Which launches are sparse.  An unfiltered search sweeps its first 1024 rows (first_segment_rows) with a dense launch, which keeps its order;
a filtered plan has sparse segments only.  So the small row counts run twice, unfiltered as they are and through an all-accepting filter,
and the same partial tiles are put behind row 1024 (1025, 1087, 1089, 1537 rows) for the unfiltered family."""
import functools

import numpy as np
import pytest

from bbqlib import bbq_amd as B, capi
from test_gpu_l2_share import CDP, _expected, _scores, _synthetic, bits32
from test_gpu_row_sums import RAGGED_K, _multibit, _ragged, _ragged_want, _small_segments, MB_K

pytestmark = pytest.mark.gpu


def _check(ix, run, want, what=""):
    """run() -> (idx [nq][k], scores, counts): exactly `want`, the oracle's heap per query"""
    ix.reset_stats()
    idx, sc, cnt = run()
    st = ix.stats()
    print("%s host_replays %d dense_fallbacks %d" % (what, st["host_replays"], st["dense_fallbacks"]))
    for q, (wi, ws) in enumerate(want):
        assert cnt[q] == len(wi), "%s query %d: count" % (what, q)
        np.testing.assert_array_equal(idx[q, :cnt[q]], wi, err_msg="%s query %d" % (what, q))
        np.testing.assert_array_equal(bits32(sc[q, :cnt[q]]), bits32(ws), err_msg="%s query %d" % (what, q))
    return idx, bits32(sc), cnt


# ------------------------------------------------------------------------------------------------ 1. waves without a tile
@pytest.mark.parametrize("nq", [37, 1])
@pytest.mark.parametrize("n", [1, 63, 65, 513, 1025, 1087, 1089, 1537])
def test_row_counts(n, nq):
    """the first n rows of the 768-d ragged index (a row's score does not depend on the other rows): unfiltered, then every row through
    the filtered family's sparse sweep (which keeps the old order)"""
    codes, corr, qq, qc = _ragged(768)
    s32, _ = _ragged_want(768, 1)
    want = [_expected(s[:n], RAGGED_K) for s in s32[:nq]]
    ix = B.Index(codes[:n], corr[:n], 768, CDP, corrections="compact")
    try:
        _small_segments(ix)
        _check(ix, lambda: ix.search_batch(qq[:nq], qc[:nq], 4, 1, RAGGED_K), want, "unfiltered")
        with capi.Filter(ix, np.ones(n, bool)) as flt:
            _check(ix, lambda: ix.search_filtered_batch(qq[:nq], qc[:nq], 4, 1, RAGGED_K, flt), want, "all rows accepted")
    finally:
        ix.close()


# 19 044 rows = 38 chunks, the last one partly filled; 37 queries.  128-d, 768-d, 1024-d, 1536-d: the compile-time widths (1, 6, 8, 12 chunks
# of a row); 200-d: the run-time width, which keeps its order
@pytest.mark.parametrize("dim,sim", [(128, 1), (768, 0), (768, 1), (768, 2), (1024, 1), (1536, 1), (200, 1)])
def test_ragged_grid(dim, sim):
    codes, corr, qq, qc = _ragged(dim)
    _, want = _ragged_want(dim, sim)
    ix = B.Index(codes, corr, dim, CDP, corrections="compact")
    try:
        _small_segments(ix)
        _check(ix, lambda: ix.search_batch(qq, qc, 4, sim, RAGGED_K), want, "37 queries")
        _check(ix, lambda: ix.search_batch(qq[:1], qc[:1], 4, sim, RAGGED_K), want[:1], "1 query")
    finally:
        ix.close()


# ------------------------------------------------------------------------------------------------ 2. a staging wave that loads no tile
def _filter_mask(which, n):
    rows = np.arange(n)
    if which == "tile0_of_each_chunk_rejected":     # wave 0 stages, and its accept word is 0
        return (rows % 512) >= 64
    if which == "whole_chunks_rejected":            # two of every three chunks: all eight accept words of the workgroup are 0
        return (rows // 512) % 3 == 1
    if which == "one_row_in_the_last_tile":
        return rows == n - 3
    assert which == "everything"
    return np.ones(n, bool)


@pytest.mark.parametrize("which", ["tile0_of_each_chunk_rejected", "whole_chunks_rejected", "one_row_in_the_last_tile", "everything"])
@pytest.mark.parametrize("dim", [768, 1024])
def test_filtered_staging_wave(dim, which):
    codes, corr, qq, qc = _ragged(dim)
    s32, _ = _ragged_want(dim, 1)
    mask = _filter_mask(which, len(codes))
    ix = B.Index(codes, corr, dim, CDP, corrections="compact")
    try:
        _small_segments(ix)
        with capi.Filter(ix, mask) as flt:
            want = [_expected(s, RAGGED_K, mask) for s in s32]
            _check(ix, lambda: ix.search_filtered_batch(qq, qc, 4, 1, RAGGED_K, flt), want, which)
    finally:
        ix.close()


# ------------------------------------------------------------------------------------------------ 3. staging wider than one wave
WIDE_N, WIDE_NQ = 5_003, 12


@functools.lru_cache(maxsize=None)
def _wide_1bit():
    """1-bit 1536-d rows against 8-plane queries: 12 chunks x 8 planes = 96 units of 16 bytes, threads 0-95 stage"""
    codes, corr, qq, qc = _synthetic(1536 + 8, WIDE_N, 1536, 1, 8, WIDE_NQ)
    s32 = _scores(codes, corr, 1536, qq, qc, 8, 1, 1)
    for a in (codes, corr, qq, qc, *s32):
        a.setflags(write=False)
    return codes, corr, qq, qc, s32


@pytest.mark.parametrize("family", ["1bit_1536_qb8", "2bit_1024_qb8", "2bit_1024_qb4"])
def test_staging_wider_than_one_wave(family):
    """2-bit 1024-d rows are 16 chunks: 64 units at queryBits 8 (the reference throws there: the oracle's extension, as bench.py's
    oracle_scores), 32 at queryBits 4.  Unfiltered, then a filter whose every fifth tile is empty"""
    if family == "1bit_1536_qb8":
        dim, ib, qb = 1536, 1, 8
        codes, corr, qq, qc, s32 = _wide_1bit()
    else:
        dim, ib, qb = 1024, 2, 8 if family.endswith("qb8") else 4
        codes, corr, qq, qc, s32 = _multibit(dim, ib, qb)
    n = len(codes)
    mask = np.random.default_rng(len(family)).random(n) < 0.3
    mask[(np.arange(n) // 64) % 5 == 0] = False     # tile 0 of chunks 0, 5, 10, ... among them: a staging wave without a tile
    ix = B.Index(codes, corr, dim, CDP, index_bits=ib, corrections="compact")
    try:
        _small_segments(ix)
        _check(ix, lambda: ix.search_batch(qq, qc, qb, 1, MB_K), [_expected(s, MB_K) for s in s32], "unfiltered")
        with capi.Filter(ix, mask) as flt:
            _check(ix, lambda: ix.search_filtered_batch(qq, qc, qb, 1, MB_K, flt), [_expected(s, MB_K, mask) for s in s32], "filtered")
    finally:
        ix.close()


# ------------------------------------------------------------------------------------------------ 4. both load arms and both grid orders
def test_load_arms_and_grid_orders():
    """resident_share's rule is (chunk & 63) < share, so the 38 chunks cover both arms of the tile's loads once part of them is resident"""
    codes, corr, qq, qc = _ragged(768)
    _, want = _ragged_want(768, 1)
    ix = B.Index(codes, corr, 768, CDP, corrections="compact")
    try:
        _small_segments(ix)
        first = None
        for mb in (0, 1, -1):
            ix.set_option("resident_mb", mb)
            for share in (1, 32):
                ix.set_option("l2_share", share)
                got = _check(ix, lambda: ix.search_batch(qq, qc, 4, 1, RAGGED_K), want, "resident_mb %d l2_share %d" % (mb, share))
                assert (ix.stats()["resident_bytes"] == 0) == (mb == 0)
                if first is None:
                    first = got
                for a, b in zip(got, first):
                    np.testing.assert_array_equal(a, b, err_msg="resident_mb %d l2_share %d" % (mb, share))
    finally:
        ix.close()


# ------------------------------------------------------------------------------------------------ 5. append mode and the flood tier
@pytest.mark.parametrize("nq", [1, 3])
def test_append_mode(nq):
    """few queries: the sweeps of several sparse segments append their candidates to the lists themselves.  A single query: the general
    path (latency_fused 0 - the fused chain has kernels of its own)"""
    codes, corr, qq, qc = _ragged(768)
    _, want = _ragged_want(768, 1)
    ix = B.Index(codes, corr, 768, CDP, corrections="compact")
    try:
        _small_segments(ix)
        ix.set_option("latency_fused", 0)
        _check(ix, lambda: ix.search_batch(qq[:nq], qc[:nq], 4, 1, RAGGED_K), want[:nq], "%d queries" % nq)
    finally:
        ix.close()


def test_flood_tier():
    """a chunk with more passing rows than its slot: 600 copies of one row that scores above everything else for the query made from
    it fill chunk 9 and spill into chunk 10, behind segments whose thresholds come from ordinary rows.  The copies tie, so the
    oracle's heap decides which of them answer - by the history the library has to replay"""
    dim, k = 768, RAGGED_K
    codes, corr, qq, qc = _ragged(dim)
    codes, corr = codes[:8192].copy(), corr[:8192].copy()
    good = 9 * 512 + 17
    codes[9 * 512:9 * 512 + 600] = codes[good]
    corr[9 * 512:9 * 512 + 600] = corr[good]
    bits = np.unpackbits(codes[good])[:dim]
    q_flood = (bits * 15).astype(np.uint8)          # the 4-bit query that weighs exactly the good row's bits
    qq2 = np.concatenate([q_flood[None, :], qq[:8]])
    qc2 = np.concatenate([qc[:1], qc[:8]]).copy()
    qc2[0, 3] = q_flood.sum()
    s32 = _scores(codes, corr, dim, qq2, qc2, 4, 1, 1)
    assert (np.sort(s32[0])[-600:] == s32[0][good]).all(), "the copies are the query's 600 best rows"
    ix = B.Index(codes, corr, dim, CDP, corrections="compact")
    try:
        _small_segments(ix)
        ix.set_option("replay_threads", 4)
        _check(ix, lambda: ix.search_batch(qq2, qc2, 4, 1, k), [_expected(s, k) for s in s32], "clustered")
        assert ix.stats()["candidates"] >= 600, "the flooded chunk's rows were all listed"
    finally:
        ix.close()
