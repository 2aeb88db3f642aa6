"""GPU: option tiles_per_wave - a wave of the unfiltered per-query sparse sweep in its digit form (768-d, 1024-d, 1536-d rows, queryBits 4)
takes 1, 2, 4 or 8 consecutive tiles of its chunk one after the other (TPW, sweep_wave_tiles in bbq_scan_body.h); the workgroup has 8, 4, 2
or 1 waves.  The option changes no answer.

The criterion everywhere: under every value in (1, 2, 4, 8) the answer is heap_topk of the oracle's scores - indices, f32 score BITS and
counts - and the three arrays are identical across the four values.  No tolerances.  host_replays / dense_fallbacks are printed.

What can go wrong with several tiles per wave, and the smallest shapes that show it:
  a wave whose loop ends early  behind the dense first segment of 1024 rows: 1025, 1089 (tile 0 full, tile 1 one row), 1153, 1217 (three
                                tiles and a row), 1281 (four tiles and a row: at 4 tiles per wave wave 0 is full and wave 1 holds one row),
                                1535, 1537 rows; 37 queries (padding workgroups of the reordered grid leave idle) and 1
  the ragged grid               19 044 rows = 38 chunks, the last partly filled, every similarity; 1024-d and 1536-d (the other widths with
                                twins) and 200-d (no twin: the option falls back to one tile per wave)
  both load arms, both orders   resident_mb 0 (with row_sums 1 and digit_planes 1 set, or the strict mode would pick the kernel without a
                                twin), 1 and -1, each under l2_share 1 and 32
  the end of the chunk          with 256, 128 and 64 threads: the flood tier (600 passing rows in several tiles of one wave and of several
                                waves, parked in the overflow area) and the append mode
  a NaN score in a late tile    the flag of the wave's running NaN vote"""
import numpy as np
import pytest

from bbqlib import bbq_amd as B, capi
from test_gpu_early_loads import _ragged, _ragged_want, _small_segments, _expected, _scores, CDP, RAGGED_K, bits32

pytestmark = pytest.mark.gpu

TPW = (1, 2, 4, 8)


def _check_tpw(ix, run, want, what="", fallbacks=None):
    """run() -> (idx [nq][k], scores, counts) under each tiles_per_wave: each equals `want`, and all equal the first"""
    first = None
    try:
        for v in TPW:
            ix.set_option("tiles_per_wave", v)
            ix.reset_stats()
            idx, sc, cnt = run()
            st = ix.stats()
            print("%s tiles_per_wave %d: host_replays %d dense_fallbacks %d" % (what, v, st["host_replays"], st["dense_fallbacks"]))
            for q, (wi, ws) in enumerate(want):
                assert cnt[q] == len(wi), "%s tiles_per_wave %d, query %d: count" % (what, v, q)
                np.testing.assert_array_equal(idx[q, :cnt[q]], wi, err_msg="%s tiles_per_wave %d, query %d" % (what, v, q))
                np.testing.assert_array_equal(bits32(sc[q, :cnt[q]]), bits32(ws), err_msg="%s tiles_per_wave %d, query %d" % (what, v, q))
            if fallbacks is not None:
                assert st["dense_fallbacks"] == fallbacks, "%s tiles_per_wave %d: dense_fallbacks" % (what, v)
            got = (idx, bits32(sc), cnt)
            if first is None:
                first = got
            for a, b in zip(got, first):
                np.testing.assert_array_equal(a, b, err_msg="%s tiles_per_wave %d against 1" % (what, v))
    finally:
        ix.set_option("tiles_per_wave", -1)
    return first


# ------------------------------------------------------------------------------------------------ 1. a wave whose loop ends early
@pytest.mark.parametrize("nq", [37, 1])
@pytest.mark.parametrize("n", [1025, 1089, 1153, 1217, 1281, 1535, 1537])
def test_loop_ends_early(n, nq):
    codes, corr, qq, qc = _ragged(768)
    s32, _ = _ragged_want(768, 1)
    want = [_expected(s[:n], RAGGED_K) for s in s32[:nq]]
    ix = B.Index(codes[:n], corr[:n], 768, CDP, corrections="compact")
    try:
        _small_segments(ix)
        _check_tpw(ix, lambda: ix.search_batch(qq[:nq], qc[:nq], 4, 1, RAGGED_K), want, "%d rows" % n)
    finally:
        ix.close()


# ------------------------------------------------------------------------------------------------ 2. the ragged grid
# 768-d, 1024-d, 1536-d: the widths with twins; 200-d: the run-time width, no twin - every value runs one tile per wave
@pytest.mark.parametrize("dim,sim", [(768, 0), (768, 1), (768, 2), (1024, 1), (1536, 1), (200, 1)])
def test_ragged_grid(dim, sim):
    codes, corr, qq, qc = _ragged(dim)
    _, want = _ragged_want(dim, sim)
    ix = B.Index(codes, corr, dim, CDP, corrections="compact")
    try:
        _small_segments(ix)
        _check_tpw(ix, lambda: ix.search_batch(qq, qc, 4, sim, RAGGED_K), want, "37 queries")
        _check_tpw(ix, lambda: ix.search_batch(qq[:1], qc[:1], 4, sim, RAGGED_K), want[:1], "1 query")
    finally:
        ix.close()


# ------------------------------------------------------------------------------------------------ 3. both load arms and both grid orders
def test_load_arms_and_grid_orders():
    """resident_share's rule is (chunk & 63) < share, so the 38 chunks cover both arms of the tiles' loads once part of them is resident;
    with resident_mb 0 every chunk is streamed - through the twins only because row_sums and digit_planes are set explicitly"""
    codes, corr, qq, qc = _ragged(768)
    _, want = _ragged_want(768, 1)
    ix = B.Index(codes, corr, 768, CDP, corrections="compact")
    try:
        _small_segments(ix)
        first = None
        for mb in (0, 1, -1):
            ix.set_option("resident_mb", mb)
            ix.set_option("row_sums", 1 if mb == 0 else -1)
            ix.set_option("digit_planes", 1 if mb == 0 else -1)
            for share in (1, 32):
                ix.set_option("l2_share", share)
                got = _check_tpw(ix, lambda: ix.search_batch(qq, qc, 4, 1, RAGGED_K), want, "resident_mb %d l2_share %d" % (mb, share))
                assert (ix.stats()["resident_bytes"] == 0) == (mb == 0)
                if first is None:
                    first = got
                for a, b in zip(got, first):
                    np.testing.assert_array_equal(a, b, err_msg="resident_mb %d l2_share %d" % (mb, share))
    finally:
        ix.close()


# ------------------------------------------------------------------------------------------------ 4. the end of the chunk with fewer threads
def test_flood_tier():
    """test_gpu_early_loads.test_flood_tier's construction: 600 copies of one row that scores above everything else for the query made from
    it fill chunk 9 - all eight tiles, so several tiles of every wave - and spill into chunk 10; more than the slot's capacity, so the
    workgroup of 256, 128 or 64 threads parks them in the overflow area"""
    dim, k = 768, RAGGED_K
    codes, corr, qq, qc = _ragged(dim)
    codes, corr = codes[:8192].copy(), corr[:8192].copy()
    good = 9 * 512 + 17
    codes[9 * 512:9 * 512 + 600] = codes[good]
    corr[9 * 512:9 * 512 + 600] = corr[good]
    bits = np.unpackbits(codes[good])[:dim]
    q_flood = (bits * 15).astype(np.uint8)
    qq2 = np.concatenate([q_flood[None, :], qq[:8]])
    qc2 = np.concatenate([qc[:1], qc[:8]]).copy()
    qc2[0, 3] = q_flood.sum()
    s32 = _scores(codes, corr, dim, qq2, qc2, 4, 1, 1)
    assert (np.sort(s32[0])[-600:] == s32[0][good]).all(), "the copies are the query's 600 best rows"
    ix = B.Index(codes, corr, dim, CDP, corrections="compact")
    try:
        _small_segments(ix)
        ix.set_option("replay_threads", 4)
        _check_tpw(ix, lambda: ix.search_batch(qq2, qc2, 4, 1, k), [_expected(s, k) for s in s32], "clustered")
        assert ix.stats()["candidates"] >= 600, "the flooded chunk's rows were all listed"
    finally:
        ix.close()


@pytest.mark.parametrize("nq", [1, 3])
def test_append_mode(nq):
    """few queries: the sweeps append their candidates to the lists themselves (a single query on the general path: latency_fused 0)"""
    codes, corr, qq, qc = _ragged(768)
    _, want = _ragged_want(768, 1)
    ix = B.Index(codes, corr, 768, CDP, corrections="compact")
    try:
        _small_segments(ix)
        ix.set_option("latency_fused", 0)
        _check_tpw(ix, lambda: ix.search_batch(qq[:nq], qc[:nq], 4, 1, RAGGED_K), want[:nq], "%d queries" % nq)
    finally:
        ix.close()


# ------------------------------------------------------------------------------------------------ 5. a NaN row in a late tile of a wave
def test_nan_row_in_a_late_tile():
    """a row whose lower interval is NaN scores NaN for every query: the compact bound cannot exclude it, the exact score raises the
    wave's NaN vote, the query is flagged and answered densely - the oracle's heap.  The rows sit behind the dense first segment in tile 3
    of a chunk (the last tile of a wave at 4 per wave, the second at 2, the fourth at 8) and in tile 7 (the last at every value)"""
    dim, nq = 768, 3
    codes, corr, qq, qc = _ragged(dim)
    codes, corr = codes[:4096].copy(), corr[:4096].copy()
    for r in (1024 + 2 * 512 + 3 * 64 + 5, 1024 + 4 * 512 + 7 * 64 + 62):
        corr[r, 0] = np.nan
    s32 = _scores(codes, corr, dim, qq[:nq], qc[:nq], 4, 1, 1)
    assert all(np.isnan(s).sum() == 2 for s in s32)
    ix = B.Index(codes, corr, dim, CDP, corrections="compact")
    try:
        _small_segments(ix)
        _check_tpw(ix, lambda: ix.search_batch(qq[:nq], qc[:nq], 4, 1, RAGGED_K), [_expected(s, RAGGED_K) for s in s32], "NaN rows", fallbacks=nq)
    finally:
        ix.close()


# ------------------------------------------------------------------------------------------------ 6. option handling
def test_option_validation():
    codes, corr, qq, qc = _ragged(128)
    ix = B.Index(codes[:1024], corr[:1024], 128, CDP)
    try:
        for bad in (0, 3, 16, -2):
            with pytest.raises(capi.BBQError) as e:
                ix.set_option("tiles_per_wave", bad)
            assert e.value.code == capi.ERR_INVALID_ARG
        for good in (-1, 1, 2, 4, 8):
            ix.set_option("tiles_per_wave", good)
    finally:
        ix.close()
