"""GPU: the sweeps with several tiles per wave (option tiles_per_wave 2, 4, 8; sweep_wave_tiles in bbq_scan_body.h) keep the exact path out of
their tile loop: a row that passes the f32 bound leaves a 4-byte entry (row in the chunk, qcDist) in a deferred list in LDS, and one loop
behind the tiles (sweep_deferred_exact) takes the entries 64 at a time - the f64 bound of a query without f32 images, the exact corrections,
the f64 score, the NaN vote, the key test, the candidate.  With the flood tier or in the append mode the list lies in the upper half of the
candidates' own 4 KB and the candidates grow into it from below.  None of it changes an answer.

The criterion everywhere is test_gpu_tiles_per_wave's: under every value in (1, 2, 4, 8) the answer is heap_topk of the oracle's scores -
indices, f32 score BITS and counts - and the three arrays are identical across the four values.  No tolerances.

What can go wrong, and the smallest shapes that show it (768-d unless said otherwise; a "planted" row is a copy of one row that scores above
every other row for the query made from its bits, so it passes the bound whatever the threshold):
  a full list                 all 512 rows of chunk 9 planted: every slot of the in-place layout is read and overwritten - with the flood tier,
                              without it (the chunk overflows its slot: flagged, answered densely) and in the append mode
  more than one batch         65 and 129 planted rows spread over the eight tiles of a chunk: at 8 tiles per wave the loop runs twice and three
                              times, at 2 and 4 the waves' lists have different lengths; one row at lane 63 of the chunk's last tile, one at
                              lane 0 of its first
  a ragged end                1024 + 512 + 65 rows, the last one planted: its tile holds one row, its wave fewer tiles than it could take
  the f64 bound               fast_bound 0 defers EVERY valid row and tests the f64 bound behind the loop: the planted chunk and the ordinary
                              ragged grid, every similarity
  a NaN and a +inf            in a chunk's last tile: the NaN vote now comes from the deferred loop
  other widths and settings   the full list and the ragged end at 1024-d and 1536-d, and under l2_share 1 / 32 and both load arms"""
import functools

import numpy as np
import pytest

from bbqlib import bbq_amd as B
from test_gpu_early_loads import _ragged, _ragged_want, _small_segments, _expected, _scores, CDP, RAGGED_K, bits32

pytestmark = pytest.mark.gpu

TPW = (1, 2, 4, 8)
CHUNK = 512
PLAIN_Q = 4                    # ordinary queries that travel with the planted one
FULL_N, FULL_AT = 8192, 9 * CHUNK   # the planted chunk: behind the dense first segment and sparse segments of ordinary rows
RAGGED_END_N = 1024 + CHUNK + 65


def _check_tpw(ix, run, want, what="", min_fallbacks=0):
    """run() -> (idx [nq][k], scores, counts) under each tiles_per_wave: each equals `want`, and all equal the first"""
    first = None
    try:
        for v in TPW:
            ix.set_option("tiles_per_wave", v)
            ix.reset_stats()
            idx, sc, cnt = run()
            st = ix.stats()
            print("%s tiles_per_wave %d: host_replays %d dense_fallbacks %d candidates %d" % (what, v, st["host_replays"], st["dense_fallbacks"], st["candidates"]))
            for q, (wi, ws) in enumerate(want):
                assert cnt[q] == len(wi), "%s tiles_per_wave %d, query %d: count" % (what, v, q)
                np.testing.assert_array_equal(idx[q, :cnt[q]], wi, err_msg="%s tiles_per_wave %d, query %d" % (what, v, q))
                np.testing.assert_array_equal(bits32(sc[q, :cnt[q]]), bits32(ws), err_msg="%s tiles_per_wave %d, query %d" % (what, v, q))
            assert st["dense_fallbacks"] >= min_fallbacks, "%s tiles_per_wave %d: dense_fallbacks" % (what, v)
            got = (idx, bits32(sc), cnt)
            if first is None:
                first = got
            for a, b in zip(got, first):
                np.testing.assert_array_equal(a, b, err_msg="%s tiles_per_wave %d against 1" % (what, v))
    finally:
        ix.set_option("tiles_per_wave", -1)
    return first


@functools.lru_cache(maxsize=None)
def _planted(dim, n, rows, sim=1):
    """the first n rows of the ragged index with copies of row rows[0] at `rows`, the query made from that row's bits in front of PLAIN_Q
    ordinary ones, and the oracle's scores.  Computed once per shape, shared and never changed"""
    codes, corr, qq, qc = _ragged(dim)
    codes, corr = codes[:n].copy(), corr[:n].copy()
    at = np.array(rows)
    if sim == 0:
        # EUCLIDEAN clamps the score of a row that lies "too close" to +0, which is where the query made from a row's bits puts that row with
        # these corrections: there the planted row is the best row ordinary query 0 has among the ordinary rows, moved to rows[0]
        src = int(np.argmax(_scores(codes, corr, dim, qq[:1], qc[:1], 4, sim, 1)[0]))
        codes[[src, at[0]]] = codes[[at[0], src]]
        corr[[src, at[0]]] = corr[[at[0], src]]
    good = at[0]
    codes[at] = codes[good]
    corr[at] = corr[good]
    if sim == 0:
        q_top, c_top = qq[0], qc[0]
    else:
        q_top = (np.unpackbits(codes[good])[:dim] * 15).astype(np.uint8)   # the 4-bit query that weighs exactly the planted row's bits
        c_top = qc[0].copy()
        c_top[3] = q_top.sum()
    qq2 = np.concatenate([q_top[None, :], qq[:PLAIN_Q]])
    qc2 = np.concatenate([c_top[None, :], qc[:PLAIN_Q]])
    s32 = _scores(codes, corr, dim, qq2, qc2, 4, sim, 1)
    best = np.sort(s32[0])[-len(at):]
    assert (best == s32[0][good]).all() and (s32[0] == s32[0][good]).sum() == len(at), "the planted rows are the query's best rows, and no other row ties"
    for a in (codes, corr, qq2, qc2, *s32):
        a.setflags(write=False)
    return codes, corr, qq2, qc2, s32


def _full(dim=768, sim=1):
    return _planted(dim, FULL_N, tuple(range(FULL_AT, FULL_AT + CHUNK)), sim)


def _ragged_end(dim=768):
    return _planted(dim, RAGGED_END_N, (RAGGED_END_N - 1,))


def _index(codes, corr, dim):
    ix = B.Index(codes, corr, dim, CDP, corrections="compact")
    _small_segments(ix)
    ix.set_option("replay_threads", 4)
    return ix


# ------------------------------------------------------------------------------------------------ 1. a full list
@pytest.mark.parametrize("mode", ["flood_tier", "no_flood_tier", "append"])
def test_full_list(mode):
    codes, corr, qq, qc, s32 = _full()
    nq = 3 if mode == "append" else len(qq)     # few queries: the sweeps append their candidates to the lists themselves
    ix = _index(codes, corr, 768)
    try:
        if mode == "no_flood_tier":
            ix.set_option("flood_rows", 0)      # 512 candidates overflow the chunk's slot: the query is flagged and answered densely
        if mode == "append":
            ix.set_option("latency_fused", 0)
        _check_tpw(ix, lambda: ix.search_batch(qq[:nq], qc[:nq], 4, 1, RAGGED_K), [_expected(s, RAGGED_K) for s in s32[:nq]], mode,
                   min_fallbacks=1 if mode == "no_flood_tier" else 0)
        if mode != "no_flood_tier":
            assert ix.stats()["candidates"] >= CHUNK, "the planted chunk's rows were all listed"
    finally:
        ix.close()


# ------------------------------------------------------------------------------------------------ 2. more than one batch of 64 entries
def _spread(per_tile):
    """per_tile rows in each of the chunk's eight tiles, and one more in the last"""
    rows = [t * 64 + (j * 64) // per_tile + 1 for t in range(8) for j in range(per_tile)]
    return sorted(set(rows + [7 * 64 + 63]))


PATTERNS = {
    "65_rows": _spread(8),                # 8 tiles per wave: two batches; 4: lists of 32 and 33; 2: of 16 and 17
    "129_rows": _spread(16),              # 8 tiles per wave: three batches; 4: 64 and 65 - one wave loops twice, the other waits at its barrier
    "lane_63_of_the_last_tile": [CHUNK - 1],
    "lane_0_of_the_first_tile": [0],
}
assert len(PATTERNS["65_rows"]) == 65 and len(PATTERNS["129_rows"]) == 129


@pytest.mark.parametrize("pattern", sorted(PATTERNS))
def test_batches(pattern):
    codes, corr, qq, qc, s32 = _planted(768, FULL_N, tuple(FULL_AT + r for r in PATTERNS[pattern]))
    ix = _index(codes, corr, 768)
    try:
        _check_tpw(ix, lambda: ix.search_batch(qq, qc, 4, 1, RAGGED_K), [_expected(s, RAGGED_K) for s in s32], pattern)
    finally:
        ix.close()


# ------------------------------------------------------------------------------------------------ 3. a ragged end
@pytest.mark.parametrize("dim", [768, 1024, 1536])
def test_ragged_end(dim):
    """chunk 3 holds 65 rows: tile 0 full, tile 1 the planted row alone, every later tile beyond the index"""
    codes, corr, qq, qc, s32 = _ragged_end(dim)
    want = [_expected(s, RAGGED_K) for s in s32]
    assert want[0][0][0] == RAGGED_END_N - 1, "the last row is the planted query's best"
    ix = _index(codes, corr, dim)
    try:
        _check_tpw(ix, lambda: ix.search_batch(qq, qc, 4, 1, RAGGED_K), want, "%d-d" % dim)
    finally:
        ix.close()


# ------------------------------------------------------------------------------------------------ 4. the f64 bound behind the loop
@pytest.mark.parametrize("sim", [0, 1, 2])
def test_f64_bound_full_list(sim):
    codes, corr, qq, qc, s32 = _full(768, sim)
    ix = _index(codes, corr, 768)
    try:
        ix.set_option("fast_bound", 0)
        _check_tpw(ix, lambda: ix.search_batch(qq, qc, 4, sim, RAGGED_K), [_expected(s, RAGGED_K) for s in s32], "fast_bound 0, sim %d" % sim)
    finally:
        ix.close()


@pytest.mark.parametrize("sim", [0, 1, 2])
def test_f64_bound_ordinary_rows(sim):
    codes, corr, qq, qc = _ragged(768)
    _, want = _ragged_want(768, sim)
    ix = _index(codes, corr, 768)
    try:
        ix.set_option("fast_bound", 0)
        _check_tpw(ix, lambda: ix.search_batch(qq, qc, 4, sim, RAGGED_K), want, "fast_bound 0, sim %d" % sim)
    finally:
        ix.close()


# ------------------------------------------------------------------------------------------------ 5. a NaN score and a +inf correction in a late tile
def test_nan_and_inf_in_a_late_tile():
    """a row whose lower interval is NaN scores NaN for every query: no bound excludes it, it is deferred, its exact score raises the NaN
    vote behind the loop, the query is flagged and answered densely.  A row whose additional correction is +inf scores +inf: deferred as
    well, and every query's best row.  Both in tile 7 of their chunks, the last tile of a wave at every value"""
    dim, nq = 768, 3
    codes, corr, qq, qc = _ragged(dim)
    codes, corr = codes[:4096].copy(), corr[:4096].copy()
    corr[1024 + 4 * CHUNK + 7 * 64 + 62, 0] = np.nan
    corr[1024 + 2 * CHUNK + 7 * 64 + 63, 2] = np.inf
    s32 = _scores(codes, corr, dim, qq[:nq], qc[:nq], 4, 1, 1)
    assert all(np.isnan(s).sum() == 1 and np.isposinf(s).sum() == 1 for s in s32)
    ix = _index(codes, corr, dim)
    try:
        _check_tpw(ix, lambda: ix.search_batch(qq[:nq], qc[:nq], 4, 1, RAGGED_K), [_expected(s, RAGGED_K) for s in s32], "NaN and +inf", min_fallbacks=nq)
    finally:
        ix.close()


# ------------------------------------------------------------------------------------------------ 6. other widths and settings
@pytest.mark.parametrize("dim", [1024, 1536])
def test_full_list_other_widths(dim):
    codes, corr, qq, qc, s32 = _full(dim)
    ix = _index(codes, corr, dim)
    try:
        _check_tpw(ix, lambda: ix.search_batch(qq, qc, 4, 1, RAGGED_K), [_expected(s, RAGGED_K) for s in s32], "%d-d" % dim)
    finally:
        ix.close()


@pytest.mark.parametrize("data", ["full_list", "ragged_end"])
def test_load_arms_and_grid_orders(data):
    """resident_mb 0 streams every chunk - through the twins only because row_sums and digit_planes are set explicitly; 1 keeps part of the
    chunks resident, -1 all of them; each under the plain grid and the one that runs a chunk's queries back to back"""
    codes, corr, qq, qc, s32 = _full() if data == "full_list" else _ragged_end()
    want = [_expected(s, RAGGED_K) for s in s32]
    ix = _index(codes, corr, 768)
    try:
        first = None
        for mb in (0, 1, -1):
            ix.set_option("resident_mb", mb)
            ix.set_option("row_sums", 1 if mb == 0 else -1)
            ix.set_option("digit_planes", 1 if mb == 0 else -1)
            for share in (1, 32):
                ix.set_option("l2_share", share)
                got = _check_tpw(ix, lambda: ix.search_batch(qq, qc, 4, 1, RAGGED_K), want, "%s resident_mb %d l2_share %d" % (data, mb, share))
                assert (ix.stats()["resident_bytes"] == 0) == (mb == 0)
                if first is None:
                    first = got
                for a, b in zip(got, first):
                    np.testing.assert_array_equal(a, b, err_msg="resident_mb %d l2_share %d" % (mb, share))
    finally:
        ix.close()
