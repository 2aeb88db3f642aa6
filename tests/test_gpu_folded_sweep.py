"""GPU: the tile loop of the sweeps with several tiles per wave (option tiles_per_wave 2, 4, 8; sweep_wave_tiles in bbq_scan_body.h) loads its
tiles through a buffer descriptor that is rebased per tile on the scalar unit - a lane's part of an address is a 32-bit offset computed once
per wave - issues a tile's nine loads under one scalar branch behind the previous tile's bound, takes the bound's verdicts as a scalar mask
straight from the compare, and removes the rows beyond the index from that mask on the scalar unit.  Its bound is the folded form
(folded_bound_passes: g from the digit counts, a threshold per tile computed once per wave for all its tiles and read with v_readlane;
tests/test_bound_folded_cpu.py holds its arithmetic to the exact score).  None of it changes an answer.

The criterion is test_gpu_deferred_exact's: under every value in (1, 2, 4, 8) the answer is heap_topk of the oracle's scores - indices, f32
score BITS and counts - and the three arrays are identical across the four values.  No tolerances.

What can go wrong, and the smallest shapes that show it (a "planted" row is a copy of one row that scores above every other row for the
query made from its bits, so it passes the bound whatever the threshold):
  the last tile's validity    1536 + 1, 63, 64 and 65 rows at 768-d, the last row planted: the rows of a partial last tile are taken out of the
                              ballot by a scalar mask of rows_here bits - 1 and 63 bits, none at 64, and at 65 a full tile in front of a
                              tile of one row in the same wave
  both load arms, one launch  resident_mb 1 keeps the first 20 chunks of every launch's range resident and streams the others; a planted row
                              in EVERY chunk behind the dense first segment - so in the first and the last chunk of either arm of every
                              launch, whatever the segment plan - under l2_share 1 and 32: the descriptor's rebasing and the `nt` arm
  widths                      the ragged grid (19 044 rows, 38 chunks, the last partly filled) at 1024-d and 1536-d: chunks 4-5, 6-7 and
                              8-11 of a row lie beyond the 4 KB an instruction's own offset reaches and go through the scalar offset, and
                              so does the correction word at every width
  similarities                all three on the ragged grid: EUCLIDEAN reads the minimum side of add_range through the descriptor's
                              scalar offset
  fast_bound 0                the threshold image of a query without f32 images is NaN in the loop: every tile's threshold is NaN and every
                              valid row is deferred
  a wave with fewer tiles     the thresholds' one load takes the wave's last tile's add_range entry in the lanes beyond its tiles: the
                              ragged ends above (1, 2 and 8 of a wave's tiles exist)
  saturated scores            EUCLIDEAN queries whose additional correction is so negative that every score clamps to +0: the threshold's
                              z image is -inf and every row passes the bound, none beats the key; with a NaN row alone in the index's
                              last tile and a +inf row in the last lane of the tile in front of it"""
import numpy as np
import pytest

from bbqlib import bbq_amd as B
from test_gpu_deferred_exact import CHUNK, RAGGED_END_N, _check_tpw, _index, _planted
from test_gpu_early_loads import _ragged, _ragged_want, _expected, _scores, RAGGED_K
from test_gpu_row_sums import RAGGED_N

pytestmark = pytest.mark.gpu

FIRST_SPARSE_CHUNK = 2   # first_segment_rows 1024: the rows in front are swept densely


# ------------------------------------------------------------------------------------------------ 1. the last tile's validity
@pytest.mark.parametrize("tail", [1, 63, 64, 65])
def test_last_tile_validity(tail):
    n = 3 * CHUNK + tail
    codes, corr, qq, qc, s32 = _planted(768, n, (n - 1,))
    want = [_expected(s, RAGGED_K) for s in s32]
    assert want[0][0][0] == n - 1, "the last valid row is the planted query's best"
    ix = _index(codes, corr, 768)
    try:
        _check_tpw(ix, lambda: ix.search_batch(qq, qc, 4, 1, RAGGED_K), want, "%d rows" % n)
    finally:
        ix.close()


# ------------------------------------------------------------------------------------------------ 2. both load arms in one launch
def _row_in_every_chunk():
    n_chunks = (RAGGED_N + CHUNK - 1) // CHUNK
    rows = [c * CHUNK + (c * 37) % CHUNK for c in range(FIRST_SPARSE_CHUNK, n_chunks - 1)]
    return tuple(rows + [RAGGED_N - 1])


def test_both_load_arms_in_one_launch():
    rows = _row_in_every_chunk()
    assert len(rows) <= RAGGED_K and len({r // CHUNK for r in rows}) == len(rows)
    codes, corr, qq, qc, s32 = _planted(768, RAGGED_N, rows)
    want = [_expected(s, RAGGED_K) for s in s32]
    assert set(rows) <= set(want[0][0].tolist()), "every planted row is in the planted query's answer"
    ix = _index(codes, corr, 768)
    try:
        ix.set_option("resident_mb", 1)
        first = None
        for share in (1, 32):
            ix.set_option("l2_share", share)
            got = _check_tpw(ix, lambda: ix.search_batch(qq, qc, 4, 1, RAGGED_K), want, "resident_mb 1 l2_share %d" % share)
            resident = ix.stats()["resident_bytes"]
            print("resident_bytes %d of %d" % (resident, RAGGED_N * ix.bytes_per_row))
            assert 0 < resident < (RAGGED_N // CHUNK) * CHUNK * ix.bytes_per_row, "some chunks resident, some streamed"
            if first is None:
                first = got
            for a, b in zip(got, first):
                np.testing.assert_array_equal(a, b, err_msg="l2_share %d" % share)
    finally:
        ix.close()


# ------------------------------------------------------------------------------------------------ 3. widths, 4. similarities, 5. fast_bound 0
@pytest.mark.parametrize("dim,sim,fast_bound", [(1024, 1, 1), (1536, 1, 1), (768, 0, 1), (768, 1, 1), (768, 2, 1), (768, 0, 0)])
def test_ragged_grid(dim, sim, fast_bound):
    codes, corr, qq, qc = _ragged(dim)
    _, want = _ragged_want(dim, sim)
    ix = _index(codes, corr, dim)
    try:
        ix.set_option("fast_bound", fast_bound)
        _check_tpw(ix, lambda: ix.search_batch(qq, qc, 4, sim, RAGGED_K), want, "%d-d sim %d fast_bound %d" % (dim, sim, fast_bound))
    finally:
        ix.close()


# ------------------------------------------------------------------------------------------------ 6. saturated scores
def test_saturated_threshold_with_nan_and_inf_in_the_last_tiles():
    dim, nq = 768, 3
    codes, corr, qq, qc = _ragged(dim)
    codes, corr = codes[:RAGGED_END_N].copy(), corr[:RAGGED_END_N].copy()
    corr[RAGGED_END_N - 1, 0] = np.nan     # alone in the index's last tile
    corr[RAGGED_END_N - 2, 2] = np.inf     # lane 63 of the full tile in front of it
    qq, qc = qq[:nq], qc[:nq].copy()
    qc[:2, 2] = -1e6                       # 1 / (1 + qadd + xadd - 2 s) < 0 for every row: the score clamps to +0
    s32 = _scores(codes, corr, dim, qq, qc, 4, 0, 1)
    assert all((s[:RAGGED_END_N - 1] == 0).all() for s in s32[:2]), "two queries whose every score is +0"
    assert all(np.isnan(s).sum() == 1 for s in s32) and (s32[2][:RAGGED_END_N - 2] > 0).all(), "and an ordinary one"
    ix = _index(codes, corr, dim)
    try:
        _check_tpw(ix, lambda: ix.search_batch(qq, qc, 4, 0, RAGGED_K), [_expected(s, RAGGED_K) for s in s32], "saturated", min_fallbacks=nq)
    finally:
        ix.close()
