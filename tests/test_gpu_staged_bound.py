"""GPU: the staged twin of the many-tile digit sweep (bbq_scan_staged_kernel, sweep_wave_tiles' STG in bbq_scan_body.h; staged_bound_for in
bbq_core.cpp) leaves the unit digit plane of a row's last 4 dwords behind the bound: stage one tests the widened bound at the midpoint of the
interval the row's D lies in, stage two - for the tiles where some row passed - resolves the rest and applies the unchanged bound.  It
changes no answer: a 768-d launch with 8 tiles per wave (the default) takes the twin behind every segment that left a threshold,
tiles_per_wave 1, 2 and 4 select kernels without stages, and under each the answer is heap_topk of the oracle's scores - indices, f32
score BITS and counts - and identical to the others'.  No tolerances.  Which kernel a launch took shows in no answer: the library counts
the launches of the twin (bbq_staged_launches) and the test asserts the count of every call.

Shapes: 3 x 512 + 37 rows - behind the dense first segment of 1024 rows a full chunk and one of 37 rows, whose wave has one tile and that
tile 37 rows - at 768-d (the width that has the twin) and at 1024-d and 1536-d (which have none); 33 queries, so one launch group of 32
and one of a single query; k 1 and 100; the three similarities.
  ties      copies of one row in both sparse chunks and in the last, partial tile, against the query made from its bits: they pass any bound
  hostile   a NaN lower interval (no bound excludes it; the query is flagged and answered densely), a +inf additional correction, a huge
            and a tiny pair of intervals in the sparse chunks
The last query has an interval width below f32's normal range: no f32 images, the f64 bound behind the loop (its launch group keeps the
kernel without stages, the other 32 queries' group takes the staged one)."""
import functools

import numpy as np
import pytest

from bbqlib import bbq_amd as B, capi
from test_gpu_l2_share import CDP, _expected, _scores, _synthetic, bits32

pytestmark = pytest.mark.gpu

N, NQ, FIRST = 3 * 512 + 37, 33, 1024
TPW = (4, 8, -1, 1)            # 8 and -1: the staged twin at 768-d; 4 and 1: kernels without stages


@functools.lru_cache(maxsize=None)
def _data(dim, data, sim):
    codes, corr, qq, qc = _synthetic(1000 + dim, N, dim, 1, 4, NQ)
    codes, corr, qq, qc = codes.copy(), corr.copy(), qq.copy(), qc.copy()
    if data == "ties":
        good = FIRST + 70
        at = [FIRST + 3, good, FIRST + 511, FIRST + 512, N - 1]
        codes[at], corr[at] = codes[good], corr[good]
        if sim != 0:   # (EUCLIDEAN clamps a row this close to the query: there the ties are ordinary rows' scores)
            qq[0] = (np.unpackbits(codes[good])[:dim] * 15).astype(np.uint8)
            qc[0, 3] = qq[0].sum()
    else:
        corr[FIRST + 64 + 5, 0] = np.nan
        corr[FIRST + 300, 2] = np.inf
        corr[FIRST + 130, :2] = (-1e20, 1e20)
        corr[FIRST + 512 + 36, :2] = (-1e-30, 1e-30)
        corr[FIRST + 7, :2] = (3e38, 3e38)
    qc[NQ - 1, 1] = qc[NQ - 1, 0] + 1e-40    # ly below f32's normal range: this query keeps the f64 bound
    with np.errstate(all="ignore"):
        s32 = _scores(codes, corr, dim, qq, qc, 4, sim, 1)
    for a in (codes, corr, qq, qc, *s32):
        a.setflags(write=False)
    return codes, corr, qq, qc, s32


@pytest.mark.parametrize("sim", [0, 1, 2])
@pytest.mark.parametrize("data", ["ties", "hostile"])
@pytest.mark.parametrize("dim", [768, 1024, 1536])
def test_staged_twin_changes_no_answer(dim, data, sim):
    codes, corr, qq, qc, s32 = _data(dim, data, sim)
    ix = B.Index(codes, corr, dim, CDP, corrections="compact")
    try:
        ix.set_option("first_segment_rows", FIRST)
        ix.set_option("segment_growth", 2)
        ix.set_option("replay_threads", 4)
        for k in (1, 100):
            want = [_expected(s, k) for s in s32]
            first = None
            for v in TPW:
                ix.set_option("tiles_per_wave", v)
                ix.reset_stats()
                before = capi.staged_launches()
                idx, sc, cnt = ix.search_batch(qq, qc, 4, sim, k)
                # the twin ran where it exists - 768-d, 8 tiles per wave: the group of 32 queries with f32 images, behind the first segment
                # (two sparse launches) - and nowhere else: not at another width or tile count, not for the group of the query without images
                assert capi.staged_launches() - before == (2 if dim == 768 and v in (8, -1) else 0), "tiles_per_wave %d: staged launches" % v
                st = ix.stats()
                print("%d-d %s sim %d k %d tiles_per_wave %d: host_replays %d dense_fallbacks %d candidates %d" % (
                    dim, data, sim, k, v, st["host_replays"], st["dense_fallbacks"], st["candidates"]))
                for q, (wi, ws) in enumerate(want):
                    assert cnt[q] == len(wi), "tiles_per_wave %d, k %d, query %d: count" % (v, k, q)
                    np.testing.assert_array_equal(idx[q, :cnt[q]], wi, err_msg="tiles_per_wave %d, k %d, query %d" % (v, k, q))
                    np.testing.assert_array_equal(bits32(sc[q, :cnt[q]]), bits32(ws), err_msg="tiles_per_wave %d, k %d, query %d" % (v, k, q))
                got = (idx, bits32(sc), cnt, st["candidates"])
                if first is None:
                    first = got
                for a, b in zip(got, first):
                    np.testing.assert_array_equal(a, b, err_msg="tiles_per_wave %d against 4, k %d" % (v, k))
    finally:
        ix.close()
