"""GPU: option digit_planes - the per-query sparse sweep of a compact 1-bit index scores a 4-plane query in three planes of ternary
digits (q - 4 = t0 + 3 t1 + 9 t2; qcDist = 4 ones + a0 + 3 a1 + 9 a2 - K, bbq_device.h) instead of four bit-planes - changes no answer.

The criterion everywhere is test_gpu_row_sums.py's: indices, f32 score BITS and counts under digit_planes 1 equal those under
digit_planes 0, the digit_planes 0 results are heap_topk of the oracle's scores, and host_replays / dense_fallbacks do not differ between
the two values.  No tolerances: the dot product is an exact integer.

Which rows the digit form scores.  Only a sparse launch can run it: first_segment_rows 1024 / segment_growth 2 leave the rows from 1024
on to sparse launches as long as 4 (k + 1) <= 1024; a larger k grows the dense first segment (4 096 rows at k = 1000, the whole of a
3 000-row index).  The table test therefore runs its index three ways: k = 1000 unfiltered as the issue states it, k = 1000 through a
filter that accepts every row - a filtered plan has sparse segments only, so EVERY row is scored by the digit form of the filtered family
and a third of them come back with their score bits - and k = 100 unfiltered, where the rows from 1024 on (the extreme rows among them)
go through the digit form of the unfiltered family.

Which widths have the form: 6, 8 and 12 chunks (768-d, 1024-d, 1536-d) unfiltered and 6 chunks filtered, where it was measured faster
(digit_twin, bbq_scan_body.h).  The other widths here - 128-d, 100-d, 200-d - answer through the plane form under either value."""
import functools

import numpy as np
import pytest

from bbqlib import bbq_amd as B, capi
from test_gpu_l2_share import CDP, _expected, _scores, _synthetic, bits32
from test_gpu_row_sums import (KIND_A, KIND_B, RAGGED_K, T_DIM, T_K, T_QB, T_SIM, _cat, _ragged, _ragged_want, _rows, _small_segments,
                               _sums, _trap_queries, _updated, _want, prove_trap)

pytestmark = pytest.mark.gpu


def _check_digit_planes(ix, run, want, values=(0, 1)):
    """run() -> (idx [nq][k], scores, counts) under each value of digit_planes: the first equals `want`, the others equal the first"""
    first = first_stats = None
    for v in values:
        ix.set_option("digit_planes", v)
        ix.reset_stats()
        idx, sc, cnt = run()
        st = ix.stats()
        st = (st["host_replays"], st["dense_fallbacks"])
        if first is None:
            first, first_stats = (idx, bits32(sc), cnt), st
            for q, (wi, ws) in enumerate(want):
                assert cnt[q] == len(wi), "digit_planes %d, query %d" % (v, q)
                np.testing.assert_array_equal(idx[q, :cnt[q]], wi, err_msg="digit_planes %d, query %d" % (v, q))
                np.testing.assert_array_equal(bits32(sc[q, :cnt[q]]), bits32(ws), err_msg="digit_planes %d, query %d" % (v, q))
        else:
            np.testing.assert_array_equal(cnt, first[2], err_msg="digit_planes %d" % v)
            np.testing.assert_array_equal(idx, first[0], err_msg="digit_planes %d" % v)
            np.testing.assert_array_equal(bits32(sc), first[1], err_msg="digit_planes %d" % v)
            assert st == first_stats, "digit_planes %d: host_replays / dense_fallbacks %r, with digit_planes %d %r" % (v, st, values[0], first_stats)
    ix.set_option("digit_planes", -1)


# ------------------------------------------------------------------------------------------------ 1. the ragged grid
# 19 044 rows = 38 chunks, the last one partly filled, 37 queries = one launch group of 32 plus 5.  W = 6, 8 and 12 (1536-d, the twin with
# a compiler barrier behind each chunk) have a digit twin; one chunk (128-d; 100-d, the last byte partly used) and the run-time width
# (200-d: two chunks) keep the plane form and must answer the same through it
@pytest.mark.parametrize("sim", [0, 1, 2])
@pytest.mark.parametrize("dim", [128, 768, 1024, 100, 1536, 200])
def test_ragged_grid(dim, sim):
    codes, corr, qq, qc = _ragged(dim)
    _, want = _ragged_want(dim, sim)
    ix = B.Index(codes, corr, dim, CDP, corrections="compact")
    try:
        _small_segments(ix)
        _check_digit_planes(ix, lambda: ix.search_batch(qq, qc, 4, sim, RAGGED_K), want)
    finally:
        ix.close()


def test_stray_bits_behind_the_last_dimension():
    """764-d rows (6 chunks: a width with a digit twin) use 4 bits of their last byte.  The library stores a row's bytes as they come, so a caller's stray bits in the other 4
    are in the tiles, in the row's popcount and - here - in its quantizedComponentSum, and the index is compact all the same.  The plane
    form never sees them (the planes are 0 there); the digit form's 4 * ones counts them, and its masks hold the value 0 (digits -1, -1,
    0) in every padding position so that they weigh 4 - 1 - 3 = 0.  Every pattern of the four stray bits, among rows without any"""
    dim = 764
    codes, corr, qq, qc = _ragged(dim)
    codes, corr = codes.copy(), corr.copy()
    assert codes.shape[1] == 96 and not (codes[:, -1] & 0x0F).any()
    stray = np.arange(len(codes)) % 23
    codes[:, -1] |= np.where(stray < 16, stray, 0).astype(np.uint8)
    corr[:, 3] = _sums(codes)   # the sum over every stored bit: what keeps the index compact
    want = [_expected(s, RAGGED_K) for s in _scores(codes, corr, dim, qq, qc, 4, 1, 1)]
    ix = B.Index(codes, corr, dim, CDP, corrections="compact")
    try:
        assert ix.bytes_per_row == 96 + 4, "the compact layout: the stray bits are part of the rows' sums"
        _small_segments(ix)
        _check_digit_planes(ix, lambda: ix.search_batch(qq, qc, 4, 1, RAGGED_K), want)
    finally:
        ix.close()


# ------------------------------------------------------------------------------------------------ 2. every table entry at every bit position
TABLE_N, TABLE_K, TABLE_RANDOM_Q = 3000, 1000, 7


@functools.lru_cache(maxsize=None)
def _table(dim):
    """3 000 rows (the last tile holds 56), all-ones, all-zeros and single-bit rows among random ones - every bit position of the row once,
    in front of and behind row 1024 - and 16 constant queries (every dimension = v), one with q[d] = d % 16, and random ones"""
    pb = (dim + 7) // 8
    codes, corr, rq, rc = _synthetic(900 + dim, TABLE_N, dim, 1, 4, TABLE_RANDOM_Q)
    codes = codes.copy()
    rng = np.random.default_rng(dim)
    ones_at = np.r_[5:9, 1030:1040, 2040:2050, 2990:2993]
    zeros_at = np.r_[9:13, 1050:1060, 2060:2070, 2993:2996]
    codes[ones_at] = 255
    if dim % 8:
        codes[ones_at, -1] = (0xFF << (8 - dim % 8)) & 0xFF
    codes[zeros_at] = 0
    single = np.r_[100:100 + dim, 1100:1100 + dim] if dim <= 128 else np.r_[1100:1100 + dim]
    bit = np.tile(np.arange(dim), len(single) // dim)
    codes[single] = 0
    codes[single, bit >> 3] = (0x80 >> (bit & 7)).astype(np.uint8)
    corr = corr.copy()
    corr[:, 3] = _sums(codes)
    const = np.repeat(np.arange(16, dtype=np.uint8)[:, None], dim, axis=1)
    ramp = (np.arange(dim) % 16).astype(np.uint8)[None, :]
    qq = np.concatenate([const, ramp, rq])
    qc = np.empty((len(qq), 4))
    qc[:] = rc[rng.integers(0, TABLE_RANDOM_Q, len(qq))]
    qc[-TABLE_RANDOM_Q:] = rc
    qc[:, 3] = qq.sum(axis=1)
    s32 = _scores(codes, corr, dim, qq, qc, 4, 1, 1)
    for a in (codes, corr, qq, qc, *s32):
        a.setflags(write=False)
    assert pb * 8 >= dim and len(codes) == TABLE_N
    return codes, corr, qq, qc, s32


@pytest.mark.parametrize("how", ["k1000", "k1000_all_rows_sparse", "k100"])
@pytest.mark.parametrize("dim", [768, 128])
def test_every_table_entry_at_every_bit_position(dim, how):
    codes, corr, qq, qc, s32 = _table(dim)
    assert int(qq.max()) == 15 and len(qq) == 17 + TABLE_RANDOM_Q
    k = 100 if how == "k100" else TABLE_K
    ix = B.Index(codes, corr, dim, CDP, corrections="compact")
    try:
        _small_segments(ix)
        want = [_expected(s, k) for s in s32]
        if how == "k1000_all_rows_sparse":
            with capi.Filter(ix, np.ones(TABLE_N, bool)) as flt:
                _check_digit_planes(ix, lambda: ix.search_filtered_batch(qq, qc, 4, 1, k, flt), want)
        else:
            _check_digit_planes(ix, lambda: ix.search_batch(qq, qc, 4, 1, k), want)
    finally:
        ix.close()


# ------------------------------------------------------------------------------------------------ 3. few queries, and a filtered search
@pytest.mark.parametrize("nq", [1, 3])
def test_few_queries(nq):
    """calls with few queries walk the index in other segments and their sweeps append the candidates to the lists themselves.  A single
    query: the fused latency path (which stages no digit masks), then the general one"""
    codes, corr, qq, qc = _ragged(768)
    _, want = _ragged_want(768, 1)
    ix = B.Index(codes, corr, 768, CDP, corrections="compact")
    try:
        _small_segments(ix)
        for fused in (1, 0):
            ix.set_option("latency_fused", fused)
            _check_digit_planes(ix, lambda: ix.search_batch(qq[:nq], qc[:nq], 4, 1, RAGGED_K), want[:nq])
    finally:
        ix.close()


def test_filtered_search():
    """a sparse mask, every fifth tile empty (its wave loads nothing): the filtered instantiation"""
    codes, corr, qq, qc = _ragged(768)
    s32, _ = _ragged_want(768, 1)
    n = len(codes)
    mask = np.random.default_rng(8).random(n) < 0.08
    mask[(np.arange(n) // 64) % 5 == 3] = False
    ix = B.Index(codes, corr, 768, CDP, corrections="compact")
    try:
        _small_segments(ix)
        with capi.Filter(ix, mask) as flt:
            want = [_expected(s, RAGGED_K, mask) for s in s32]
            _check_digit_planes(ix, lambda: ix.search_filtered_batch(qq, qc, 4, 1, RAGGED_K, flt), want)
    finally:
        ix.close()


# ------------------------------------------------------------------------------------------------ 4. strict mode
def test_strict_mode_keeps_its_answers():
    """resident_mb 0: the automatic row_sums is off, so no launch has a digit twin to take, whatever digit_planes says.  Answers equal."""
    codes, corr, qq, qc = _ragged(768)
    _, want = _ragged_want(768, 1)
    ix = B.Index(codes, corr, 768, CDP, corrections="compact")
    try:
        _small_segments(ix)
        ix.set_option("resident_mb", 0)
        _check_digit_planes(ix, lambda: ix.search_batch(qq, qc, 4, 1, RAGGED_K), want, values=(0, -1, 1))
        _check_digit_planes(ix, lambda: ix.search_batch(qq, qc, 4, 1, RAGGED_K), want, values=(-1, 1, 0))
        assert ix.stats()["resident_bytes"] == 0
    finally:
        ix.close()


# ------------------------------------------------------------------------------------------------ 5. option validation
def test_option_validation():
    codes, corr, qq, qc = _ragged(128)
    ix = B.Index(codes[:1024], corr[:1024], 128, CDP)
    try:
        for bad in (-2, 2, 7):
            with pytest.raises(capi.BBQError) as e:
                ix.set_option("digit_planes", bad)
            assert e.value.code == capi.ERR_INVALID_ARG
        for good in (-1, 0, 1):
            ix.set_option("digit_planes", good)
    finally:
        ix.close()


# ------------------------------------------------------------------------------------------------ 6. row sums under mutation
def test_row_sums_under_mutation():
    """the digit form's qcDist depends on `ones`, where the plane form only took it for the bound: a stale sum is a wrong score, not a
    lost row.  One update that turns all-ones rows sparse and all-zeros rows full (test_gpu_row_sums._updated, whose traps are proved
    there and here), then one append across a tile boundary - 3 000 rows end 8 lanes short of one - with all-ones rows landing in the
    padding lanes, whose entries were 0."""
    (codes, corr), ords, new, (codes2, corr2) = _updated()
    qq, qc = _trap_queries()
    prove_trap(codes2, corr2, _sums(codes), KIND_A + KIND_B)
    step = _cat(_rows("dense_top", 30, 41), _rows("sparse_top", 30, 42), _rows("bg", 40, 43))
    codes3, corr3 = _cat((codes2, corr2), step)
    ix = B.Index(codes, corr, T_DIM, CDP, corrections="compact")
    try:
        _small_segments(ix)
        run = lambda: ix.search_batch(qq, qc, T_QB, T_SIM, T_K)
        _check_digit_planes(ix, run, _want(codes, corr))
        ix.update_rows(ords, *new)
        _check_digit_planes(ix, run, _want(codes2, corr2))
        ix.append_rows(*step)
        assert ix.n == len(codes3) and len(codes2) % 64 != 0 and len(codes3) // 64 > len(codes2) // 64
        _check_digit_planes(ix, run, _want(codes3, corr3))
    finally:
        ix.close()
