"""CPU: the grouped search's contract restated in numpy - which groups are live and where they rank (bbq_groups_plan, held to the
restatement over every layout and mask the GPU test uses, and its refusals) and which row represents a group for a query
(`representatives`, the model tests/test_gpu_grouped.py imports).  The status rule is the span search's over the representatives'
scores (test_spans_cpu.expected_status)."""
import functools

import numpy as np
import pytest

import test_spans_cpu as SC               # expected_status: the rule, shared with the span search
import test_spans_filtered_cpu as FC      # masks: shared with the filtered span search
from bbqlib import capi

BIG = 1600                                # a group of more than three chunks of 512 rows ...
BIG_AT = 37                               # ... that starts in the middle of a tile


def offsets_of(sizes):
    off = np.zeros(len(sizes) + 1, np.int64)
    off[1:] = np.cumsum(sizes)
    return off


def _tiled(n, s):
    """groups of s rows, the last one shorter"""
    return np.unique(np.append(np.arange(0, n, s), n)).astype(np.int64)


@functools.lru_cache(maxsize=None)
def layouts(n):
    """the group layouts of an index of n >= 1 rows, by name, each where it fits; read-only"""
    rng = np.random.default_rng(4321 + n)
    out = {"singletons": np.arange(n + 1, dtype=np.int64), "one_group": np.array([0, n], np.int64)}
    for s in (63, 64, 65, 512, 513):
        if n > s:
            out["groups_of_%d" % s] = _tiled(n, s)
    if n >= BIG_AT + BIG + 1:
        out["big_mid_tile"] = np.array([0, BIG_AT, BIG_AT + BIG, n], np.int64)
    sizes = []
    while sum(sizes) < n:
        sizes.append(min(int(rng.integers(1, 21)), n - sum(sizes)))
    out["random_1_20"] = offsets_of(sizes)
    if n >= 3:                            # empty groups first, last and three in a row between two non-empty ones
        cut = sorted({1, n // 2, n - 1} | set(_tiled(n, 7).tolist()) - {0, n})
        out["empty_groups"] = np.array([0, 0] + cut[:2] + [cut[1]] * 3 + cut[2:] + [n, n], np.int64)
    for name, off in out.items():
        assert off[0] == 0 and off[-1] == n and (np.diff(off) >= 0).all(), name
        off.setflags(write=False)
    return out


def chunk_edge_layouts(n):
    """groups that meet the edges of 512-row chunks and 64-row tiles in every way: ending at one, beginning at one, crossing one by a
    row on either side, crossing two chunks, and whole chunks"""
    cuts = {0, n}
    for c in range(512, n, 512):
        cuts |= {c - 70, c - 1, c + 1, c + 64, c + 130}
    a = np.array(sorted(x for x in cuts if 0 <= x <= n), np.int64)
    b = np.array(sorted({0, n} | {x for x in (3, 511, 512, 513, 1024, 1600) if x < n}), np.int64)
    c = np.array(sorted({0, n} | {x for x in (500, 1700) if x < n}), np.int64)              # one group over two chunk edges
    d = np.array(sorted({0, n} | set(range(512, n, 512))), np.int64)                          # every group one chunk
    return {"around_chunk_edges": a, "on_and_beside_edges": b, "across_two_edges": c, "whole_chunks": d}


def plan(offsets, mask):
    """bbq_groups_plan restated: (slot per group - its rank among the live groups, -1 without an accepted row - and L)"""
    off = np.asarray(offsets, np.int64)
    live = np.array([bool(mask[b:e].any()) for b, e in zip(off[:-1], off[1:])], bool)
    slot = np.where(live, np.cumsum(live) - 1, -1).astype(np.int32)
    return slot, int(live.sum())


def rank_keys(scores):
    """the library's score keys as int64, a NaN as 0: below every number (the smallest number's key, -inf's, is 0x007fffff)"""
    s = np.ascontiguousarray(scores, np.float32)
    bits = s.view(np.uint32).astype(np.int64)
    key = np.where(bits & 0x80000000, ~bits & 0xffffffff, bits | 0x80000000)
    return np.where(np.isnan(s), 0, key)


def representatives_slow(scores, offsets, mask):
    """the definition, group by group: the accepted row of the greatest rank, the lowest ord among equals"""
    key = rank_keys(scores)
    ords, groups = [], []
    for g, (b, e) in enumerate(zip(offsets[:-1], offsets[1:])):
        rows = np.arange(b, e)[np.asarray(mask[b:e], bool)]
        if len(rows):
            ords.append(rows[np.argmax(key[rows])])          # argmax: the first of the greatest
            groups.append(g)
    return np.array(ords, np.int64), np.array(groups, np.int64)


def representatives(scores, offsets, mask):
    """per live group, ascending: (the ord of its representative for a query whose rows score `scores`, the group).  A group's
    representative is its accepted row whose score ranks highest - NaN below every number, numbers by key (-0.0 below +0.0) - and among
    rows of equal rank the lowest ord; the same answer as representatives_slow, in one pass"""
    off = np.asarray(offsets, np.int64)
    n = int(off[-1])
    if n == 0:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    assert n < (1 << 30)
    rank = rank_keys(scores) * (1 << 30) + (n - np.arange(n))         # > 0 for every row; greater = better
    rank = np.where(np.asarray(mask, bool), rank, 0)
    nonempty = np.nonzero(np.diff(off) > 0)[0]
    best = np.maximum.reduceat(rank, off[nonempty])
    live = best > 0
    return (n - (best[live] & ((1 << 30) - 1))).astype(np.int64), nonempty[live].astype(np.int64)


def test_the_model_on_small_cases():
    f, nan = np.float32, np.nan
    s = np.array([1, 3, 3, nan, nan, f(-0.0), f(0.0), 2, nan], np.float32)
    off = np.array([0, 3, 3, 5, 7, 8, 9], np.int64)
    everything = np.ones(9, bool)
    ords, groups = representatives(s, off, everything)
    assert ords.tolist() == [1, 3, 6, 7, 8] and groups.tolist() == [0, 2, 3, 4, 5]     # lowest ord of equals; all NaN: the lowest; +0 over -0
    keep = np.array([1, 0, 1, 0, 1, 1, 0, 0, 1], bool)
    ords, groups = representatives(s, off, keep)
    assert ords.tolist() == [2, 4, 5, 8] and groups.tolist() == [0, 2, 3, 5]           # group 4 has no accepted row
    assert plan(off, keep)[0].tolist() == [0, -1, 1, 2, -1, 3] and plan(off, keep)[1] == 4
    one = np.array([2, nan, 5, 5], np.float32)
    assert representatives(one, np.array([0, 4]), np.ones(4, bool))[0].tolist() == [2]   # a NaN inside a larger group never represents
    assert representatives(one, np.array([0, 4]), np.array([0, 1, 0, 0], bool))[0].tolist() == [1]
    assert len(representatives(one, np.array([0, 4]), np.zeros(4, bool))[0]) == 0
    assert len(representatives(np.zeros(0, np.float32), np.array([0, 0, 0]), np.zeros(0, bool))[0]) == 0
    assert rank_keys([-np.inf])[0] == 0x007fffff and rank_keys([nan])[0] == 0 and rank_keys([f(-0.0)])[0] + 1 == rank_keys([f(0.0)])[0]


def test_the_fast_model_is_the_definition():
    rng = np.random.default_rng(7)
    for n in (1, 2, 70, 700):
        s = rng.standard_normal(n).astype(np.float32)
        s[rng.random(n) < 0.2] = np.nan
        s[rng.random(n) < 0.3] = np.float32(1.5)                   # many equal scores
        s[rng.random(n) < 0.1] = np.float32(-0.0)
        s[rng.random(n) < 0.1] = np.float32(0.0)
        for off in layouts(n).values():
            for mask in FC.masks(n).values():
                a, b = representatives(s, off, mask), representatives_slow(s, off, mask)
                np.testing.assert_array_equal(a[0], b[0])
                np.testing.assert_array_equal(a[1], b[1])
                assert len(a[0]) == plan(off, mask)[1]
                np.testing.assert_array_equal(plan(off, mask)[0][a[1]], np.arange(len(a[1])))


def test_the_layouts():
    for n in (1, 2, 12, 100, 1000, 2100):
        lay = layouts(n)
        assert (np.diff(lay["singletons"]) == 1).all() and len(lay["one_group"]) == 2
        assert ("big_mid_tile" in lay) == (n >= 1638) and ("groups_of_513" in lay) == (n > 513)
        if n >= 3:
            e = lay["empty_groups"]
            assert e[1] == 0 and e[-2] == n and (np.diff(e) == 0).sum() >= 5
            z = np.diff(e) == 0
            assert (z[:-2] & z[1:-1] & z[2:]).any()                # three in a row
        sizes = np.diff(lay["random_1_20"])
        assert sizes.min() >= 1 and sizes.max() <= 20
    big = layouts(2100)["big_mid_tile"]
    assert big[1] % 64 != 0 and big[2] - big[1] > 1536
    for off in chunk_edge_layouts(2100).values():
        assert off[0] == 0 and off[-1] == 2100 and (np.diff(off) > 0).all()


@pytest.mark.parametrize("n", [1, 2, 12, 100, 1000, 2100])
def test_groups_plan_is_the_restatement(n):
    """bbq_groups_plan over every layout x mask; the accept words' bits beyond n are ignored"""
    everything = dict(layouts(n))
    if n > 1024:
        everything.update(chunk_edge_layouts(n))
    for lname, off in everything.items():
        for mname, mask in FC.masks(n).items():
            slot, live = capi.groups_plan(off, n, mask)
            want_slot, want_live = plan(off, mask)
            np.testing.assert_array_equal(slot, want_slot, err_msg="%s %s" % (lname, mname))
            assert live == want_live, (lname, mname)
        slot, live = capi.groups_plan(off, n, None)                                  # no filter: every non-empty group is live
        np.testing.assert_array_equal(slot, plan(off, np.ones(n, bool))[0])
        assert live == (np.diff(off) > 0).sum()
    # a set bit beyond the last row is no accepted row: the last group stays dead
    import ctypes as C
    words = capi.pack_mask(np.zeros(n, bool)).copy()
    if n % 64:
        words[-1] |= np.uint64(1) << np.uint64(n % 64)
        off = np.array([0, n], np.int64)
        slot, live = np.zeros(1, np.int32), C.c_int64(-1)
        assert capi.lib().bbq_groups_plan(off.ctypes.data, 1, n, words.ctypes.data, slot.ctypes.data, C.byref(live)) == capi.OK
        assert live.value == 0 and slot[0] == -1


def test_groups_plan_of_an_empty_index():
    slot, live = capi.groups_plan([0], 0)
    assert len(slot) == 0 and live == 0
    slot, live = capi.groups_plan([0, 0, 0], 0)
    assert slot.tolist() == [-1, -1] and live == 0


def test_groups_plan_refusals():
    import ctypes as C
    L = capi.lib()

    def raw(off, n_groups, n_rows):
        off = np.ascontiguousarray(off, np.int64)
        slot, live = np.full(max(n_groups, 1), -7, np.int32), C.c_int64(-7)
        rc = L.bbq_groups_plan(off.ctypes.data, n_groups, n_rows, None, slot.ctypes.data, C.byref(live))
        return rc, L.bbq_last_error().decode("utf-8"), (slot == -7).all() and live.value == -7

    assert raw([0, 4, 10], 2, 10)[0] == capi.OK
    for off, n_groups, n_rows, word in (([1, 4, 10], 2, 10, "[0]"),          # not starting at 0
                                        ([0, 6, 4, 10], 3, 10, "ascend"),    # descending
                                        ([0, 4, 9], 2, 10, "10"),            # not ending at n_rows
                                        ([0, 4, 11], 2, 10, "10"),
                                        ([0], -1, 0, "n_groups")):
        rc, msg, untouched = raw(off, n_groups, n_rows)
        assert rc == capi.ERR_INVALID_ARG and word in msg and "bbq_groups_plan" in msg and untouched, (off, msg)
    slot, live = np.zeros(2, np.int32), C.c_int64(0)
    assert L.bbq_groups_plan(None, 2, 10, None, slot.ctypes.data, C.byref(live)) == capi.ERR_INVALID_ARG
    assert L.bbq_groups_plan(np.array([0, 4, 10], np.int64).ctypes.data, 2, 10, None, slot.ctypes.data, None) == capi.ERR_INVALID_ARG
    with pytest.raises(capi.BBQError):
        capi.groups_plan([0, 5, 3, 10], 10)


def test_the_rule_over_representatives():
    """the status of a query is the span search's rule over its representatives' scores"""
    s = np.array([5, 1, 5, 2, np.nan, 3, 0.5], np.float32)
    off = np.array([0, 2, 4, 5, 7], np.int64)                      # representatives: 5 (row 0), 5 (row 2), NaN (row 4), 3 (row 5)
    everything = np.ones(7, bool)
    rep = s[representatives(s, off, everything)[0]]
    assert SC.expected_status(rep, 1) == 1                         # a NaN representative
    no_nan = np.array([1, 1, 1, 1, 0, 1, 1], bool)
    rep = s[representatives(s, off, no_nan)[0]]
    assert rep.tolist() == [5, 5, 3] and SC.expected_status(rep, 1) == 1 and SC.expected_status(rep, 2) == 1      # two equal among the k + 1 largest
    rep = s[representatives(s, off, np.array([1, 1, 0, 1, 0, 1, 1], bool))[0]]
    assert rep.tolist() == [5, 2, 3] and SC.expected_status(rep, 1) == 0 and SC.expected_status(rep, 2) == 0 and SC.expected_status(rep, 3) == 1
