"""CPU: filtered search without a device.  (1) The argument checks of bbq_filter_* / bbq_search_filtered_batch that come before
anything touches the device.  (2) The exactness argument of the accepted-space plan (DESIGN.md "Filtered search"; build_filtered_plan,
bbq_core.cpp) restated in numpy: segments cut by ACCEPTED rows seen, thresholds = order statistics of rank min(k, |A|) over the
accepted rows of the earlier segments, candidates = accepted rows strictly above them, the host-only bbq_replay over the candidate
lists - compared with the oracle's heap over the accepted rows in ascending ord.  The restated plan is held, segment by segment, to
the library's own (bbq_filter_plan, host only)."""
import ctypes as C

import numpy as np
import pytest

import orclib as O
from bbqlib import capi

CHUNK = 512


# ------------------------------------------------------------------------------------------------ argument checks

def _err():
    return capi.lib().bbq_last_error().decode("utf-8")


def test_filter_create_argument_checks_come_before_the_device():
    L = capi.lib()
    out = C.c_void_p(1)
    words = np.zeros(4, np.uint64)
    # null index
    assert L.bbq_filter_create(None, words.ctypes.data, 4, C.byref(out)) == capi.ERR_INVALID_ARG
    assert "目标向量集合不能为空" in _err() and out.value is None
    # null bits
    assert L.bbq_filter_create(None, None, 4, C.byref(out)) == capi.ERR_INVALID_ARG
    assert "accept_bits is null" in _err()
    # wrong n_words (the comparison with the index's size needs an index: tests/test_gpu_filtered.py)
    assert L.bbq_filter_create(None, words.ctypes.data, -1, C.byref(out)) == capi.ERR_INVALID_ARG
    assert "n_words" in _err()
    assert L.bbq_filter_create(None, words.ctypes.data, 4, None) == capi.ERR_INVALID_ARG
    assert "out is null" in _err()
    rows = np.zeros(3, np.int32)
    assert L.bbq_filter_create_rows(None, rows.ctypes.data, 3, C.byref(out)) == capi.ERR_INVALID_ARG
    assert "目标向量集合不能为空" in _err()
    assert L.bbq_filter_create_rows(None, None, 3, C.byref(out)) == capi.ERR_INVALID_ARG
    assert "rows is null" in _err()
    assert L.bbq_filter_count(None) == 0
    L.bbq_filter_destroy(None)  # like free(NULL)


def test_filtered_search_refuses_a_null_filter():
    L = capi.lib()
    qq = np.zeros(8, np.uint8)
    qc = np.zeros(4, np.float64)
    idx = np.zeros(5, np.int32)
    sc = np.zeros(5, np.float32)
    cnt = np.zeros(1, np.int64)
    rc = L.bbq_search_filtered_batch(None, None, 1, qq.ctypes.data, qc.ctypes.data, 4, 1, 5, idx.ctypes.data, sc.ctypes.data, cnt.ctypes.data)
    assert rc == capi.ERR_INVALID_ARG and "filter is null" in _err()


def test_pack_mask_is_the_documented_word_layout():
    rng = np.random.default_rng(1)
    for n in (1, 63, 64, 65, 1000):
        m = rng.random(n) < 0.4
        w = capi.pack_mask(m)
        assert w.dtype == np.dtype("<u8") and w.shape[0] == (n + 63) // 64
        for r in range(n):
            assert bool((int(w[r >> 6]) >> (r & 63)) & 1) == bool(m[r])


# ------------------------------------------------------------------------------------------------ the plan and its exactness

def key_of(s32):
    """bbq_entry.h key_of_bits: unsigned order of the keys = float order of the scores"""
    b = np.ascontiguousarray(s32, np.float32).view(np.uint32)
    return np.where(b & np.uint32(0x80000000), ~b, b | np.uint32(0x80000000)).astype(np.uint32)


def cap_for(k, before):
    lam = k * CHUNK / max(before, 1)
    c = int(np.ceil(lam + 8.0 * np.sqrt(lam) + 16.0))
    return min(max((c + 7) // 8 * 8, 16), CHUNK)


def filtered_plan(mask, k_dev, s0_opt=4096, growth=8):
    """build_filtered_plan: [(chunk_begin, chunk_end, cap)] from the cumulative accepted counts per chunk"""
    n = mask.shape[0]
    n_chunks = (n + CHUNK - 1) // CHUNK
    per = np.add.reduceat(mask.astype(np.int64), np.arange(0, n, CHUNK)) if n else np.zeros(0, np.int64)
    cum = np.concatenate([[0], np.cumsum(per)])
    A = int(cum[-1])
    if A == 0:
        return [], cum
    nz = np.flatnonzero(per)
    first, end = int(nz[0]), int(nz[-1]) + 1
    s0 = min(max(s0_opt, (4 * k_dev + CHUNK - 1) // CHUNK * CHUNK), 8192)
    where = lambda acc: int(np.searchsorted(cum, acc, side="left"))  # noqa: E731
    segs = []

    def add(b, e, bound):
        most = int(per[b:e].max())
        segs.append((b, e, min(bound, max(16, (most + 7) // 8 * 8))))

    b = first
    e = min(max(where(s0), b + 1), end)
    add(b, e, CHUNK)
    b = e
    while b < end:
        before = int(cum[b])
        nb = where(before * growth)
        e = nb if (nb > b and nb < end and cum[nb] <= A // 2) else end
        add(b, e, cap_for(k_dev, before))
        b = e
    assert n_chunks >= end
    # the restatement is held to the library's own plan (bbq_filter_plan runs build_filtered_plan): a drift on either side shows here
    assert [(b, e - b, cap) for b, e, cap in segs] == capi.filter_plan(mask, k_dev, s0_opt, growth)
    return segs, cum


def test_filter_plan_of_nothing_and_its_argument_checks():
    assert capi.filter_plan(np.zeros(5000, bool), 11) == []
    assert capi.filter_plan(np.zeros(0, bool), 11) == []
    one = np.zeros(5000, bool)
    one[4999] = True
    assert capi.filter_plan(one, 2) == [(9, 1, 16)]
    for bad in ({"k_dev": 0}, {"first_segment_rows": 512}, {"growth": 1}):
        with pytest.raises(capi.BBQError) as e:
            capi.filter_plan(one, **dict({"k_dev": 11}, **bad))
        assert e.value.code == capi.ERR_INVALID_ARG


def simulate(s32, mask, k, device_select, **plan_opts):
    """what the device lists for one query, segment by segment, and the replayed answer; also returns the largest number of
    candidates a chunk produced relative to its segment's cap (> 1 would be an overflow: flood tier / dense path, never a wrong answer)"""
    A = int(mask.sum())
    keff = min(k, A)
    k_dev = keff + 1 if device_select else keff
    segs, cum = filtered_plan(mask, k_dev, **plan_opts)
    keys = key_of(s32)
    seen = np.zeros(0, np.uint32)
    lists, fill = [], 0.0
    for (b, e, cap) in segs:
        theta = np.uint32(0) if seen.shape[0] < k_dev else np.sort(seen)[-k_dev]
        rows = np.arange(b * CHUNK, min(e * CHUNK, s32.shape[0]))
        rows = rows[mask[rows]]
        # the finalize kernel takes the threshold from the LISTED keys of the earlier segments + the running top keys: the k_dev
        # largest of those are the k_dev largest of every accepted row seen, because a row at or below a threshold is not among them
        seen = np.concatenate([seen, keys[rows]])
        cand = rows[(keys[rows] > theta) & ~np.isnan(s32[rows])]
        if cand.size:
            per_chunk = np.bincount(cand // CHUNK - b)
            fill = max(fill, per_chunk.max() / cap)
        lists.append((cand.astype(np.uint64) << np.uint64(32)) | np.ascontiguousarray(s32[cand], np.float32).view(np.uint32).astype(np.uint64))
    got = capi.replay(lists, A, k) if lists else (np.zeros(0, np.int32), np.zeros(0, np.float32))
    return got, segs, fill


def oracle(s32, mask, k):
    acc = np.flatnonzero(mask)
    pos, sc = O.heap_topk(s32[acc], k)
    return acc[pos].astype(np.int32), sc


def _scores(n, seed, ties):
    rng = np.random.default_rng(seed)
    s = (0.5 + 0.1 * rng.standard_normal(n)).astype(np.float32)
    if ties:  # planted equal scores, among them the very best values
        top = np.sort(s)[::-1]
        for v, cnt in ((top[0], 7), (top[15], 30), (top[99], 40), (top[100], 3), (np.float32(0.5), 500)):
            s[rng.choice(n, cnt, replace=False)] = v
        s[rng.choice(n, 50, replace=False)] = np.float32(-0.0)
        s[rng.choice(n, 50, replace=False)] = np.float32(0.0)
    return s


def _masks(n, seed):
    rng = np.random.default_rng(seed)
    idx = np.arange(n)
    m = {"ones": np.ones(n, bool), "random_50": rng.random(n) < 0.5, "random_1": rng.random(n) < 0.01,
         "last_10pct": idx >= n - n // 10, "first_half": idx < n // 2, "every_64th": idx % 64 == 0,
         "two_clusters": ((idx > n // 5) & (idx < n // 5 + 3000)) | (idx > n - 9000)}
    m["rows_1000"] = np.zeros(n, bool)
    m["rows_1000"][rng.choice(n, 1000, replace=False)] = True
    m["one_row"] = np.zeros(n, bool)
    m["one_row"][n - 1] = True
    return m


@pytest.mark.parametrize("ties", [False, True])
@pytest.mark.parametrize("device_select", [False, True])
def test_accepted_space_plan_is_exact(ties, device_select):
    n = 300_000
    s32 = _scores(n, 3, ties)
    for mname, mask in _masks(n, 4).items():
        A = int(mask.sum())
        for k in (1, 10, 100, 1000, A, A + 5):
            if min(k, A) > 4096:
                continue  # the dense path serves those
            for opts in ({}, {"s0_opt": 1024, "growth": 2}):
                got, segs, _ = simulate(s32, mask, k, device_select, **opts)
                want = oracle(s32, mask, k)
                np.testing.assert_array_equal(got[0], want[0], err_msg="%s k=%d %r" % (mname, k, opts))
                np.testing.assert_array_equal(got[1].view(np.uint32), want[1].view(np.uint32))


def test_rejected_rows_never_reach_a_threshold():
    """rejected rows hold strictly higher scores than every accepted row: thresholds over A only must still list the accepted answer"""
    n, k = 100_000, 50
    s32 = _scores(n, 8, True)
    mask = np.random.default_rng(9).random(n) < 0.3
    s32[~mask] += np.float32(10.0)
    got, _, _ = simulate(s32, mask, k, True)
    want = oracle(s32, mask, k)
    np.testing.assert_array_equal(got[0], want[0])
    assert mask[got[0]].all()


def test_clustered_filter_gets_segments_in_accepted_space():
    """the accepted rows are the last 10 %: a plan cut by rows swept would meet them all in its last segment; cut by accepted rows
    they get a first segment of s0 accepted rows and boundaries that grow by `growth`, and nothing before the first accepted row"""
    n, k = 2_000_000, 101
    mask = np.arange(n) >= n - n // 10
    segs, cum = filtered_plan(mask, k)
    assert segs[0][0] == (n - n // 10) // CHUNK, "the sweep starts at the first chunk with an accepted row"
    assert segs[-1][1] == (n + CHUNK - 1) // CHUNK
    seen = [int(cum[e]) for _, e, _ in segs]
    assert 4096 <= seen[0] < 4096 + CHUNK
    assert len(segs) >= 3 and all(seen[i] >= 8 * seen[i - 1] for i in range(1, len(segs) - 1))
    # a random 1 % filter: the first segment spans ~100 x more rows than accepted ones, and no chunk needs more slots than it accepts
    mask = np.random.default_rng(2).random(n) < 0.01
    segs, cum = filtered_plan(mask, k)
    assert 4096 <= cum[segs[0][1]] < 4096 + CHUNK and (segs[0][1] - segs[0][0]) * CHUNK > 300_000
    assert all(cap <= 32 for _, _, cap in segs)
    # expected candidates stay within the caps: the busiest chunk of a random-score run fills a fraction of its slots
    s32 = _scores(n, 5, False)
    _, _, fill = simulate(s32, mask, 100, True)
    assert fill <= 1.0
