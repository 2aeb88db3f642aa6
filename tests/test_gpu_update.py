"""GPU: rows of a device-resident index replaced in place (bbq_index_update_rows, bbq_index_update, bbq_vectors_update,
bbq_update_winners).  The contract: after an update the index is indistinguishable from one created whole over the same rows with the
rows at ords[i] replaced - size and capacity unchanged - and a filter made before it still serves.  The expected value is always the
ORACLE over the updated row set (tests/test_gpu_compact.py's RowSet.oracle_over: the replacement rows are other rows of the same set,
so the oracle's scores are re-indexed, or tests/append_recipe.py's per-row recipe for raw rows) plus a twin created whole, files
included.  Last-wins among duplicate ords is stated by a Python loop.  Bit-exact: indices, f32 score bits and order, ties included;
no tolerances."""
import numpy as np
import pytest

import orclib as O
from bbqlib import bbq_amd as B, capi
from append_recipe import oracle_rows
from test_gpu_append import Oracle, canon32, canon64, check_export, file_bytes, make_index
from test_gpu_compact import CASES, RESET, row_set

pytestmark = pytest.mark.gpu

VARIANTS = ({}, {"force_dense": 1}, {"sweep_share": 4}, {"sweep_share": 32}, {"device_select": 0})
EDGES = (63, 64, 65, 511, 512, 513)


def duplicates_of(n):
    """one ord named three times, interleaved with others"""
    d = n // 2
    return [0, d, n - 1, d, 1 % n, d]


def ords_of(n):
    """the shapes where the scatter can go wrong, for a set of n rows"""
    rng = np.random.default_rng(8000 + n)
    p = {"row_0": [0], "last_row": [n - 1], "tile_edges": [e for e in EDGES if e < n], "whole_tile_1": [o for o in range(64, 128) if o < n],
         "partial_last_tile": list(range((n - 1) // 64 * 64, n)), "every_row": list(range(n - 1, -1, -1)), "every_10th": list(range(3, n, 10)),
         "random_half_shuffled": list(rng.permutation(n)[:n // 2]), "duplicates": duplicates_of(n), "empty": []}
    return {k: np.array(v, np.int64) for k, v in p.items()}


PATTERNS = tuple(ords_of(1000))


def sources_of(ords, n):
    return np.array([(7 * int(o) + 3 + i) % n for i, o in enumerate(ords)], np.int64)


def apply_in_order(src, ords, frm):
    """the block applied entry by entry: the last of equal ords wins.  Returns the winners' positions, ascending by ord."""
    last = {}
    for i, o in enumerate(ords):
        src[int(o)] = frm[i]
        last[int(o)] = i
    return np.array([last[o] for o in sorted(last)], np.int64)


def needs_sums(codes, corr, ib):
    """does a creation over these rows store explicit component sums: is some quantizedComponentSum not the implied one?"""
    implied = np.unpackbits(codes, axis=1).sum(axis=1) if ib == 1 else codes.astype(np.int64).sum(axis=1)
    return bool((corr[:, 3] != implied).any())


def check_updated(rs, ix, twin, src, tmp_path, msg, variants=VARIANTS):
    """ix, holding the rows `src` of the set after its update, against the oracle over them and the twin created whole over them"""
    n = len(src)
    assert ix.n == n == capi.lib().bbq_index_size(ix._h)
    assert ix.capacity == twin.capacity == (n + 63) // 64 * 64
    # the record format is never re-decided: an index that stores explicit sums keeps storing them when no row needs them any more,
    # and only then do its files differ from those of the twin, whose own creation stores none
    same_format = not needs_sums(rs.codes, rs.corr, rs.ib) or needs_sums(rs.codes[src], rs.corr[src], rs.ib)
    if same_format:
        assert ix.bytes_per_row == twin.bytes_per_row
    else:
        assert ix.bytes_per_row > twin.bytes_per_row
    check_export(ix, rs.codes[src], rs.corr[src], msg)
    orc = rs.oracle_over(src)
    orc.check_score_rows(ix, msg)
    for opts in variants:
        for k_, v in opts.items():
            ix.set_option(k_, v)
        orc.check_search(ix, sorted({1, 10, 100, n, n + 5}), "%s %s" % (msg, opts), single=True)
        for k_ in opts:
            ix.set_option(k_, RESET[k_])
    if same_format:
        assert file_bytes(ix, str(tmp_path / "updated"), rs.cen, rs.sim) == file_bytes(twin, str(tmp_path / "twin"), rs.cen, rs.sim), msg
    return orc


# ------------------------------------------------------------------------------------------------ 1. every row set x every pattern

@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("compact", [True, False])
@pytest.mark.parametrize("name", CASES)
def test_update_rows_equals_created_whole(name, compact, pattern, tmp_path):
    rs = row_set(name)
    n = rs.n
    ords = ords_of(n)[pattern]
    frm = sources_of(ords, n)
    msg = "%s compact=%s %s" % (name, compact, pattern)
    src = np.arange(n)
    winners = apply_in_order(src, ords, frm)
    np.testing.assert_array_equal(capi.update_winners(ords, n), winners, err_msg=msg)
    if pattern == "duplicates":
        assert len({int(f) for o, f in zip(ords, frm) if o == n // 2}) == min(3, n), "the duplicate ord has no three sources: the case is void"
    ix = rs.index(compact)
    twin = rs.index(compact, src)
    try:
        before = (ix.capacity, file_bytes(ix, str(tmp_path / "before"), rs.cen, rs.sim))
        ix.update_rows(ords, rs.codes[frm], rs.corr[frm])
        if len(ords) == 0:
            assert (ix.capacity, file_bytes(ix, str(tmp_path / "after"), rs.cen, rs.sim)) == before
        check_updated(rs, ix, twin, src, tmp_path, msg)
    finally:
        ix.close()
        twin.close()


# ------------------------------------------------------------------------------------------------ 2. raw rows

@pytest.mark.parametrize("compact", [True, False])
@pytest.mark.parametrize("name", CASES)
def test_update_raw_equals_created_whole(name, compact, tmp_path):
    """seeded fp32 rows through bbq_index_update: the rows are the oracle recipe's against the build's centroid, and codes_out /
    corr_out carry all n rows of the block, duplicate losers included"""
    rs = row_set(name)
    n, dim = rs.n, rs.dim
    if name == "seeded_1000x129":
        lam, iters, queries = 0.1, 5, O.mulberry32(202, 2 * dim).reshape(2, dim)
    else:
        g = O.load_golden(name)
        lam, iters, queries = g["lambda"], g["iters"], O.golden_inputs(g)[1]
    ords = np.array([e for e in EDGES if e < n] + duplicates_of(n), np.int64)
    fresh = O.mulberry32(301 + dim, len(ords) * dim).reshape(len(ords), dim).copy()
    fresh[1] = -1.25
    wcodes, wcorr = oracle_rows(fresh, rs.cen, rs.sim, rs.ib, lam, iters)
    codes, corr = rs.codes.copy(), rs.corr.copy()
    for i, o in enumerate(ords):   # applied in order: the last of equal ords wins
        codes[o], corr[o] = wcodes[i], wcorr[i]
    msg = "%s compact=%s raw" % (name, compact)
    orc = Oracle(codes, corr, dim, rs.cen, rs.sim, rs.qb, queries, rs.ib, lam, iters)
    ix = rs.index(compact)
    twin = None
    try:
        got_codes, got_corr = ix.update(ords, fresh, rs.cen, rs.sim, lam, iters)
        np.testing.assert_array_equal(got_codes, wcodes, err_msg=msg)
        np.testing.assert_array_equal(canon64(got_corr), canon64(wcorr), err_msg=msg)
        # the twin is created whole from the rows as the device made them: they equal the recipe's up to the bits of a NaN - a 1-d
        # row has a zero-width interval - which a file keeps as they are (as in tests/test_gpu_append.py)
        tcodes, tcorr = rs.codes.copy(), rs.corr.copy()
        for i, o in enumerate(ords):
            tcodes[o], tcorr[o] = got_codes[i], got_corr[i]
        twin = make_index(tcodes, tcorr, dim, rs.cdp, compact, rs.ib)
        assert ix.n == n and ix.capacity == twin.capacity
        check_export(ix, codes, corr, msg)
        orc.check_score_rows(ix, msg)
        orc.check_search(ix, sorted({1, 10, 100, n, n + 5}), msg, single=True)
        if not needs_sums(rs.codes, rs.corr, rs.ib) or needs_sums(codes, corr, rs.ib):   # otherwise the twin's creation stores no sums
            assert file_bytes(ix, str(tmp_path / "updated"), rs.cen, rs.sim) == file_bytes(twin, str(tmp_path / "twin"), rs.cen, rs.sim), msg
        assert ix.update(ords, fresh, rs.cen, rs.sim, lam, iters, want_host_copy=False) == (None, None)   # the same rows again: nothing changes
        check_export(ix, codes, corr, msg + " twice")
        assert file_bytes(ix, str(tmp_path / "again"), rs.cen, rs.sim) == file_bytes(ix, str(tmp_path / "updated"), rs.cen, rs.sim), msg
    finally:
        ix.close()
        if twin is not None:
            twin.close()


# ------------------------------------------------------------------------------------------------ 3. a filter made before

@pytest.mark.parametrize("mask_name", ["random_50", "only_last_row"])
@pytest.mark.parametrize("compact", [True, False])
def test_filter_made_before_an_update_still_serves(compact, mask_name):
    rs = row_set("seeded_1000x129")
    n = rs.n
    r = np.arange(n)
    mask = {"random_50": np.random.default_rng(8100).random(n) < 0.5, "only_last_row": r == n - 1}[mask_name]
    acc, rej = np.flatnonzero(mask), np.flatnonzero(~mask)
    ords = np.concatenate([acc[:40], rej[:40], [n - 1, 0, 63, 64]])   # rows inside and outside the filter
    frm = sources_of(ords, n)
    src = np.arange(n)
    apply_in_order(src, ords, frm)
    orc = rs.oracle_over(src)
    ix = rs.index(compact)
    try:
        with capi.Filter(ix, mask) as flt:
            ix.update_rows(ords, rs.codes[frm], rs.corr[frm])
            assert flt.count == len(acc)
            for k in sorted({1, 10, len(acc) + 5}):
                idx, sc, cnt = ix.search_filtered_batch(orc.qq, orc.qc, rs.qb, rs.sim, k, flt)
                for qi in range(len(orc.qq)):
                    pos, ws = O.heap_topk(orc.scores[qi][2][acc], k)
                    np.testing.assert_array_equal(idx[qi, :cnt[qi]], acc[pos], err_msg="%s q%d k=%d" % (mask_name, qi, k))
                    np.testing.assert_array_equal(canon32(sc[qi, :cnt[qi]]), canon32(ws))
    finally:
        ix.close()


# ------------------------------------------------------------------------------------------------ 4. the three mutations in sequence

@pytest.mark.parametrize("compact", [True, False])
def test_update_then_append_then_compact(compact, tmp_path):
    rs = row_set("seeded_1000x129")
    n = rs.n
    ords = ords_of(n)["random_half_shuffled"]
    frm = sources_of(ords, n)
    src = np.arange(n)
    apply_in_order(src, ords, frm)
    ix = rs.index(compact)
    try:
        ix.update_rows(ords, rs.codes[frm], rs.corr[frm])
        new = np.resize(np.arange(n)[::-1], 70)
        ix.append_rows(rs.codes[new], rs.corr[new])
        src = np.concatenate([src, new])
        again = np.array([n + 69, n, 999, 1000, 1023, 1024], np.int64)   # an update of appended rows, across the old end
        frm2 = sources_of(again, n)
        ix.update_rows(again, rs.codes[frm2], rs.corr[frm2])
        apply_in_order(src, again, frm2)
        mask = np.random.default_rng(8200).random(len(src)) < 0.6
        with capi.Filter(ix, mask) as flt:
            ix.compact(flt)
        src = src[mask]
        twin = rs.index(compact, src)
        try:
            check_updated(rs, ix, twin, src, tmp_path, "update, append, update, compact", variants=({},))
        finally:
            twin.close()
    finally:
        ix.close()


# ------------------------------------------------------------------------------------------------ 5. explicit component sums

def test_explicit_sums(tmp_path):
    """an index created with a row whose quantizedComponentSum is not its popcount stores the sums, takes any row and keeps storing
    them - replace that very row too: answers and export are the twin's, whose own creation then stores none.  An index without
    explicit sums refuses such a row and is left byte for byte as it was."""
    sim, dim, n = 1, 96, 300
    base = O.mulberry32(311, n * dim).reshape(n, dim)
    queries = O.mulberry32(312, 2 * dim).reshape(2, dim)
    plain_codes, plain_corr, cen = O.build_index(base, sim)
    cdp = O.centroid_dp(cen)
    odd_corr = plain_corr.copy()
    odd_corr[70, 3] += 2.0
    ords = np.array([5, 200, 64], np.int64)
    new_codes, new_corr = plain_codes[[9, 10, 11]].copy(), plain_corr[[9, 10, 11]].copy()
    new_corr[1, 3] -= 3.0   # a row whose sum is not its popcount
    ix = B.Index(plain_codes, odd_corr, dim, cdp)
    try:
        bpr = ix.bytes_per_row
        codes, corr = plain_codes.copy(), odd_corr.copy()
        codes[ords], corr[ords] = new_codes, new_corr
        ix.update_rows(ords, new_codes, new_corr)
        twin = B.Index(codes, corr, dim, cdp)
        try:
            assert ix.bytes_per_row == twin.bytes_per_row == bpr
            check_export(ix, codes, corr, "explicit sums")
            orc = Oracle(codes, corr, dim, cen, sim, 4, queries)
            orc.check_search(ix, [1, 10, 100, n], "explicit sums", single=True)
            orc.check_score_rows(ix, "explicit sums")
            assert file_bytes(ix, str(tmp_path / "a"), cen, sim) == file_bytes(twin, str(tmp_path / "b"), cen, sim)
        finally:
            twin.close()
        # the rows that needed the sums replaced: the index keeps storing them, the twin's creation decides otherwise
        back = np.array([70, 200], np.int64)
        ix.update_rows(back, plain_codes[back], plain_corr[back])
        codes[back], corr[back] = plain_codes[back], plain_corr[back]
        twin = B.Index(codes, corr, dim, cdp)
        try:
            assert ix.bytes_per_row == bpr and twin.bytes_per_row < bpr
            check_export(ix, codes, corr, "explicit sums, replaced")
            orc = Oracle(codes, corr, dim, cen, sim, 4, queries)
            for h in (ix, twin):
                orc.check_search(h, [1, 10, 100, n], "explicit sums, replaced", single=True)
                orc.check_score_rows(h, "explicit sums, replaced")
        finally:
            twin.close()
    finally:
        ix.close()
    for compact in (True, False):
        ix = make_index(plain_codes, plain_corr, dim, cdp, compact)
        try:
            before = file_bytes(ix, str(tmp_path / "before"), cen, sim)
            with pytest.raises(B.BBQError) as e:
                ix.update_rows(ords, new_codes, new_corr)
            assert e.value.code == capi.ERR_UNSUPPORTED
            assert file_bytes(ix, str(tmp_path / "after"), cen, sim) == before
        finally:
            ix.close()


# ------------------------------------------------------------------------------------------------ 6. refusals

def test_refusals_leave_the_index_as_it_was(tmp_path):
    import torch
    rs = row_set("seeded_1000x129")
    L = capi.lib()
    n, dim = rs.n, rs.dim
    root = rs.index(True)
    multi = B.Index.create_multi(rs.codes, rs.corr, dim, rs.cdp, [0, 0], pilot_rows=512)
    shard = B.Index(rs.codes, rs.corr, dim, rs.cdp, row_base=1024)
    pilot = B.Index(rs.codes, rs.corr, dim, rs.cdp, row_base=1024, pilot_codes=rs.codes[:512], pilot_corr=rs.corr[:512])
    rs2, rs_e = row_set("ib2_100d_cos_qb4"), row_set("m_100d_euc_qb4")
    two_bit, euclid = rs2.index(True), rs_e.index(True)
    try:
        def snapshot(ix, r):
            return (ix.n, ix.capacity, file_bytes(ix, str(tmp_path / "snap"), r.cen, r.sim))

        before = snapshot(root, rs)
        fresh = O.mulberry32(321, 4 * dim).reshape(4, dim).copy()
        good = np.array([3, 64, 999, 3], np.int32)
        for bad_ord in (-1, n):
            ords = np.array([3, bad_ord, 5, 7], np.int64)
            for call in (lambda: root.update_rows(ords, rs.codes[:4], rs.corr[:4]), lambda: root.update(ords, fresh, rs.cen, rs.sim)):
                with pytest.raises(B.BBQError) as e:
                    call()
                assert e.value.code == capi.ERR_INVALID_ARG
            with pytest.raises(B.BBQError) as e:
                capi.update_winners(ords, n)
            assert e.value.code == capi.ERR_INVALID_ARG
            assert snapshot(root, rs) == before
        # NaN / Infinity at a known place, on a EUCLIDEAN set (COSINE normalises first: a NaN spreads over its row, an Infinity becomes one)
        before_e = snapshot(euclid, rs_e)
        fresh_e = O.mulberry32(322, 4 * rs_e.dim).reshape(4, rs_e.dim).copy()
        for value, code in ((np.nan, capi.ERR_NAN_INPUT), (np.inf, capi.ERR_INF_INPUT), (-np.inf, capi.ERR_INF_INPUT)):
            poisoned = fresh_e.copy()
            poisoned[2, 77] = value
            poisoned[3, 5] = value   # behind the first in row-major order
            with pytest.raises(B.BBQError) as e:
                euclid.update([3, 64, 256, 3], poisoned, rs_e.cen, rs_e.sim)   # the offender is a row that would win
            assert (e.value.code, e.value.bad_row, e.value.bad_col) == (code, 2, 77)
            poisoned = fresh_e.copy()
            poisoned[0, 9] = value
            with pytest.raises(B.BBQError) as e:
                euclid.update([3, 64, 256, 3], poisoned, rs_e.cen, rs_e.sim)   # ... and one that loses to a later duplicate
            assert (e.value.code, e.value.bad_row, e.value.bad_col) == (code, 0, 9)
            assert snapshot(euclid, rs_e) == before_e
        poisoned = fresh.copy()
        poisoned[1, 100] = np.nan
        with pytest.raises(B.BBQError) as e:   # COSINE: the row's norm is NaN, and with it its first value
            root.update(good, poisoned, rs.cen, rs.sim)
        assert (e.value.code, e.value.bad_row, e.value.bad_col) == (capi.ERR_NAN_INPUT, 1, 0)
        assert snapshot(root, rs) == before
        # a multi-bit code out of range, in a row that loses to a later duplicate: every row of the block is validated
        before2 = snapshot(two_bit, rs2)
        c2, r2 = rs2.codes[:3].copy(), rs2.corr[:3].copy()
        c2[0, 17] = 4
        r2[0, 3] = c2[0].sum()
        with pytest.raises(B.BBQError) as e:
            two_bit.update_rows([8, 70, 8], c2, r2)
        assert e.value.code == capi.ERR_INVALID_ARG
        assert snapshot(two_bit, rs2) == before2
        # a null pointer with n > 0
        o4 = np.ascontiguousarray(good)
        assert L.bbq_index_update_rows(root._h, o4.ctypes.data, None, rs.corr.ctypes.data, 4) == capi.ERR_INVALID_ARG
        assert L.bbq_index_update_rows(root._h, o4.ctypes.data, rs.codes.ctypes.data, None, 4) == capi.ERR_INVALID_ARG
        assert L.bbq_index_update_rows(root._h, None, rs.codes.ctypes.data, rs.corr.ctypes.data, 4) == capi.ERR_INVALID_ARG
        assert L.bbq_index_update_rows(None, o4.ctypes.data, rs.codes.ctypes.data, rs.corr.ctypes.data, 4) == capi.ERR_INVALID_ARG
        assert L.bbq_index_update(root._h, o4.ctypes.data, None, 4, rs.cen.ctypes.data, rs.sim, 0.1, 5, None, None, None, None) == capi.ERR_INVALID_ARG
        assert L.bbq_index_update(root._h, o4.ctypes.data, fresh.ctypes.data, 4, None, rs.sim, 0.1, 5, None, None, None, None) == capi.ERR_INVALID_ARG
        assert L.bbq_index_update_rows(root._h, o4.ctypes.data, rs.codes.ctypes.data, rs.corr.ctypes.data, -1) == capi.ERR_INVALID_ARG
        assert L.bbq_index_update_rows(root._h, None, None, None, 0) == capi.OK
        assert snapshot(root, rs) == before
        # out of scope: a multi-device handle, a shard with row_base > 0, an index with a pilot replica
        for ix in (multi, shard, pilot):
            assert L.bbq_index_update_rows(ix._h, o4.ctypes.data, rs.codes.ctypes.data, rs.corr.ctypes.data, 4) == capi.ERR_UNSUPPORTED
            assert L.bbq_index_update(ix._h, o4.ctypes.data, fresh.ctypes.data, 4, rs.cen.ctypes.data, rs.sim, 0.1, 5, None, None, None, None) == capi.ERR_UNSUPPORTED
        check_export(shard, rs.codes, rs.corr, "refused shard")
        # a bbq_shard_scan_begin batch that has not been waited for
        k, nq = 10, len(rs.orc.qq)
        cap = int(root.shard_list_cap(k)) * nq
        d_packed = torch.zeros(cap, dtype=torch.int64, device="cuda")
        d_off = torch.zeros(nq + 1, dtype=torch.int64, device="cuda")
        d_flags = torch.zeros(nq, dtype=torch.int32, device="cuda")
        root.shard_scan_begin(rs.orc.qq, rs.orc.qc, rs.qb, rs.sim, k, d_packed.data_ptr(), cap, d_off.data_ptr(), d_flags.data_ptr())
        assert L.bbq_index_update_rows(root._h, o4.ctypes.data, rs.codes.ctypes.data, rs.corr.ctypes.data, 4) == capi.ERR_INVALID_ARG
        assert L.bbq_index_update(root._h, o4.ctypes.data, fresh.ctypes.data, 4, rs.cen.ctypes.data, rs.sim, 0.1, 5, None, None, None, None) == capi.ERR_INVALID_ARG
        root.shard_scan_wait()
        assert snapshot(root, rs) == before
        # ... and waited for, the root index takes the update; a sharded scan of it afterwards equals the oracle
        frm = sources_of(good, n)
        src = np.arange(n)
        apply_in_order(src, good, frm)
        root.update_rows(good, rs.codes[frm], rs.corr[frm])
        orc = rs.oracle_over(src)
        total = root.shard_scan(orc.qq, orc.qc, rs.qb, rs.sim, k, d_packed.data_ptr(), cap, d_off.data_ptr(), d_flags.data_ptr())
        assert int(d_flags.abs().sum().item()) == 0
        idx, sc, cnt = B.replay_batch([d_packed[:total].cpu().numpy().view(np.uint64)], [d_off.cpu().numpy()], nq, n, k)
        for qi in range(nq):
            wi, ws = orc.topk(qi, k)
            np.testing.assert_array_equal(idx[qi, :cnt[qi]], wi)
            np.testing.assert_array_equal(canon32(sc[qi, :cnt[qi]]), canon32(ws))
    finally:
        for h in (root, multi, shard, pilot, two_bit, euclid):
            h.close()


# ------------------------------------------------------------------------------------------------ 7. the fp32 side of the rerank recipe

@pytest.mark.parametrize("selector,how", [(0, "heap"), (1, "sort")])
@pytest.mark.parametrize("dim", [96, 129])
def test_vectors_update_and_rerank(dim, selector, how):
    sim, n, k, factor = 1, 1000, 10, 5
    base = O.mulberry32(331 + dim, n * dim).reshape(n, dim)
    queries = O.mulberry32(332, 3 * dim).reshape(3, dim)
    codes, corr, cen = O.build_index(base, sim)
    cdp = O.centroid_dp(cen)
    ords = np.array([0, 63, 64, 999, 500, 64, 7, 500, 500], np.int64)   # with duplicates
    fresh = O.mulberry32(333 + dim, len(ords) * dim).reshape(len(ords), dim)
    wcodes, wcorr = oracle_rows(fresh, cen, sim, 1)
    base2, codes2, corr2 = base.copy(), codes.copy(), corr.copy()
    for i, o in enumerate(ords):
        base2[o], codes2[o], corr2[o] = fresh[i], wcodes[i], wcorr[i]
    orc = Oracle(codes2, corr2, dim, cen, sim, 4, queries)
    ix, dv = make_index(codes, corr, dim, cdp, True), B.Vectors(base)
    whole_ix, whole_dv = make_index(codes2, corr2, dim, cdp, True), B.Vectors(base2)
    try:
        ix.update(ords, fresh, cen, sim)
        dv.update(ords, fresh)
        assert dv.n == n == capi.lib().bbq_vectors_size(dv._h)
        for bad in (-1, n):
            with pytest.raises(B.BBQError) as e:
                dv.update([3, bad], fresh[:2])
            assert e.value.code == capi.ERR_INVALID_ARG
        dv.update([], fresh[:0])
        rows = [np.arange(n, dtype=np.int32)] * 3
        for x, y in zip(dv.rerank_scores(queries, rows, 1), whole_dv.rerank_scores(queries, rows, 1)):
            np.testing.assert_array_equal(canon64(x), canon64(y))
        got = B.search_rerank_batch(ix, dv, queries, orc.qq, orc.qc, 4, sim, k, factor, selector, 1)
        want = B.search_rerank_batch(whole_ix, whole_dv, queries, orc.qq, orc.qc, 4, sim, k, factor, selector, 1)
        for qi in range(3):
            cand, csc = orc.topk(qi, k * factor)
            true = O.true_similarity(queries[qi:qi + 1], base2[cand], 1)[0]
            pos = O.rerank_select(true, k, how)
            np.testing.assert_array_equal(got[0][qi, :got[3][qi]], cand[pos])
            np.testing.assert_array_equal(canon32(got[1][qi, :got[3][qi]]), canon32(csc[pos]))
            np.testing.assert_array_equal(canon64(got[2][qi, :got[3][qi]]), canon64(true[pos]))
        for a, b in zip(got, want):
            np.testing.assert_array_equal(np.asarray(a).view(np.uint8), np.asarray(b).view(np.uint8))
    finally:
        for h in (ix, dv, whole_ix, whole_dv):
            h.close()


# ------------------------------------------------------------------------------------------------ the Python mirror

def test_api_update_vectors_on_the_device():
    sim, dim, n = 1, 100, 400
    a = O.mulberry32(341, n * dim).reshape(n, dim)
    q = O.mulberry32(343, dim)
    fmt = B.BinaryQuantizationFormat({"queryBits": 4, "indexBits": 1, "quantizer": {"similarityFunction": "COSINE", "lambda": 0.1, "iters": 5}})
    tv = fmt.quantizeVectors(list(a))["quantizedVectors"]
    codes, corr, cen = O.build_index(a, sim)
    ords = [399, 7, 64, 7]
    fresh = O.mulberry32(342, 4 * dim).reshape(4, dim)
    wcodes, wcorr = oracle_rows(fresh, cen, sim, 1)
    for i, o in enumerate(ords):
        codes[o], corr[o] = wcodes[i], wcorr[i]
    old_row = tv.vectorValue(7)
    old_copy = old_row.copy()
    assert fmt.updateVectors(tv, ords, list(fresh)) is tv and tv.size() == n == tv._device().n
    np.testing.assert_array_equal(old_row, old_copy)   # rows handed out earlier stay valid
    for ord_ in (0, 7, 64, 399):
        np.testing.assert_array_equal(tv.vectorValue(ord_), codes[ord_])
        t = tv.getCorrectiveTerms(ord_)
        got = np.array([t["lowerInterval"], t["upperInterval"], t["additionalCorrection"], t["quantizedComponentSum"]])
        np.testing.assert_array_equal(canon64(got), canon64(corr[ord_]))
    wi, ws = O.search(q, codes, corr, cen, sim, 4, 25)
    got = fmt.searchNearestNeighbors(q, tv, 25)
    assert [r["index"] for r in got] == list(wi)
    np.testing.assert_array_equal(canon32([r["score"] for r in got]), canon32(ws))
    with pytest.raises(Exception, match="向量索引 %d 不存在" % n):
        fmt.updateVectors(tv, [n], list(fresh[:1]))
    assert fmt.updateVectors(tv, [], []) is tv and tv.size() == n
