"""GPU: an index compacted to a filter's accepted rows on the device (bbq_index_compact, bbq_index_remove_rows, bbq_vectors_compact).
The contract: after a compaction the index is indistinguishable from one created whole over the kept rows.  The expected value is
always the ORACLE over rows[mask] - orc_score_all + the reference heap, as tests/test_gpu_append.py builds it (a row's score does not
depend on the other rows, so the oracle scores every query once over all rows and the heaps run over the kept ones) - and a twin
index created whole over those rows is compared as well, files included.  Bit-exact: indices, f32 score bits and order, ties
included; no tolerances."""
import functools

import numpy as np
import pytest

import orclib as O
from bbqlib import bbq_amd as B, capi
from test_gpu_append import Oracle, canon32, canon64, check_export, file_bytes, make_index

pytestmark = pytest.mark.gpu

# one golden case each of ties_*, m_768d_* (w16 = 6), m_100d_*, ib2_*, ib4_*, ib8_*, edge_dim1 - all of them cases test_gpu_append.py
# uses - and a seeded 1000 x 129-d 1-bit set: w16 = 2 with a padded chunk, 15 full tiles + a partial tile of 40 rows, two chunks
CASES = ("ties_cos_qb4", "m_768d_cos_qb4", "m_100d_euc_qb4", "ib2_100d_cos_qb4", "ib4_96d_euc_qb4", "ib8_64d_cos_qb4", "edge_dim1", "seeded_1000x129")
RESET = {"force_dense": 0, "sweep_share": 1, "device_select": 1}


class RowSet:
    """one row set: the fp32 rows, the oracle's rows quantized from them and, per query, its scores of all of them"""

    def __init__(self, name):
        if name == "seeded_1000x129":
            self.sim, self.n, self.dim, self.ib, self.qb = 1, 1000, 129, 1, 4
            base = O.mulberry32(201, self.n * self.dim).reshape(self.n, self.dim)
            queries = O.mulberry32(202, 2 * self.dim).reshape(2, self.dim)
            lam, iters = 0.1, 5
        else:
            g = O.load_golden(name)
            self.sim, self.n, self.dim, self.ib, self.qb = O.SIMS[g["sim"]], g["n"], g["dim"], g["ib"], g["qb"]
            base, queries = O.golden_inputs(g)
            lam, iters = g["lambda"], g["iters"]
        self.base, self.queries, self.lam, self.iters = base, queries, lam, iters
        self.codes, self.corr, self.cen = O.build_index(base, self.sim, lam, iters, ib=self.ib)
        self.cdp = O.centroid_dp(self.cen)
        self.orc = Oracle(self.codes, self.corr, self.dim, self.cen, self.sim, self.qb, queries, self.ib, lam, iters)

    def index(self, compact, rows=None):
        sel = slice(None) if rows is None else rows
        return make_index(self.codes[sel], self.corr[sel], self.dim, self.cdp, compact, self.ib)

    def oracle_over(self, rows):
        """the expected answers of the index over these rows of the set, in this order"""
        o = object.__new__(Oracle)
        o.sim, o.qb, o.n, o.qq, o.qc, o._heaps = self.sim, self.qb, len(rows), self.orc.qq, self.orc.qc, {}
        o.scores = [tuple(a[rows] for a in s) for s in self.orc.scores]
        return o


@functools.lru_cache(maxsize=None)
def row_set(name):
    return RowSet(name)


def masks_of(n):
    """the shapes where the gather can go wrong, for a set of n rows"""
    r = np.arange(n)
    full, rng = n // 64, np.random.default_rng(7000 + n)
    m = {"keep_all": np.ones(n, bool), "keep_none": np.zeros(n, bool), "only_row_0": r == 0, "only_last_row": r == n - 1,
         "partial_last_tile": r >= (n - 1) // 64 * 64}
    for cnt in (63, 64, 65):   # the destination tile boundary: that many rows, spread over the whole set
        m["exactly_%d" % cnt] = np.isin(r, np.round(np.linspace(0, n - 1, min(cnt, n))).astype(np.int64))
    m["tiles_0_3_last_full_rejected"] = ~np.isin(r // 64, [0, 3, full - 1])   # source words of 0
    m["alternating"] = r % 2 == 1
    m["every_10th"] = r % 10 == 3             # one destination tile draws on ten source tiles
    m["middle_block"] = (r >= n // 3) & (r < 2 * n // 3)
    m["random_90"] = rng.random(n) < 0.9
    m["random_50"] = rng.random(n) < 0.5
    return m


MASK_NAMES = tuple(masks_of(1000))


def check_compacted(rs, ix, twin, kept, compact, tmp_path, msg, single=True):
    """ix, compacted to the rows `kept` of the set, against the oracle over them and the twin created whole over them"""
    m = len(kept)
    assert ix.n == m and capi.lib().bbq_index_size(ix._h) == m
    assert ix.capacity == twin.capacity == (m + 63) // 64 * 64
    assert ix.bytes_per_row == twin.bytes_per_row
    check_export(ix, rs.codes[kept], rs.corr[kept], msg)
    assert file_bytes(ix, str(tmp_path / "compacted"), rs.cen, rs.sim) == file_bytes(twin, str(tmp_path / "twin"), rs.cen, rs.sim), msg
    orc = rs.oracle_over(kept)
    if m == 0:
        idx, sc, cnt = ix.search_batch(orc.qq, orc.qc, rs.qb, rs.sim, 5)
        assert (cnt == 0).all()
        return orc
    orc.check_search(ix, sorted({1, 10, 100, m, m + 5}), msg, single=single)
    orc.check_score_rows(ix, msg)
    return orc


# ------------------------------------------------------------------------------------------------ 1. every row set x every mask

@pytest.mark.parametrize("mask_name", MASK_NAMES)
@pytest.mark.parametrize("compact", [True, False])
@pytest.mark.parametrize("name", CASES)
def test_compact_equals_created_whole(name, compact, mask_name, tmp_path):
    rs = row_set(name)
    mask = masks_of(rs.n)[mask_name]
    kept = np.flatnonzero(mask)
    m = len(kept)
    msg = "%s compact=%s %s" % (name, compact, mask_name)
    np.testing.assert_array_equal(capi.kept_rows(mask), kept)
    ix, twin = rs.index(compact), rs.index(compact, kept)
    try:
        before = (ix.capacity, file_bytes(ix, str(tmp_path / "before"), rs.cen, rs.sim))
        with capi.Filter(ix, mask) as flt:
            assert flt.count == m
            ix.compact(flt)
            if m == rs.n:   # the no-op: nothing changes, capacity and files included
                assert (ix.capacity, file_bytes(ix, str(tmp_path / "after"), rs.cen, rs.sim)) == before
            else:           # the filter used no longer fits the new size
                with pytest.raises(B.BBQError) as e:
                    ix.search_filtered_batch(rs.orc.qq, rs.orc.qc, rs.qb, rs.sim, 3, flt)
                assert e.value.code == capi.ERR_INVALID_ARG
        orc = check_compacted(rs, ix, twin, kept, compact, tmp_path, msg)
        # a filter made afterwards: the oracle over the doubly restricted rows
        if m > 0:
            again = np.random.default_rng(11).random(m) < 0.6
            acc = np.flatnonzero(again)
            with capi.Filter(ix, again) as flt2:
                assert flt2.count == len(acc)
                for k in sorted({1, 10, len(acc) + 5}):
                    idx, sc, cnt = ix.search_filtered_batch(orc.qq, orc.qc, rs.qb, rs.sim, k, flt2)
                    for qi in range(len(orc.qq)):
                        pos, ws = O.heap_topk(orc.scores[qi][2][acc], k)
                        np.testing.assert_array_equal(idx[qi, :cnt[qi]], acc[pos], err_msg="%s refiltered q%d k=%d" % (msg, qi, k))
                        np.testing.assert_array_equal(canon32(sc[qi, :cnt[qi]]), canon32(ws))
        # a later append behaves as on the twin: 70 more rows, files included
        new = np.resize(np.arange(rs.n), 70)
        rows = np.concatenate([kept, new])
        ix.append_rows(rs.codes[new], rs.corr[new])
        twin.append_rows(rs.codes[new], rs.corr[new])
        whole = rs.index(compact, rows)
        try:
            assert ix.n == m + 70 and ix.capacity == twin.capacity
            check_export(ix, rs.codes[rows], rs.corr[rows], msg + " + 70")
            files = file_bytes(ix, str(tmp_path / "grown"), rs.cen, rs.sim)
            assert files == file_bytes(twin, str(tmp_path / "twin_grown"), rs.cen, rs.sim), msg
            assert files == file_bytes(whole, str(tmp_path / "whole"), rs.cen, rs.sim), msg
            rs.oracle_over(rows).check_search(ix, sorted({1, 10, m + 70}), msg + " + 70", single=True)
        finally:
            whole.close()
    finally:
        ix.close()
        twin.close()


# ------------------------------------------------------------------------------------------------ 2. the other search paths

@pytest.mark.parametrize("compact", [True, False])
def test_search_variants_after_a_compaction(compact):
    rs = row_set("ties_cos_qb4")
    mask = masks_of(rs.n)["random_50"]
    kept = np.flatnonzero(mask)
    orc = rs.oracle_over(kept)
    ix = rs.index(compact)
    try:
        with capi.Filter(ix, mask) as flt:
            ix.compact(flt)
        for opts in ({"force_dense": 1}, {"sweep_share": 4}, {"sweep_share": 32}, {"device_select": 0}):
            for k_, v in opts.items():
                ix.set_option(k_, v)
            orc.check_search(ix, sorted({1, 10, 100, len(kept), len(kept) + 5}), "variant %s" % opts, single=True)
            for k_ in opts:
                ix.set_option(k_, RESET[k_])
    finally:
        ix.close()


# ------------------------------------------------------------------------------------------------ 3. explicit component sums

def test_explicit_sums_are_kept(tmp_path):
    """an index created from rows of which two carry a quantizedComponentSum that is not their popcount stores the sums, and a
    compaction never re-decides that: with one of the two kept the files are the twin's; with both removed the twin stores no sums -
    answers and export still match, and the index still stores them (bytes_per_row unchanged)"""
    sim, dim, n = 1, 96, 300
    base = O.mulberry32(211, n * dim).reshape(n, dim)
    queries = O.mulberry32(212, 2 * dim).reshape(2, dim)
    codes, corr, cen = O.build_index(base, sim)
    corr[[70, 200], 3] += 2.0
    cdp = O.centroid_dp(cen)
    orc = Oracle(codes, corr, dim, cen, sim, 4, queries)
    rng = np.random.default_rng(213)
    for keep_one in (True, False):
        mask = rng.random(n) < 0.7
        mask[70], mask[200] = keep_one, False
        kept = np.flatnonzero(mask)
        ix = B.Index(codes, corr, dim, cdp)
        twin = B.Index(codes[kept], corr[kept], dim, cdp)
        try:
            bpr = ix.bytes_per_row
            with capi.Filter(ix, mask) as flt:
                ix.compact(flt)
            assert ix.n == len(kept) and ix.bytes_per_row == bpr
            check_export(ix, codes[kept], corr[kept], "explicit sums")
            o = object.__new__(Oracle)
            o.sim, o.qb, o.n, o.qq, o.qc, o._heaps = sim, 4, len(kept), orc.qq, orc.qc, {}
            o.scores = [tuple(a[kept] for a in s) for s in orc.scores]
            for h in (ix, twin):
                o.check_search(h, [1, 10, 100, len(kept)], "explicit sums keep_one=%s" % keep_one, single=True)
                o.check_score_rows(h, "explicit sums")
            if keep_one:
                assert twin.bytes_per_row == bpr
                assert file_bytes(ix, str(tmp_path / "a"), cen, sim) == file_bytes(twin, str(tmp_path / "b"), cen, sim)
            else:
                assert twin.bytes_per_row < bpr   # the twin's own creation decides has_x1 = 0
        finally:
            ix.close()
            twin.close()


# ------------------------------------------------------------------------------------------------ 4. remove_rows

@pytest.mark.parametrize("compact", [True, False])
def test_remove_rows_equals_the_mask_form(compact, tmp_path):
    rs = row_set("seeded_1000x129")
    drop = np.array([999, 5, 64, 5, 63, 700, 128, 999, 0, 511, 512, 64], np.int32)   # unordered, with duplicates
    mask = np.ones(rs.n, bool)
    mask[drop] = False
    kept = np.flatnonzero(mask)
    a, b, twin = rs.index(compact), rs.index(compact), rs.index(compact, kept)
    try:
        a.remove_rows(drop)
        with capi.Filter(b, mask) as flt:
            b.compact(flt)
        assert file_bytes(a, str(tmp_path / "a"), rs.cen, rs.sim) == file_bytes(b, str(tmp_path / "b"), rs.cen, rs.sim)
        check_compacted(rs, a, twin, kept, compact, tmp_path, "remove_rows")
        # a row outside the index: BBQ_ERR_INVALID_ARG, and the index is unchanged - same export, same files
        before = (a.n, a.capacity, file_bytes(a, str(tmp_path / "snap"), rs.cen, rs.sim))
        for bad in ([3, len(kept)], [-1], [7, 2**31 - 1]):
            with pytest.raises(B.BBQError) as e:
                a.remove_rows(bad)
            assert e.value.code == capi.ERR_INVALID_ARG
            assert (a.n, a.capacity, file_bytes(a, str(tmp_path / "snap"), rs.cen, rs.sim)) == before
            check_export(a, rs.codes[kept], rs.corr[kept], "refused remove_rows")
        a.remove_rows([])   # nothing named: nothing changes
        assert (a.n, a.capacity, file_bytes(a, str(tmp_path / "snap"), rs.cen, rs.sim)) == before
    finally:
        for h in (a, b, twin):
            h.close()


# ------------------------------------------------------------------------------------------------ 5. refusals leave the index unchanged

def test_refusals_leave_the_index_unchanged(tmp_path):
    import torch
    rs = row_set("seeded_1000x129")
    L = capi.lib()
    n = rs.n
    root, other = rs.index(True), rs.index(True, np.arange(900))
    multi = B.Index.create_multi(rs.codes, rs.corr, rs.dim, rs.cdp, [0, 0], pilot_rows=512)
    shard = B.Index(rs.codes, rs.corr, rs.dim, rs.cdp, row_base=1024)
    pilot = B.Index(rs.codes, rs.corr, rs.dim, rs.cdp, row_base=1024, pilot_codes=rs.codes[:512], pilot_corr=rs.corr[:512])
    drop = np.array([1, 2, 3], np.int32)
    try:
        def snapshot(ix):
            return (ix.n, ix.capacity, ix.export()[0].tobytes(), canon64(ix.export()[1]).tobytes(), file_bytes(ix, str(tmp_path / "snap"), rs.cen, rs.sim))

        before = snapshot(root)
        half = np.arange(n) % 2 == 0
        with capi.Filter(other, np.ones(900, bool)) as small, capi.Filter(root, half) as fits:
            # a filter made for another size
            assert L.bbq_index_compact(root._h, small._h) == capi.ERR_INVALID_ARG
            assert L.bbq_index_compact(root._h, None) == capi.ERR_INVALID_ARG
            assert snapshot(root) == before
            # out of scope: a multi-device handle, a shard with row_base > 0, an index with a pilot replica
            for ix in (multi, shard, pilot):
                assert L.bbq_index_compact(ix._h, fits._h) == capi.ERR_UNSUPPORTED
                assert L.bbq_index_remove_rows(ix._h, drop.ctypes.data, 3) == capi.ERR_UNSUPPORTED
                assert L.bbq_index_size(ix._h) == n
            check_export(shard, rs.codes, rs.corr, "refused shard")
            # a bbq_shard_scan_begin batch that has not been waited for
            k, nq = 10, len(rs.orc.qq)
            cap = int(root.shard_list_cap(k)) * nq
            d_packed = torch.zeros(cap, dtype=torch.int64, device="cuda")
            d_off = torch.zeros(nq + 1, dtype=torch.int64, device="cuda")
            d_flags = torch.zeros(nq, dtype=torch.int32, device="cuda")
            root.shard_scan_begin(rs.orc.qq, rs.orc.qc, rs.qb, rs.sim, k, d_packed.data_ptr(), cap, d_off.data_ptr(), d_flags.data_ptr())
            assert L.bbq_index_compact(root._h, fits._h) == capi.ERR_INVALID_ARG
            assert L.bbq_index_remove_rows(root._h, drop.ctypes.data, 3) == capi.ERR_INVALID_ARG
            root.shard_scan_wait()
            assert snapshot(root) == before
            # ... and waited for, the root index compacts; a sharded scan of it afterwards equals the oracle
            root.compact(fits)
            with pytest.raises(B.BBQError) as e:   # the used filter afterwards
                root.search_filtered_batch(rs.orc.qq, rs.orc.qc, rs.qb, rs.sim, 3, fits)
            assert e.value.code == capi.ERR_INVALID_ARG
        kept = np.flatnonzero(half)
        orc = rs.oracle_over(kept)
        cap = int(root.shard_list_cap(k)) * nq
        d_packed = torch.zeros(cap, dtype=torch.int64, device="cuda")
        total = root.shard_scan(orc.qq, orc.qc, rs.qb, rs.sim, k, d_packed.data_ptr(), cap, d_off.data_ptr(), d_flags.data_ptr())
        assert int(d_flags.abs().sum().item()) == 0
        idx, sc, cnt = B.replay_batch([d_packed[:total].cpu().numpy().view(np.uint64)], [d_off.cpu().numpy()], nq, len(kept), k)
        for qi in range(nq):
            wi, ws = orc.topk(qi, k)
            np.testing.assert_array_equal(idx[qi, :cnt[qi]], wi)
            np.testing.assert_array_equal(canon32(sc[qi, :cnt[qi]]), canon32(ws))
    finally:
        for h in (root, other, multi, shard, pilot):
            h.close()


# ------------------------------------------------------------------------------------------------ 6. the fp32 side of the rerank recipe

@pytest.mark.parametrize("selector,how", [(0, "heap"), (1, "sort")])
@pytest.mark.parametrize("dim", [96, 129])
def test_vectors_compact_and_rerank(dim, selector, how):
    sim, n, k, factor = 1, 1000, 10, 5
    base = O.mulberry32(221 + dim, n * dim).reshape(n, dim)
    queries = O.mulberry32(222, 3 * dim).reshape(3, dim)
    codes, corr, cen = O.build_index(base, sim)
    cdp = O.centroid_dp(cen)
    mask = np.random.default_rng(223).random(n) < 0.5
    mask[[0, 63, 64, 999]] = [True, False, True, True]
    kept = np.flatnonzero(mask)
    orc = Oracle(codes[kept], corr[kept], dim, cen, sim, 4, queries)
    ix, dv = make_index(codes, corr, dim, cdp, True), B.Vectors(base)
    whole_ix, whole_dv = make_index(codes[kept], corr[kept], dim, cdp, True), B.Vectors(base[kept])
    try:
        with capi.Filter(ix, mask) as flt:
            ix.compact(flt)
            dv.compact(flt)
            assert dv.n == len(kept) == capi.lib().bbq_vectors_size(dv._h)
            assert capi.lib().bbq_vectors_compact(dv._h, flt._h) == capi.ERR_INVALID_ARG   # made for the old size
            assert dv.n == len(kept)
        with capi.Filter(ix, np.ones(len(kept), bool)) as everything:
            dv.compact(everything)                                                       # every row kept: nothing changes
        assert dv.n == len(kept)
        rows = [np.array([0, 1, len(kept) // 2, len(kept) - 1], np.int32)] * 3
        for x, y, r in zip(dv.rerank_scores(queries, rows, 1), whole_dv.rerank_scores(queries, rows, 1), rows):
            np.testing.assert_array_equal(canon64(x), canon64(y))
        got = B.search_rerank_batch(ix, dv, queries, orc.qq, orc.qc, 4, sim, k, factor, selector, 1)
        want = B.search_rerank_batch(whole_ix, whole_dv, queries, orc.qq, orc.qc, 4, sim, k, factor, selector, 1)
        for qi in range(3):
            cand, csc = orc.topk(qi, k * factor)   # the recipe over vectors[mask]: candidates, their true scores, the reference's selector
            true = O.true_similarity(queries[qi:qi + 1], base[kept][cand], 1)[0]
            pos = O.rerank_select(true, k, how)
            np.testing.assert_array_equal(got[0][qi, :got[3][qi]], cand[pos])
            np.testing.assert_array_equal(canon32(got[1][qi, :got[3][qi]]), canon32(csc[pos]))
            np.testing.assert_array_equal(canon64(got[2][qi, :got[3][qi]]), canon64(true[pos]))
        for a, b in zip(got, want):
            np.testing.assert_array_equal(np.asarray(a).view(np.uint8), np.asarray(b).view(np.uint8))
        with capi.Filter(ix, np.zeros(len(kept), bool)) as nothing:
            dv.compact(nothing)
        assert dv.n == 0
    finally:
        for h in (ix, dv, whole_ix, whole_dv):
            h.close()


# ------------------------------------------------------------------------------------------------ the Python mirror

def test_api_remove_and_compact_vectors_on_the_device():
    sim, dim, n = 1, 100, 400
    a = O.mulberry32(231, n * dim).reshape(n, dim)
    q = O.mulberry32(233, dim)
    fmt = B.BinaryQuantizationFormat({"queryBits": 4, "indexBits": 1, "quantizer": {"similarityFunction": "COSINE", "lambda": 0.1, "iters": 5}})
    tv = fmt.quantizeVectors(list(a))["quantizedVectors"]
    codes, corr, cen = O.build_index(a, sim)
    keep = np.ones(n, bool)
    keep[[399, 7, 64, 7]] = False
    assert fmt.removeVectors(tv, [399, 7, 64, 7]) is tv and tv.size() == n - 3 and tv._device().n == n - 3
    mask = np.arange(n - 3) % 3 != 1
    assert fmt.compactVectors(tv, mask) is tv
    kept = np.flatnonzero(keep)[mask]
    assert tv.size() == len(kept) == tv._device().n
    for ord_ in (0, 1, 63, 64, len(kept) - 1):
        np.testing.assert_array_equal(tv.vectorValue(ord_), codes[kept[ord_]])
        t = tv.getCorrectiveTerms(ord_)
        got = np.array([t["lowerInterval"], t["upperInterval"], t["additionalCorrection"], t["quantizedComponentSum"]])
        np.testing.assert_array_equal(canon64(got), canon64(corr[kept[ord_]]))
    wi, ws = O.search(q, codes[kept], corr[kept], cen, sim, 4, 25)
    got = fmt.searchNearestNeighbors(q, tv, 25)
    assert [r["index"] for r in got] == list(wi)
    np.testing.assert_array_equal(canon32([r["score"] for r in got]), canon32(ws))
    with pytest.raises(Exception, match="向量索引 %d 不存在" % len(kept)):
        fmt.removeVectors(tv, [len(kept)])
    assert tv.size() == len(kept) == tv._device().n
