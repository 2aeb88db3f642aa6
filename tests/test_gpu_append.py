"""GPU: rows appended to a device-resident index (bbq_index_append_rows, bbq_index_append, bbq_index_reserve, bbq_vectors_append).
The contract: after an append the index is indistinguishable from one created whole over the old rows followed by the new ones.  The
expected value is always the ORACLE over all rows - orc_score_all + the reference heap over rows from orc_build_index* or from the
per-row recipe (orc_normalize, orc_scalar_quantize against the build's centroid, orc_pack_binary; tests/test_append_cpu.py holds the
recipe to the oracle's own build) - and a twin index created whole is compared as well.  Bit-exact: indices, f32 score bits and
order, ties included; no tolerances."""
import os

import numpy as np
import pytest

import orclib as O
from bbqlib import bbq_amd as B, capi
from append_recipe import oracle_rows

pytestmark = pytest.mark.gpu


def canon32(a):
    a = np.array(a, np.float32)
    a[np.isnan(a)] = np.nan
    return a.view(np.uint32)


def canon64(a):
    a = np.array(a, np.float64)
    a[np.isnan(a)] = np.nan
    return a.view(np.uint64)


def _reference_accepts(name):
    return not any("per_row_error" in rec for rec in O.load_golden(name)["queries"])


_WANTED = ("ties_", "m_768d_", "m_100d_", "ib2_", "ib4_", "ib8_", "big_20000x128_cos", "big_50000x768_cos", "big_30000x1536_mip",
           "big_20000x1024_euc_qb8", "edge_dim1")
CASES = [n for n in O.golden_names() if n.startswith(_WANTED) and _reference_accepts(n)]
CUTS = (0, 1, 63, 64, 65, 511, 512, 513)   # 0: an index created over zero rows, every row appended
VARIANTS = ({}, {"force_dense": 1}, {"sweep_share": 4}, {"sweep_share": 32}, {"device_select": 0})


def make_index(codes, corr, dim, cdp, compact, ib=1, **kw):
    return B.Index(codes, corr, dim, cdp, corrections="compact" if compact else "inline", index_bits=ib, **kw)


def grown_index(codes, corr, dim, cdp, compact, ib, bounds):
    """an index created over rows [0, bounds[0]) and grown piece by piece to bounds[-1]"""
    ix = make_index(codes[:bounds[0]], corr[:bounds[0]], dim, cdp, compact, ib)
    for a, b in zip(bounds, bounds[1:]):
        ix.append_rows(codes[a:b], corr[a:b])
        assert ix.n == b
    return ix


class Oracle:
    """the expected answers of one row set: per query the oracle's f32 scores of ALL rows, heaps on demand"""

    def __init__(self, codes, corr, dim, cen, sim, qb, queries, ib=1, lam=0.1, iters=5):
        self.sim, self.qb, self.n = sim, qb, codes.shape[0]
        qs = [B.quantize_query(q, cen, sim, qb, lam, iters) for q in queries]
        self.qq, self.qc = np.stack([a for a, _ in qs]), np.stack([b for _, b in qs])
        self.scores = [O.score_all(codes, corr, dim, self.qq[i], self.qc[i], qb, sim, O.centroid_dp(cen), ib=ib) for i in range(len(qs))]
        self._heaps = {}

    def topk(self, qi, k):
        if (qi, k) not in self._heaps:
            self._heaps[(qi, k)] = O.heap_topk(self.scores[qi][2], k)
        return self._heaps[(qi, k)]

    def check_search(self, ix, ks, msg, single=False):
        for k in ks:
            idx, sc, cnt = ix.search_batch(self.qq, self.qc, self.qb, self.sim, k)
            for qi in range(len(self.qq)):
                wi, ws = self.topk(qi, k)
                assert cnt[qi] == len(wi) == min(k, self.n)
                np.testing.assert_array_equal(idx[qi, :cnt[qi]], wi, err_msg="%s q%d k=%d" % (msg, qi, k))
                np.testing.assert_array_equal(canon32(sc[qi, :cnt[qi]]), canon32(ws), err_msg="%s q%d k=%d" % (msg, qi, k))
                if single:  # the single-query call takes paths of its own (fused latency chain, pre-sampled threshold)
                    i1, s1 = ix.search(self.qq[qi], self.qc[qi], self.qb, self.sim, k)
                    np.testing.assert_array_equal(i1, wi, err_msg="%s single q%d k=%d" % (msg, qi, k))
                    np.testing.assert_array_equal(canon32(s1), canon32(ws))

    def check_score_rows(self, ix, msg):
        for qi in range(len(self.qq)):
            d, s64, s32 = ix.score_rows(self.qq[qi], self.qc[qi], self.qb, self.sim)
            od, os64, os32 = self.scores[qi]
            np.testing.assert_array_equal(d, od, err_msg=msg)
            np.testing.assert_array_equal(canon64(s64), canon64(os64), err_msg=msg)
            np.testing.assert_array_equal(canon32(s32), canon32(os32), err_msg=msg)


def check_export(ix, codes, corr, msg):
    c, r = ix.export()
    np.testing.assert_array_equal(c, codes, err_msg=msg)
    np.testing.assert_array_equal(canon64(r), canon64(corr), err_msg=msg)


def file_bytes(ix, prefix, cen, sim):
    ix.save(prefix, cen, sim)
    return open(prefix + ".veb", "rb").read(), open(prefix + ".vemb", "rb").read()


# ------------------------------------------------------------------------------------------------ 1. append_rows parity

@pytest.mark.parametrize("compact", [True, False])
@pytest.mark.parametrize("name", CASES)
def test_append_rows_parity(name, compact, tmp_path):
    g = O.load_golden(name)
    sim, n, dim, ib, qb = O.SIMS[g["sim"]], g["n"], g["dim"], g["ib"], g["qb"]
    base, queries = O.golden_inputs(g)
    codes, corr, cen = O.build_index(base, sim, g["lambda"], g["iters"], ib=ib)   # the rows are the oracle's
    cdp = O.centroid_dp(cen)
    orc = Oracle(codes, corr, dim, cen, sim, qb, queries, ib, g["lambda"], g["iters"])
    ks = sorted({1, 10, 100, n, n + 5})
    twin = make_index(codes, corr, dim, cdp, compact, ib)
    twin_files = file_bytes(twin, str(tmp_path / "twin"), cen, sim)
    splits = [[c, n] for c in sorted({c for c in CUTS + (n - 1,) if 0 <= c < n})]
    if n >= 3:
        splits.append([n // 3, 2 * n // 3, n])   # three pieces
    try:
        for bounds in splits:
            msg = "%s compact=%s pieces=%s" % (name, compact, bounds)
            ix = grown_index(codes, corr, dim, cdp, compact, ib, bounds)
            try:
                assert ix.n == n and capi.lib().bbq_index_size(ix._h) == n
                assert ix.bytes_per_row == twin.bytes_per_row
                check_export(ix, codes, corr, msg)
                orc.check_score_rows(ix, msg)
                for opts in VARIANTS:
                    for name_, v in opts.items():
                        ix.set_option(name_, v)
                    orc.check_search(ix, ks, "%s %s" % (msg, opts), single=not opts)
                    for name_ in opts:
                        ix.set_option(name_, {"force_dense": 0, "sweep_share": 1, "device_select": 1}[name_])
                # the files are the twin's, byte for byte: padding lanes of the last tile and add_range of every touched tile included
                assert file_bytes(ix, str(tmp_path / "grown"), cen, sim) == twin_files, msg
            finally:
                ix.close()
        orc.check_search(twin, ks, name + " twin")
    finally:
        twin.close()


# ------------------------------------------------------------------------------------------------ 2. ties across the seam

@pytest.mark.parametrize("compact", [True, False])
@pytest.mark.parametrize("sim,qb", [(1, 4), (0, 4), (2, 1)])
def test_ties_across_the_seam(sim, qb, compact):
    """the appended block repeats existing rows - among them the queries' best - so equal scores sit on both sides of old_size, inside
    the answer and at its edge: index order and score bits must be the oracle heap's"""
    dim, n_old = 64, 1500
    a = O.mulberry32(31, n_old * dim).reshape(n_old, dim)
    queries = O.mulberry32(32, 3 * dim).reshape(3, dim)
    ocodes, ocorr, cen = O.build_index(a, sim)
    probe = Oracle(ocodes, ocorr, dim, cen, sim, qb, queries)
    best = np.unique(np.concatenate([probe.topk(qi, 12)[0] for qi in range(3)]))
    rows = np.concatenate([best, best[::-1], np.arange(0, n_old, 7), best])
    bcodes, bcorr = ocodes[rows], ocorr[rows]
    allc, allr = np.concatenate([ocodes, bcodes]), np.concatenate([ocorr, bcorr])
    orc = Oracle(allc, allr, dim, cen, sim, qb, queries)
    assert any(len(np.unique(canon32(orc.topk(qi, 10)[1]))) < 10 for qi in range(3)), "no tie inside the answers: the case is void"
    ix = make_index(ocodes, ocorr, dim, O.centroid_dp(cen), compact)
    try:
        ix.append_rows(bcodes, bcorr)
        for opts in ({}, {"device_select": 0}, {"sweep_share": 4}, {"force_dense": 1}):
            for k_, v in opts.items():
                ix.set_option(k_, v)
            orc.check_search(ix, [1, 2, 3, 10, 12, 13, 36, 37, 100, ix.n], "seam %s" % opts, single=True)
            for k_ in opts:
                ix.set_option(k_, {"force_dense": 0, "sweep_share": 1, "device_select": 1}[k_])
        check_export(ix, allc, allr, "seam")
    finally:
        ix.close()


# ------------------------------------------------------------------------------------------------ 3. raw append

# (dimension 1 only with 1-bit rows: a multi-bit index of dimension 1 is stored as packed 1-bit rows, whose popcounts are not their code
# sums - whether five built rows already force explicit sums, and with them an index that takes any row, is a matter of their values)
RAW = [(sim, dim, na, nb, ib) for sim, dim, na, nb in [(1, 768, 1000, 700), (0, 100, 257, 65), (2, 64, 64, 1), (1, 1536, 130, 513), (2, 1, 5, 70)]
       for ib in (1, 2, 4) if dim > 1 or ib == 1]


@pytest.mark.parametrize("compact", [True, False])
@pytest.mark.parametrize("sim,dim,na,nb,ib", RAW)
def test_raw_append_equals_the_oracle_recipe(sim, dim, na, nb, ib, compact, tmp_path):
    a = O.mulberry32(41 + dim, na * dim).reshape(na, dim)
    b = O.mulberry32(43 + dim, nb * dim).reshape(nb, dim).copy()
    b[0] = 0.0
    if nb > 2:
        b[2] = -1.25
    queries = O.mulberry32(44, 2 * dim).reshape(2, dim)
    acodes, acorr, cen = O.build_index(a, sim, ib=ib)
    bcodes, bcorr = oracle_rows(b, cen, sim, ib)
    allc, allr = np.concatenate([acodes, bcodes]), np.concatenate([acorr, bcorr])
    ix, codes, corr, bcen = B.Index.build(a, sim, index_bits=ib, corrections="compact" if compact else "inline")
    try:
        np.testing.assert_array_equal(bcen.view(np.uint32), cen.view(np.uint32))
        half = nb // 2
        got1 = ix.append(b[:half], cen, sim)                       # (an empty block when nb == 1)
        got2 = ix.append(b[half:], cen, sim)
        assert ix.n == na + nb
        np.testing.assert_array_equal(np.concatenate([got1[0], got2[0]]), bcodes)
        np.testing.assert_array_equal(canon64(np.concatenate([got1[1], got2[1]])), canon64(bcorr))
        check_export(ix, allc, allr, "raw append")
        qb = 4
        orc = Oracle(allc, allr, dim, cen, sim, qb, queries, ib)
        orc.check_score_rows(ix, "raw append")
        orc.check_search(ix, sorted({1, 10, 100, ix.n, ix.n + 5}), "raw append", single=True)
        # ... without host copies, and the files of a twin created whole from the same rows: the rows as the device made them (they
        # equal the oracle's up to the bits of a NaN - a 1-d row has a zero-width interval - which a file keeps as they are)
        assert ix.append(b[:3], cen, sim, want_host_copy=False) == (None, None)
        allc, allr = np.concatenate([allc, bcodes[:3]]), np.concatenate([allr, bcorr[:3]])
        check_export(ix, allc, allr, "raw append without host copies")
        new_c, new_r = np.concatenate([got1[0], got2[0]]), np.concatenate([got1[1], got2[1]])
        twin = make_index(np.concatenate([codes, new_c, new_c[:3]]), np.concatenate([corr, new_r, new_r[:3]]), dim, O.centroid_dp(cen), compact, ib)
        try:
            assert file_bytes(ix, str(tmp_path / "grown"), cen, sim) == file_bytes(twin, str(tmp_path / "twin"), cen, sim)
        finally:
            twin.close()
    finally:
        ix.close()


@pytest.mark.parametrize("compact", [True, False])
@pytest.mark.parametrize("sim,dim,n,ib", [(1, 64, 1, 1), (0, 100, 64, 1), (2, 64, 130, 1), (1, 100, 130, 2)])
def test_build_equals_raw_append_to_empty(sim, dim, n, ib, compact, tmp_path):
    """a build is a raw append to an empty index: one lane, exactly a tile, two tiles and a partly filled third"""
    rows = O.mulberry32(141 + n, n * dim).reshape(n, dim)
    queries = O.mulberry32(142, 2 * dim).reshape(2, dim)
    ocodes, ocorr, ocen = O.build_index(rows, sim, ib=ib)
    a, acodes, acorr, cen = B.Index.build(rows, sim, index_bits=ib, corrections="compact" if compact else "inline")
    b = make_index(ocodes[:0], ocorr[:0], dim, O.centroid_dp(cen), compact, ib)
    try:
        np.testing.assert_array_equal(cen.view(np.uint32), ocen.view(np.uint32))
        bcodes, bcorr = b.append(rows, cen, sim)
        assert a.n == b.n == n
        for codes, corr in ((acodes, acorr), (bcodes, bcorr)):
            np.testing.assert_array_equal(codes, ocodes)
            np.testing.assert_array_equal(canon64(corr), canon64(ocorr))
        assert a.bytes_per_row == b.bytes_per_row
        assert a.capacity == b.capacity
        fa, fb = file_bytes(a, str(tmp_path / "built"), cen, sim), file_bytes(b, str(tmp_path / "appended"), cen, sim)
        assert fa[0] == fb[0] and fa[1] == fb[1]
        orc = Oracle(ocodes, ocorr, dim, ocen, sim, 4, queries, ib)
        for ix, msg in ((a, "built"), (b, "appended to empty")):
            orc.check_search(ix, sorted({1, 10, n}), msg)
    finally:
        a.close()
        b.close()


def test_raw_append_to_an_index_with_explicit_sums():
    """an index created from rows whose quantizedComponentSum is not their popcount stores the sums: it takes any row, raw rows too"""
    sim, dim = 1, 96
    a = O.mulberry32(51, 300 * dim).reshape(300, dim)
    b = O.mulberry32(52, 100 * dim).reshape(100, dim)
    acodes, acorr, cen = O.build_index(a, sim)
    acorr[::7, 3] += 2.0
    bcodes, bcorr = oracle_rows(b, cen, sim, 1)
    odd = bcorr.copy()
    odd[::3, 3] -= 1.0
    allc, allr = np.concatenate([acodes, bcodes, bcodes]), np.concatenate([acorr, bcorr, odd])
    ix = B.Index(acodes, acorr, dim, O.centroid_dp(cen))
    try:
        got = ix.append(b, cen, sim)
        np.testing.assert_array_equal(got[0], bcodes)
        np.testing.assert_array_equal(canon64(got[1]), canon64(bcorr))
        ix.append_rows(bcodes, odd)
        check_export(ix, allc, allr, "explicit sums")
        orc = Oracle(allc, allr, dim, cen, sim, 4, O.mulberry32(53, 2 * dim).reshape(2, dim))
        orc.check_score_rows(ix, "explicit sums")
        orc.check_search(ix, [1, 10, 100, ix.n], "explicit sums", single=True)
    finally:
        ix.close()


# ------------------------------------------------------------------------------------------------ 4. failure leaves the index unchanged

def _snapshot(ix, orc, tmp_path, cen, sim):
    return (ix.n, ix.capacity, ix.export()[0].tobytes(), canon64(ix.export()[1]).tobytes(), file_bytes(ix, str(tmp_path / "snap"), cen, sim),
            [a.tobytes() for a in ix.search_batch(orc.qq, orc.qc, orc.qb, orc.sim, 20)])


@pytest.mark.parametrize("compact", [True, False])
@pytest.mark.parametrize("n_old", [1000, 1024])
def test_failed_append_leaves_the_index_unchanged(n_old, compact, tmp_path):
    sim, dim = 1, 128
    a = O.mulberry32(61, n_old * dim).reshape(n_old, dim)
    b = O.mulberry32(62, 200 * dim).reshape(200, dim).copy()
    queries = O.mulberry32(63, 2 * dim).reshape(2, dim)
    ix, codes, corr, cen = B.Index.build(a, sim, corrections="compact" if compact else "inline")
    orc = Oracle(codes, corr, dim, cen, sim, 4, queries)
    try:
        before = _snapshot(ix, orc, tmp_path, cen, sim)
        for val, code, row, col in ((np.nan, capi.ERR_NAN_INPUT, 150, 0), (np.inf, capi.ERR_NAN_INPUT, 150, 17), (-np.inf, capi.ERR_NAN_INPUT, 150, 17)):
            bad = b.copy()
            bad[150, 17] = val   # COSINE validates the normalised rows: see tests/test_append_cpu.py for the position and the code
            bad[199, 3] = val
            with pytest.raises(B.BBQError) as e:
                ix.append(bad, cen, sim)
            assert (e.value.code, e.value.bad_row, e.value.bad_col) == (code, row, col)
            with pytest.raises(B.BBQError) as e2:
                B.quantize_rows(bad, cen, sim)
            assert (e2.value.code, e2.value.bad_row, e2.value.bad_col, str(e2.value)) == (code, row, col, str(e.value))
            assert _snapshot(ix, orc, tmp_path, cen, sim) == before
        for esim, val, code in ((0, np.inf, capi.ERR_INF_INPUT), (2, np.nan, capi.ERR_NAN_INPUT)):
            bad = b.copy()
            bad[42, 99] = val
            with pytest.raises(B.BBQError) as e:
                ix.append(bad, cen, esim)
            assert (e.value.code, e.value.bad_row, e.value.bad_col) == (code, 42, 99)
            assert _snapshot(ix, orc, tmp_path, cen, sim) == before
        # a row whose component sum is not its popcount: the index stores no sums
        bcodes, bcorr = oracle_rows(b, cen, sim, 1)
        odd = bcorr.copy()
        odd[77, 3] += 1.0
        with pytest.raises(B.BBQError) as e:
            ix.append_rows(bcodes, odd)
        assert e.value.code == capi.ERR_UNSUPPORTED and "quantizedComponentSum" in str(e.value)
        assert _snapshot(ix, orc, tmp_path, cen, sim) == before
        # bad arguments
        with pytest.raises(B.BBQError) as e:
            ix.append(b[:, :100], cen[:100], sim)
        assert e.value.code == capi.ERR_DIM_MISMATCH
        f = np.ascontiguousarray(b)
        assert capi.lib().bbq_index_append(ix._h, f.ctypes.data, 200, cen.ctypes.data, 7, 0.1, 5, None, None, None, None) == capi.ERR_INVALID_ARG
        assert capi.lib().bbq_index_append(ix._h, f.ctypes.data, 200, None, sim, 0.1, 5, None, None, None, None) == capi.ERR_INVALID_ARG
        assert capi.lib().bbq_index_append(ix._h, f.ctypes.data, -1, cen.ctypes.data, sim, 0.1, 5, None, None, None, None) == capi.ERR_INVALID_ARG
        assert capi.lib().bbq_index_append_rows(ix._h, None, bcorr.ctypes.data, 5) == capi.ERR_INVALID_ARG
        assert capi.lib().bbq_index_append(ix._h, f.ctypes.data, 2**32, cen.ctypes.data, sim, 0.1, 5, None, None, None, None) == capi.ERR_UNSUPPORTED
        assert capi.lib().bbq_index_append_rows(ix._h, None, None, 0) == capi.OK     # n == 0 changes nothing
        assert capi.lib().bbq_index_append(ix._h, None, 0, None, sim, 0.1, 5, None, None, None, None) == capi.OK
        assert _snapshot(ix, orc, tmp_path, cen, sim) == before
        # ... and the index still takes the good rows
        ix.append_rows(bcodes, bcorr)
        check_export(ix, np.concatenate([codes, bcodes]), np.concatenate([corr, bcorr]), "after the failures")
    finally:
        ix.close()


@pytest.mark.parametrize("compact", [True, False])
def test_failed_append_multibit_code_out_of_range(compact, tmp_path):
    sim, dim, ib = 0, 100, 2
    a = O.mulberry32(64, 200 * dim).reshape(200, dim)
    codes, corr, cen = O.build_index(a, sim, ib=ib)
    orc = Oracle(codes, corr, dim, cen, sim, 4, O.mulberry32(65, 2 * dim).reshape(2, dim), ib)
    ix = make_index(codes[:130], corr[:130], dim, O.centroid_dp(cen), compact, ib)
    try:
        small = Oracle(codes[:130], corr[:130], dim, cen, sim, 4, O.mulberry32(65, 2 * dim).reshape(2, dim), ib)
        before = _snapshot(ix, small, tmp_path, cen, sim)
        bad_codes, bad_corr = codes[130:].copy(), corr[130:].copy()
        bad_corr[69, 3] += 4 - float(bad_codes[69, 99])   # (the sum stays the code sum: only the range is wrong)
        bad_codes[69, 99] = 4                              # 2^indexBits
        with pytest.raises(B.BBQError) as e:
            ix.append_rows(bad_codes, bad_corr)
        assert e.value.code == capi.ERR_INVALID_ARG and str(e.value) == "indexBits=2: a quantized value is not below 4"
        assert _snapshot(ix, small, tmp_path, cen, sim) == before
        ix.append_rows(codes[130:], corr[130:])
        orc.check_search(ix, [1, 10, 200], "after the refused rows")
    finally:
        ix.close()


@pytest.mark.parametrize("compact", [True, False])
def test_an_emptied_index_decides_its_format_like_one_created_over_zero_rows(compact, tmp_path):
    """The one place where "an index without explicit sums refuses a row whose quantizedComponentSum is not its popcount" does not
    hold: an index that holds neither rows nor room.  A compaction to zero rows leaves "the index of zero rows", and that index - like
    one created over zero rows - decides its record format at its next append: it takes the odd row and stores explicit sums from then
    on, exactly as a twin created whole over those rows.  With room reserved first the format stays decided and the row is refused."""
    sim, dim, n = 1, 96, 130
    base = O.mulberry32(66, n * dim).reshape(n, dim)
    codes, corr, cen = O.build_index(base, sim)
    cdp = O.centroid_dp(cen)
    odd = corr.copy()
    odd[[3, 64], 3] += 2.0
    orc = Oracle(codes, odd, dim, cen, sim, 4, O.mulberry32(67, 2 * dim).reshape(2, dim))
    emptied, fresh, twin = make_index(codes, corr, dim, cdp, compact), make_index(codes[:0], corr[:0], dim, cdp, compact), make_index(codes, odd, dim, cdp, compact)
    kept_room = make_index(codes, corr, dim, cdp, compact)
    try:
        with pytest.raises(B.BBQError) as e:             # while it holds rows, the index refuses the rows
            emptied.append_rows(codes, odd)
        assert e.value.code == capi.ERR_UNSUPPORTED
        emptied.remove_rows(np.arange(n))
        assert (emptied.n, emptied.capacity) == (0, 0)
        want = file_bytes(twin, str(tmp_path / "twin"), cen, sim)
        for ix, msg in ((emptied, "emptied"), (fresh, "created over zero rows")):
            ix.append_rows(codes, odd)
            assert (ix.n, ix.capacity, ix.bytes_per_row) == (n, twin.capacity, twin.bytes_per_row), msg
            check_export(ix, codes, odd, msg)
            assert file_bytes(ix, str(tmp_path / "grown"), cen, sim) == want, msg
            orc.check_search(ix, [1, 10, n], msg, single=True)
            orc.check_score_rows(ix, msg)
        # emptied, but with room: the allocations exist in the format decided at creation, and the row is refused
        kept_room.remove_rows(np.arange(n))
        kept_room.reserve(64)
        before = (kept_room.n, kept_room.capacity, file_bytes(kept_room, str(tmp_path / "before"), cen, sim))
        with pytest.raises(B.BBQError) as e:
            kept_room.append_rows(codes, odd)
        assert e.value.code == capi.ERR_UNSUPPORTED
        assert (kept_room.n, kept_room.capacity, file_bytes(kept_room, str(tmp_path / "after"), cen, sim)) == before
    finally:
        for h in (emptied, fresh, twin, kept_room):
            h.close()


# ------------------------------------------------------------------------------------------------ 5. capacity

@pytest.mark.parametrize("compact", [True, False])
def test_reserve_and_geometric_growth(compact):
    sim, dim, n = 1, 64, 12000
    base = O.mulberry32(71, n * dim).reshape(n, dim)
    codes, corr, cen = O.build_index(base, sim)
    queries = O.mulberry32(72, 2 * dim).reshape(2, dim)
    ix = make_index(codes[:1000], corr[:1000], dim, O.centroid_dp(cen), compact)
    try:
        assert ix.capacity == 1024                       # whole 64-row tiles
        ix.reserve(500)
        assert ix.capacity == 1024                       # never shrinks
        ix.reserve(3000)
        assert ix.capacity == 3008                       # exactly what was asked for, in tiles
        Oracle(codes[:1000], corr[:1000], dim, cen, sim, 4, queries).check_search(ix, [1, 10, 1000], "after reserve", single=True)
        at = 1000
        for step in (1, 63, 500, 1000, 444):             # ... to 3008 rows: inside the reservation
            ix.append_rows(codes[at:at + step], corr[at:at + step])
            at += step
            assert (ix.n, ix.capacity) == (at, 3008)
            check_export(ix, codes[:at], corr[:at], "inside the reservation")
        Oracle(codes[:at], corr[:at], dim, cen, sim, 4, queries).check_search(ix, [1, 10, 100, at], "inside the reservation", single=True)
        ix.append_rows(codes[at:at + 1], corr[at:at + 1])   # one row too many: max(tiles needed, 1.5 x tiles held) = 70 tiles
        at += 1
        assert (ix.n, ix.capacity) == (at, 47 * 3 // 2 * 64)
        ix.append_rows(codes[at:5000], corr[at:5000])     # 79 tiles needed, 1.5 x 70 = 105 held
        assert (ix.n, ix.capacity) == (5000, 105 * 64)
        ix.append_rows(codes[5000:n], corr[5000:n])       # beyond 1.5 x 105 = 157 tiles: what is needed, 188 tiles
        assert (ix.n, ix.capacity) == (n, 188 * 64)
        check_export(ix, codes, corr, "after growth")
        orc = Oracle(codes, corr, dim, cen, sim, 4, queries)
        orc.check_search(ix, [1, 10, 100, n, n + 5], "after growth", single=True)
        orc.check_score_rows(ix, "after growth")
        assert capi.lib().bbq_index_reserve(ix._h, -1) == capi.ERR_INVALID_ARG
        assert capi.lib().bbq_index_reserve(ix._h, 2**32) == capi.ERR_UNSUPPORTED
    finally:
        ix.close()


# ------------------------------------------------------------------------------------------------ 6. crossing path switches

def test_growth_across_path_switches():
    """a 64-d index grown from 1 000 rows past 262 144 (single-query calls start to pre-sample their threshold there) and past
    6 000 000 (the default sub-batch of a 256-query call halves there, effective_batch): single-query calls and 256-query batches
    against the oracle after each step.  The rows are synthetic (codes and corrections drawn directly: an append of quantized rows asks
    nothing of where they come from); a row's score does not depend on the rows behind it, so the oracle scores every query once over
    all rows and the heaps run over the prefixes."""
    from concurrent.futures import ThreadPoolExecutor
    sim, dim, qb, nq = 1, 64, 4, 256
    sizes = [1000, 70000, 262143, 262144, 262145, 300000, 2500000, 5999999, 6000000, 6100000]
    ks, singles = (1, 10, 100), (0, 1, 2, 3, 100, 200, 254, 255)
    n = sizes[-1]
    rng = np.random.default_rng(81)
    codes = rng.integers(0, 256, (n, dim // 8), dtype=np.uint8)
    corr = np.empty((n, 4), np.float64)
    corr[:, 0] = -0.2 - 0.1 * rng.random(n)
    corr[:, 1] = 0.2 + 0.1 * rng.random(n)
    corr[:, 2] = 0.05 * rng.standard_normal(n)
    corr[:, 3] = np.unpackbits(codes, axis=1).sum(axis=1)
    cen = (0.01 * rng.standard_normal(dim)).astype(np.float32)
    cdp = O.centroid_dp(cen)
    qq, qc = B.quantize_queries(rng.standard_normal((nq, dim)).astype(np.float32), cen, sim, qb)
    got = {}
    ix = make_index(codes[:sizes[0]], corr[:sizes[0]], dim, cdp, True)
    try:
        for at, nxt in zip(sizes, sizes[1:] + [None]):
            assert ix.n == at
            for k in ks:
                idx, sc, cnt = ix.search_batch(qq, qc, qb, sim, k)
                assert (cnt == k).all()
                got[(at, k)] = (idx, sc, {qi: ix.search(qq[qi], qc[qi], qb, sim, k) for qi in singles})
            if nxt is not None:
                ix.append_rows(codes[at:nxt], corr[at:nxt])
    finally:
        ix.close()

    def check(qi):
        s32 = O.score_all(codes, corr, dim, qq[qi], qc[qi], qb, sim, cdp)[2]
        for at in sizes:
            for k in ks:
                wi, ws = O.heap_topk(s32[:at], k)
                idx, sc, single = got[(at, k)]
                np.testing.assert_array_equal(idx[qi], wi, err_msg="batch n=%d q%d k=%d" % (at, qi, k))
                np.testing.assert_array_equal(canon32(sc[qi]), canon32(ws), err_msg="batch n=%d q%d k=%d" % (at, qi, k))
                if qi in single:
                    np.testing.assert_array_equal(single[qi][0], wi, err_msg="single n=%d q%d k=%d" % (at, qi, k))
                    np.testing.assert_array_equal(canon32(single[qi][1]), canon32(ws))

    with ThreadPoolExecutor(8) as pool:   # the oracle's C functions run outside the interpreter lock
        list(pool.map(check, range(nq)))


# ------------------------------------------------------------------------------------------------ 7. persistence

@pytest.mark.parametrize("compact", [True, False])
@pytest.mark.parametrize("ib", [1, 2])
def test_save_load_append_again(ib, compact, tmp_path):
    sim, dim, n = 2, 200, 3000
    base = O.mulberry32(91, n * dim).reshape(n, dim)
    codes, corr, cen = O.build_index(base, sim, ib=ib)
    cdp = O.centroid_dp(cen)
    queries = O.mulberry32(92, 2 * dim).reshape(2, dim)
    ix = make_index(codes[:1000], corr[:1000], dim, cdp, compact, ib)
    ix.reserve(4000)                                      # spare capacity must not show in the files
    ix.append_rows(codes[1000:1777], corr[1000:1777])
    twin = make_index(codes[:1777], corr[:1777], dim, cdp, compact, ib)
    try:
        files = file_bytes(ix, str(tmp_path / "grown"), cen, sim)
        assert files == file_bytes(twin, str(tmp_path / "twin"), cen, sim)
        n_tiles = (1777 + 63) // 64
        assert len(files[0]) == n_tiles * (ix.bytes_per_row * 64) + (n_tiles * (64 * 32 + 8) if compact else 0)
        assert B.file_info(str(tmp_path / "grown"))["n_rows"] == 1777
    finally:
        ix.close()
        twin.close()
    ix2, cen2, _ = B.Index.load(str(tmp_path / "grown"))
    try:
        assert (ix2.n, ix2.capacity) == (1777, n_tiles * 64)
        np.testing.assert_array_equal(cen2.view(np.uint32), cen.view(np.uint32))
        ix2.append_rows(codes[1777:2500], corr[1777:2500])
        got = ix2.append(base[2500:], cen2, sim)          # ... and raw rows against the stored centroid
        np.testing.assert_array_equal(got[0], codes[2500:])
        np.testing.assert_array_equal(canon64(got[1]), canon64(corr[2500:]))
        check_export(ix2, codes, corr, "loaded + appended")
        orc = Oracle(codes, corr, dim, cen, sim, 4, queries, ib)
        orc.check_search(ix2, [1, 10, 100, n], "loaded + appended", single=True)
        whole = make_index(codes, corr, dim, cdp, compact, ib)
        try:
            assert file_bytes(ix2, str(tmp_path / "again"), cen, sim) == file_bytes(whole, str(tmp_path / "whole"), cen, sim)
        finally:
            whole.close()
    finally:
        ix2.close()


# ------------------------------------------------------------------------------------------------ 8. filters

@pytest.mark.parametrize("compact", [True, False])
def test_filters_and_appends(compact):
    sim, dim, n_old, n = 1, 128, 5000, 9000
    base = O.mulberry32(101, n * dim).reshape(n, dim)
    codes, corr, cen = O.build_index(base, sim)
    orc = Oracle(codes, corr, dim, cen, sim, 4, O.mulberry32(102, 3 * dim).reshape(3, dim))
    ix = make_index(codes[:n_old], corr[:n_old], dim, O.centroid_dp(cen), compact)
    try:
        old = capi.Filter(ix, np.ones(n_old, bool))
        ix.append_rows(codes[n_old:], corr[n_old:])
        with pytest.raises(B.BBQError) as e:               # made before the append: it no longer fits the index
            ix.search_filtered_batch(orc.qq, orc.qc, 4, sim, 10, old)
        assert e.value.code == capi.ERR_INVALID_ARG
        old.close()
        rng = np.random.default_rng(5)
        masks = {"straddle": (np.arange(n) >= n_old - 100) & (np.arange(n) < n_old + 100), "random_50": rng.random(n) < 0.5,
                 "new_only": np.arange(n) >= n_old, "old_only": np.arange(n) < n_old, "seam_pair": np.isin(np.arange(n), [n_old - 1, n_old]),
                 "ones": np.ones(n, bool), "random_1": rng.random(n) < 0.01}
        for mname, mask in masks.items():
            acc = np.flatnonzero(mask)
            with capi.Filter(ix, mask) as flt:
                assert flt.count == len(acc)
                for k in sorted({1, 10, 100, len(acc), len(acc) + 5}):
                    idx, sc, cnt = ix.search_filtered_batch(orc.qq, orc.qc, 4, sim, k, flt)
                    for qi in range(3):
                        pos, ws = O.heap_topk(orc.scores[qi][2][acc], k)
                        np.testing.assert_array_equal(idx[qi, :cnt[qi]], acc[pos], err_msg="%s q%d k=%d" % (mname, qi, k))
                        np.testing.assert_array_equal(canon32(sc[qi, :cnt[qi]]), canon32(ws))
    finally:
        ix.close()


# ------------------------------------------------------------------------------------------------ 9. rerank

@pytest.mark.parametrize("selector,how", [(0, "heap"), (1, "sort")])
def test_vectors_append_and_rerank(selector, how):
    sim, dim, n_old, n, k, factor = 1, 96, 2000, 3100, 10, 5
    base = O.mulberry32(111, n * dim).reshape(n, dim)
    queries = O.mulberry32(112, 4 * dim).reshape(4, dim)
    codes, corr, cen = O.build_index(base, sim)
    orc = Oracle(codes, corr, dim, cen, sim, 4, queries)
    ix = make_index(codes[:n_old], corr[:n_old], dim, O.centroid_dp(cen), True)
    dv = B.Vectors(base[:n_old])
    whole_ix, whole_dv = make_index(codes, corr, dim, O.centroid_dp(cen), True), B.Vectors(base)
    try:
        ix.append_rows(codes[n_old:], corr[n_old:])
        with pytest.raises(B.BBQError):                   # the fp32 side has not grown yet
            B.search_rerank_batch(ix, dv, queries, orc.qq, orc.qc, 4, sim, k, factor, selector, 1)
        dv.append(base[n_old:2500])
        dv.append(base[2500:])
        assert dv.n == n and capi.lib().bbq_vectors_size(dv._h) == n
        got = B.search_rerank_batch(ix, dv, queries, orc.qq, orc.qc, 4, sim, k, factor, selector, 1)
        want = B.search_rerank_batch(whole_ix, whole_dv, queries, orc.qq, orc.qc, 4, sim, k, factor, selector, 1)
        for qi in range(4):
            cand, csc = orc.topk(qi, k * factor)           # the oracle: candidates, their true scores, the reference's selector
            true = O.true_similarity(queries[qi:qi + 1], base[cand], 1)[0]
            pos = O.rerank_select(true, k, how)
            np.testing.assert_array_equal(got[0][qi, :got[3][qi]], cand[pos])
            np.testing.assert_array_equal(canon32(got[1][qi, :got[3][qi]]), canon32(csc[pos]))
            np.testing.assert_array_equal(canon64(got[2][qi, :got[3][qi]]), canon64(true[pos]))
        for a, b in zip(got, want):
            np.testing.assert_array_equal(np.asarray(a).view(np.uint8), np.asarray(b).view(np.uint8))
        rows = [np.array([0, n_old - 1, n_old, n - 1], np.int32)] * 4
        for x, y in zip(dv.rerank_scores(queries, rows, 1), whole_dv.rerank_scores(queries, rows, 1)):
            np.testing.assert_array_equal(canon64(x), canon64(y))
        with pytest.raises(B.BBQError) as e:
            dv.append(base[:3, :50])
        assert e.value.code == capi.ERR_DIM_MISMATCH
    finally:
        for h in (ix, dv, whole_ix, whole_dv):
            h.close()


# ------------------------------------------------------------------------------------------------ 10. scope

def test_scope_and_root_shard():
    import torch
    sim, dim, n_old, n = 1, 64, 3000, 5000
    base = O.mulberry32(121, n * dim).reshape(n, dim)
    codes, corr, cen = O.build_index(base, sim)
    cdp = O.centroid_dp(cen)
    f = np.ascontiguousarray(base[n_old:])
    L = capi.lib()

    def refused(ix, want):
        assert L.bbq_index_append_rows(ix._h, codes[n_old:].ctypes.data, corr[n_old:].ctypes.data, n - n_old) == want
        assert L.bbq_index_append(ix._h, f.ctypes.data, n - n_old, cen.ctypes.data, sim, 0.1, 5, None, None, None, None) == want
        assert L.bbq_index_reserve(ix._h, n) == want
        assert L.bbq_index_size(ix._h) == n_old

    multi = B.Index.create_multi(codes[:n_old], corr[:n_old], dim, cdp, [0, 0], pilot_rows=1024)
    shard = B.Index(codes[1024:1024 + n_old], corr[1024:1024 + n_old], dim, cdp, row_base=1024)
    pilot = B.Index(codes[1024:1024 + n_old], corr[1024:1024 + n_old], dim, cdp, row_base=1024, pilot_codes=codes[:1024], pilot_corr=corr[:1024])
    root = B.Index(codes[:n_old], corr[:n_old], dim, cdp, row_base=0)
    try:
        for ix in (multi, shard, pilot):
            refused(ix, capi.ERR_UNSUPPORTED)
        with pytest.raises(B.BBQError) as e:              # a wrong dimension
            root.append_rows(codes[n_old:, :7], corr[n_old:])
        assert e.value.code == capi.ERR_DIM_MISMATCH
        with pytest.raises(B.BBQError) as e:
            root.append(base[n_old:, :32], cen[:32], sim)
        assert e.value.code == capi.ERR_DIM_MISMATCH
        assert L.bbq_index_append(root._h, f.ctypes.data, n - n_old, cen.ctypes.data, 3, 0.1, 5, None, None, None, None) == capi.ERR_INVALID_ARG
        assert root.n == n_old
        # a root shard: an un-waited batch refuses the append, a waited one does not; the scan after it equals the oracle
        orc = Oracle(codes, corr, dim, cen, sim, 4, O.mulberry32(122, 5 * dim).reshape(5, dim))
        k, nq = 10, 5
        cap = int(root.shard_list_cap(k)) * nq
        d_packed = torch.zeros(cap, dtype=torch.int64, device="cuda")
        d_off = torch.zeros(nq + 1, dtype=torch.int64, device="cuda")
        d_flags = torch.zeros(nq, dtype=torch.int32, device="cuda")
        root.shard_scan_begin(orc.qq, orc.qc, 4, sim, k, d_packed.data_ptr(), cap, d_off.data_ptr(), d_flags.data_ptr())
        refused(root, capi.ERR_INVALID_ARG)
        root.shard_scan_wait()
        root.append_rows(codes[n_old:4000], corr[n_old:4000])
        root.append(base[4000:], cen, sim, want_host_copy=False)
        assert root.n == n
        cap = int(root.shard_list_cap(k)) * nq
        d_packed = torch.zeros(cap, dtype=torch.int64, device="cuda")
        total = root.shard_scan(orc.qq, orc.qc, 4, sim, k, d_packed.data_ptr(), cap, d_off.data_ptr(), d_flags.data_ptr())
        assert int(d_flags.abs().sum().item()) == 0
        off = d_off.cpu().numpy()
        idx, sc, cnt = B.replay_batch([d_packed[:total].cpu().numpy().view(np.uint64)], [off], nq, n, k)
        for qi in range(nq):
            wi, ws = orc.topk(qi, k)
            np.testing.assert_array_equal(idx[qi, :cnt[qi]], wi)
            np.testing.assert_array_equal(canon32(sc[qi, :cnt[qi]]), canon32(ws))
        root.shard_scan_begin(orc.qq, orc.qc, 4, sim, k, d_packed.data_ptr(), cap, d_off.data_ptr(), d_flags.data_ptr())
        assert root.shard_scan_wait() > 0
    finally:
        for ix in (multi, shard, pilot, root):
            ix.close()


# ------------------------------------------------------------------------------------------------ the Python mirror

@pytest.mark.parametrize("ib", [1, 2])
def test_api_append_vectors_on_the_device(ib):
    sim, dim = 1, 100
    a = O.mulberry32(131, 300 * dim).reshape(300, dim)
    b = O.mulberry32(132, 90 * dim).reshape(90, dim)
    q = O.mulberry32(133, dim)
    fmt = B.BinaryQuantizationFormat({"queryBits": 4, "indexBits": ib, "quantizer": {"similarityFunction": "COSINE", "lambda": 0.1, "iters": 5}})
    tv = fmt.quantizeVectors(list(a))["quantizedVectors"]
    assert fmt.appendVectors(tv, list(b)) is tv and tv.size() == 390
    acodes, acorr, cen = O.build_index(a, sim, ib=ib)
    bcodes, bcorr = oracle_rows(b, cen, sim, ib)
    allc, allr = np.concatenate([acodes, bcodes]), np.concatenate([acorr, bcorr])
    for ord_ in (0, 299, 300, 389):
        np.testing.assert_array_equal(tv.vectorValue(ord_), allc[ord_])
        t = tv.getCorrectiveTerms(ord_)
        got = np.array([t["lowerInterval"], t["upperInterval"], t["additionalCorrection"], t["quantizedComponentSum"]])
        np.testing.assert_array_equal(canon64(got), canon64(allr[ord_]))
    wi, ws = O.search(q, allc, allr, cen, sim, 4, 25, ib=ib)
    got = fmt.searchNearestNeighbors(q, tv, 25)
    assert [r["index"] for r in got] == list(wi)
    np.testing.assert_array_equal(canon32([r["score"] for r in got]), canon32(ws))
    bad = b[:4].copy()
    bad[2, 5] = np.inf
    with pytest.raises(Exception, match="向量 2 位置 5 包含NaN值"):   # COSINE: Infinity / Infinity
        fmt.appendVectors(tv, list(bad))
    assert tv.size() == 390 and tv._device().n == 390
