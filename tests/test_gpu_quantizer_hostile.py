"""GPU: bbq_quantize1_kernel - the one kernel behind bbq_index_build*, bbq_index_append and bbq_index_update - on the hostile rows and
parameters of tests/quant_hostile.py, through every path that launches it: the build, the 1-bit append straight into the tile records
(row0 > 0, padding lanes), the staged 1-bit path (scratch tile set + untile) and the staged multi-bit path.  Expected values come from
the ORACLE only (orc_build_index*, the per-row recipe of tests/append_recipe.py, orc_score_all*, the reference heap); what the batches
reach - every exit of optimizeIntervals, NaN intervals, non-finite scale and centroid, f32 overflow and denormals - is asserted on the
CPU in tests/test_quantizer_hostile_cpu.py.  Bit-exact through canon32 / canon64 (JS has one NaN); no tolerances."""
import functools

import numpy as np
import pytest

import orclib as O
import quant_hostile as Q
from append_recipe import oracle_rows
from bbqlib import bbq_amd as B
from quant_hostile import canon32, canon64
from test_gpu_append import check_export, file_bytes, make_index
from test_gpu_update import EDGES, duplicates_of, needs_sums

pytestmark = pytest.mark.gpu

SHAPES = [(name, n, dim) for name in Q.BATCHES for n in Q.NS for dim in Q.DIMS]
SIMS = (0, 1, 2)
ONE_BIT = [(lam, iters) for ib, lam, iters in Q.GRID if ib == 1]          # the 1-bit points of the grid, for append and update
MULTI_BIT = [(ib, lam, iters) for ib, lam, iters in Q.GRID if ib in (2, 8)]
QBS = (4, 1)                                                              # the first query is scored as a 4-bit query, the second as a 1-bit one
N_OLD = 65                                                                # benign rows the appended-to indexes are cut from


def _ids(shape):
    return "-".join(str(s) for s in shape)


class Expected:
    """the oracle's answers over one row set for two queries: (qq, qc, qb, (qcdist, score64, score32)) each"""

    def __init__(self, codes, corr, cen, sim, ib, lam, iters, queries):
        dim = cen.shape[0]
        cdp = O.centroid_dp(cen)
        self.sim, self.n, self.q = sim, codes.shape[0], []
        for q, qb in zip(queries, QBS):
            qq, qc = O.quantize_query(q, cen, sim, qb, lam, iters)
            self.q.append((qq, qc, qb, O.score_all(codes, corr, dim, qq, qc, qb, sim, cdp, ib)))

    def check_score_rows(self, ix, msg):
        for qi, (qq, qc, qb, (od, os64, os32)) in enumerate(self.q):
            d, s64, s32 = ix.score_rows(qq, qc, qb, self.sim)
            np.testing.assert_array_equal(d, od, err_msg="%s q%d qcDist" % (msg, qi))
            np.testing.assert_array_equal(canon64(s64), canon64(os64), err_msg="%s q%d f64 scores" % (msg, qi))
            np.testing.assert_array_equal(canon32(s32), canon32(os32), err_msg="%s q%d f32 scores" % (msg, qi))

    def check_search(self, ix, ks, msg):
        for qi, (qq, qc, qb, (_, _, os32)) in enumerate(self.q):
            for k in ks:
                wi, ws = O.heap_topk(os32, k)
                idx, sc = ix.search(qq, qc, qb, self.sim, k)
                np.testing.assert_array_equal(idx, wi, err_msg="%s q%d k=%d" % (msg, qi, k))
                np.testing.assert_array_equal(canon32(sc), canon32(ws), err_msg="%s q%d k=%d" % (msg, qi, k))


# ------------------------------------------------------------------------------------------------ 1. build

@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_build_hostile(shape):
    name, n, dim = shape
    rows = Q.batch(name, n, dim)
    queries = Q.queries(name, n, dim)
    for sim in SIMS:
        for ib, lam, iters in Q.GRID:
            ocodes, ocorr, ocen = Q.oracle_build(name, n, dim, sim, ib, lam, iters)
            exp = Expected(ocodes, ocorr, ocen, sim, ib, lam, iters, queries)
            for layout in ("compact", "inline"):
                msg = "%s sim=%d ib=%d lambda=%g iters=%d %s" % (_ids(shape), sim, ib, lam, iters, layout)
                ix, codes, corr, cen = B.Index.build(rows, sim, lam, iters, index_bits=ib, corrections=layout)
                try:
                    np.testing.assert_array_equal(canon32(cen), canon32(ocen), err_msg=msg + " centroid")
                    np.testing.assert_array_equal(codes, ocodes, err_msg=msg + " codes")
                    np.testing.assert_array_equal(canon64(corr), canon64(ocorr), err_msg=msg + " corrections")
                    check_export(ix, ocodes, ocorr, msg + " export")
                    exp.check_score_rows(ix, msg)
                    if name in ("mixed", "extreme"):
                        exp.check_search(ix, (1, 10, n), msg)
                finally:
                    ix.close()


# ------------------------------------------------------------------------------------------------ 2. append, 1 bit, straight into the tiles

@functools.lru_cache(maxsize=None)
def old_rows(dim, sim, ib, lam, iters):
    """N_OLD benign rows as the oracle builds them: what the appended-to and updated indexes are created from"""
    return O.build_index(Q.benign(N_OLD, dim), sim, lam, iters, ib)


@functools.lru_cache(maxsize=None)
def hostile_rows(name, dim, sim, ib, lam, iters):
    """the batch of 257 rows followed by the centroid itself, and the oracle's rows for them against that centroid"""
    cen = old_rows(dim, sim, ib, lam, iters)[2]
    rows = np.concatenate([Q.batch(name, 257, dim), cen[None, :]])
    return (rows,) + oracle_rows(rows, cen, sim, ib, lam, iters)


APPEND = [(name, dim) for name in Q.BATCHES for dim in Q.DIMS]


@pytest.mark.parametrize("r", [0, 1, 63, 64, 65])
@pytest.mark.parametrize("name,dim", APPEND)
def test_append_hostile_one_bit(name, dim, r):
    """r old rows (0: an empty index), then the hostile rows in two calls: the first starts at lane r % 64, the second inside a tile"""
    queries = np.stack([Q.batch(name, 257, dim)[1], Q.benign(1, dim, 1)[0]])
    for sim in SIMS:
        for lam, iters in ONE_BIT:
            acodes, acorr, cen = old_rows(dim, sim, 1, lam, iters)
            rows, wcodes, wcorr = hostile_rows(name, dim, sim, 1, lam, iters)
            allc, allr = np.concatenate([acodes[:r], wcodes]), np.concatenate([acorr[:r], wcorr])
            exp = Expected(allc, allr, cen, sim, 1, lam, iters, queries)
            for compact in (True, False):
                msg = "%s dim=%d r=%d sim=%d lambda=%g iters=%d compact=%s" % (name, dim, r, sim, lam, iters, compact)
                ix = make_index(acodes[:r], acorr[:r], dim, O.centroid_dp(cen), compact)
                try:
                    cut = 100
                    assert (r + cut) % 64 != 0
                    got1 = ix.append(rows[:cut], cen, sim, lam, iters)
                    got2 = ix.append(rows[cut:], cen, sim, lam, iters)
                    assert ix.n == r + len(rows)
                    np.testing.assert_array_equal(np.concatenate([got1[0], got2[0]]), wcodes, err_msg=msg + " codes")
                    np.testing.assert_array_equal(canon64(np.concatenate([got1[1], got2[1]])), canon64(wcorr), err_msg=msg + " corrections")
                    check_export(ix, allc, allr, msg + " export")
                    exp.check_score_rows(ix, msg)
                finally:
                    ix.close()


# ------------------------------------------------------------------------------------------------ 3. the staged paths

def _update_ords(n, count):
    """tile edges, one ord named three times, then other ords until every hostile row has a place"""
    head = [e for e in EDGES if e < n] + duplicates_of(n)
    rest = [int(o) for o in np.random.default_rng(8300 + n).permutation(n) if o not in head]
    return np.array(head + rest[:count - len(head)], np.int64)


@functools.lru_cache(maxsize=None)
def staged_inputs(name, dim, sim, ib, lam, iters):
    """601 benign rows as the oracle builds them, the hostile rows (the batch of 257, then the centroid itself) and the oracle's rows for
    them against that centroid"""
    bcodes, bcorr, cen = O.build_index(Q.benign(601, dim), sim, lam, iters, ib)
    rows = np.concatenate([Q.batch(name, 257, dim), cen[None, :]])
    return (bcodes, bcorr, cen, rows) + oracle_rows(rows, cen, sim, ib, lam, iters)


def _check_staged(name, dim, sim, ib, lam, iters, compact, explicit, tmp_path, queries):
    """update, then append, on an index of 601 benign rows (quantize_staged: every multi-bit index, and a 1-bit one with explicit
    component sums for the append; the update always); against the oracle over the updated set and a twin created whole"""
    bcodes, bcorr, cen, rows, wcodes, wcorr = staged_inputs(name, dim, sim, ib, lam, iters)
    n = len(bcodes)
    ords = _update_ords(n, len(rows))
    assert len(ords) == len(rows) and ords[0] == 63
    if explicit:
        bcorr = bcorr.copy()         # a sum that is not the implied one, in a row that stays: the index stores the sums and takes any row
        bcorr[min(set(range(n)) - set(ords.tolist())), 3] += 2.0
    codes, corr = bcodes.copy(), bcorr.copy()
    for i, o in enumerate(ords):     # applied in order: the last of equal ords wins
        codes[o], corr[o] = wcodes[i], wcorr[i]
    allc, allr = np.concatenate([codes, wcodes]), np.concatenate([corr, wcorr])
    msg = "%s dim=%d sim=%d ib=%d lambda=%g iters=%d compact=%s explicit=%s" % (name, dim, sim, ib, lam, iters, compact, explicit)
    cdp = O.centroid_dp(cen)
    ix = make_index(bcodes, bcorr, dim, cdp, compact, ib)
    twin = None
    try:
        ucodes, ucorr = ix.update(ords, rows, cen, sim, lam, iters)
        np.testing.assert_array_equal(ucodes, wcodes, err_msg=msg + " update codes")
        np.testing.assert_array_equal(canon64(ucorr), canon64(wcorr), err_msg=msg + " update corrections")
        check_export(ix, codes, corr, msg + " updated")
        Expected(codes, corr, cen, sim, ib, lam, iters, queries).check_score_rows(ix, msg + " updated")
        acodes, acorr = ix.append(rows, cen, sim, lam, iters)
        np.testing.assert_array_equal(acodes, wcodes, err_msg=msg + " append codes")
        np.testing.assert_array_equal(canon64(acorr), canon64(wcorr), err_msg=msg + " append corrections")
        check_export(ix, allc, allr, msg + " appended")
        exp = Expected(allc, allr, cen, sim, ib, lam, iters, queries)
        exp.check_score_rows(ix, msg + " appended")
        # the twin is created whole from the rows as the device made them (they are the oracle's up to the bits of a NaN, which a file keeps)
        tcodes, tcorr = bcodes.copy(), bcorr.copy()
        for i, o in enumerate(ords):
            tcodes[o], tcorr[o] = ucodes[i], ucorr[i]
        twin = make_index(np.concatenate([tcodes, acodes]), np.concatenate([tcorr, acorr]), dim, cdp, compact, ib)
        exp.check_score_rows(twin, msg + " twin")
        assert ix.bytes_per_row == twin.bytes_per_row, msg
        assert file_bytes(ix, str(tmp_path / "grown"), cen, sim) == file_bytes(twin, str(tmp_path / "twin"), cen, sim), msg
    finally:
        ix.close()
        if twin is not None:
            twin.close()


@pytest.mark.parametrize("explicit", [False, True])
@pytest.mark.parametrize("name,dim", APPEND)
def test_staged_hostile_one_bit(name, dim, explicit, tmp_path):
    """explicit: the index was created with explicit component sums (has_x1), so the append is staged as well as the update"""
    queries = np.stack([Q.batch(name, 257, dim)[1], Q.benign(1, dim, 1)[0]])
    for sim in SIMS:
        for lam, iters in ONE_BIT:
            for compact in (True, False):
                _check_staged(name, dim, sim, 1, lam, iters, compact, explicit, tmp_path, queries)


@pytest.mark.parametrize("ib,lam,iters", MULTI_BIT)
@pytest.mark.parametrize("name,dim", [(name, dim) for name in ("mixed", "extreme") for dim in Q.DIMS if dim > 1])
def test_staged_hostile_multi_bit(name, dim, ib, lam, iters, tmp_path):
    """(dimension 1 only with 1-bit rows: a multi-bit index of dimension 1 is stored as packed 1-bit rows, tests/test_gpu_append.py)
    A row with NaN intervals has a NaN component sum, which is not its code sum: such rows need an index that stores the sums."""
    queries = np.stack([Q.batch(name, 257, dim)[1], Q.benign(1, dim, 1)[0]])
    for sim in SIMS:
        explicit = needs_sums(*staged_inputs(name, dim, sim, ib, lam, iters)[4:], ib)
        for compact in (True, False):
            _check_staged(name, dim, sim, ib, lam, iters, compact, explicit, tmp_path, queries)
