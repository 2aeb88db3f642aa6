"""CPU: the quantizer on hostile rows and parameters (tests/quant_hostile.py).
  1. the oracle's traced entry (orc_scalar_quantize_trace) gives the bytes of the untraced one
  2. the batches provably arrive where they are aimed: every way optimizeIntervals can end is taken by enough rows
  3. the host quantizer (bbq_quantize_vectors, bbq_quantize_query) equals the oracle on all of it, bit for bit
  4. the oracle itself is pinned to the reference on such rows (tests/golden/quant_hostile_*.json, recorded by running it)
Exit-class counts as measured (mixed, n = 601, rows summed over the grid and the three similarity functions):
  dim   ran out/0  ran out/>=1  determinant  converged/>=1  rose/0  rose/>=1  NaN loss
   13      1803        793         2092          4214        5398     124       678
   64      1803       2228         2008          2606        5448     331       548
  131      1803       2345         1964          2328        5546     438       484
extreme at (1, 0.1, 5) under EUCLIDEAN, dim > 1: 67-315 determinant exits and 17-199 NaN rows; overflow: every row NaN; identical:
every row leaves at the non-finite scale.
"""
import numpy as np
import pytest

import orclib as O
import quant_hostile as Q
from bbqlib import bbq_amd as B
from quant_hostile import canon64

SHAPES = [(name, n, dim) for name in Q.BATCHES for n in Q.NS for dim in Q.DIMS]
FLOOR = 16


def _ids(shape):
    return "%s-%dx%d" % shape


# ---------------------------------------------------------------- 1. one body, two entries

@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_traced_oracle_equals_untraced(shape):
    name, n, dim = shape
    for sn in Q.SIM_NAMES:
        sim = O.SIMS[sn]
        for ib, lam, iters in Q.GRID:
            codes, corr, cen = Q.oracle_build(name, n, dim, sim, ib, lam, iters)
            tcodes, tcorr, trace = Q.traced(name, n, dim, sim, ib, lam, iters)
            msg = "%s %s ib=%d lambda=%g iters=%d" % (_ids(shape), sn, ib, lam, iters)
            assert tcodes.tobytes() == codes.tobytes(), msg
            assert tcorr.tobytes() == corr.tobytes(), msg
            assert ((trace[:, 0] >= 0) & (trace[:, 0] <= 4) & (trace[:, 1] >= 0) & (trace[:, 1] <= iters)).all(), msg
            if iters == 0:
                assert np.isin(trace[:, 0], (Q.EXIT_ITERS, Q.EXIT_SCALE)).all() and not trace[:, 1:].any(), msg


# ---------------------------------------------------------------- 2. reach conditions

@pytest.mark.parametrize("dim", [13, 64, 131])
def test_mixed_reaches_every_exit(dim):
    """over the grid and the three similarity functions, each way of ending has at least FLOOR rows"""
    rows, total = [], np.zeros(len(Q.CLASSES), np.int64)
    for sn in Q.SIM_NAMES:
        for ib, lam, iters in Q.GRID:
            _, corr, trace = Q.traced("mixed", 601, dim, O.SIMS[sn], ib, lam, iters)
            cnt = Q.classify(trace, corr)
            rows.append(("%s ib=%d lambda=%g iters=%d" % (sn, ib, lam, iters), cnt))
            total += cnt
    rows.append(("all of mixed 601x%d" % dim, total))
    text = Q.table(rows)
    print(text)
    assert (total[:7] >= FLOOR).all(), "\n" + text


@pytest.mark.parametrize("shape", [s for s in SHAPES if s[0] != "mixed"], ids=_ids)
def test_other_batches_arrive(shape):
    name, n, dim = shape
    rows = []
    for sn in ("EUCLIDEAN", "MAXIMUM_INNER_PRODUCT"):
        sim = O.SIMS[sn]
        cen = Q.oracle_build(name, n, dim, sim, 1, 0.1, 5)[2]
        _, corr, trace = Q.traced(name, n, dim, sim, 1, 0.1, 5)
        cnt = Q.classify(trace, corr)
        rows.append(("%s %s ib=1 lambda=0.1 iters=5" % (_ids(shape), sn), cnt))
        text = Q.table(rows)
        if name == "identical":      # the centroid is the row: a zero centred vector, scale = 0.9 / 0
            np.testing.assert_array_equal(cen, Q.batch(name, n, dim)[0])
            assert (trace[:, 0] == Q.EXIT_SCALE).all(), "\n" + text
        elif name == "overflow":     # the f32 centroid sum overflows, and with it every centred value
            assert not np.isfinite(cen).all() and np.isnan(corr).any(axis=1).all(), "\n" + text
        elif sn == "EUCLIDEAN":      # extreme
            assert cnt[9] >= FLOOR, "\n" + text
            # (a row of one dimension has a zero-width interval and a NaN step from the start: no determinant is ever computed)
            assert dim == 1 or cnt[2] >= FLOOR, "\n" + text
    print(Q.table(rows))
    if name == "overflow":   # COSINE rows are normalised first: nothing overflows
        _, ccorr, ccen = Q.oracle_build(name, n, dim, O.SIMS["COSINE"], 1, 0.1, 5)
        assert np.isfinite(ccen).all() and np.isfinite(ccorr[:, 2:]).all()


# ---------------------------------------------------------------- 3. the host quantizer

@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_host_quantizer_equals_oracle(shape):
    name, n, dim = shape
    rows = Q.batch(name, n, dim)
    qs = Q.queries(name, n, dim)
    for sn in Q.SIM_NAMES:
        sim = O.SIMS[sn]
        for ib, lam, iters in Q.GRID:
            msg = "%s %s ib=%d lambda=%g iters=%d" % (_ids(shape), sn, ib, lam, iters)
            ocodes, ocorr, ocen = Q.oracle_build(name, n, dim, sim, ib, lam, iters)
            codes, corr, cen = B.quantize_vectors(rows, sim, ib, lam, iters, n_threads=3)
            np.testing.assert_array_equal(Q.canon32(cen), Q.canon32(ocen), err_msg=msg)
            np.testing.assert_array_equal(codes, ocodes, err_msg=msg)
            np.testing.assert_array_equal(canon64(corr), canon64(ocorr), err_msg=msg)
            for qb in (1, 2, 4, 8):
                for q in qs:
                    oq, oc = O.quantize_query(q, ocen, sim, qb, lam, iters)
                    qq, qc = B.quantize_query(q, ocen, sim, qb, lam, iters)
                    np.testing.assert_array_equal(qq, oq, err_msg=msg + " qb=%d" % qb)
                    np.testing.assert_array_equal(canon64(qc), canon64(oc), err_msg=msg + " qb=%d" % qb)


# ---------------------------------------------------------------- 4. the reference pin

PINNED = O.golden_names("quant_hostile_*")


def test_reference_pin_covers_every_exit():
    """the rows recorded from the reference take every exit between them, and some carry NaN corrections"""
    assert len(PINNED) == 12
    total, rows = np.zeros(len(Q.CLASSES), np.int64), []
    for name in PINNED:
        g = O.load_golden(name)
        base, _ = O.golden_inputs(g)
        assert base.shape == (48, 13) and g["full"]
        sim = O.SIMS[g["sim"]]
        cen = O.build_index(base, sim, g["lambda"], g["iters"], g["ib"])[2]
        _, corr, trace = O.quantize_trace(base, cen, sim, g["ib"], g["lambda"], g["iters"])
        cnt = Q.classify(trace, corr)
        rows.append((name, cnt))
        total += cnt
    text = Q.table(rows)
    print(text)
    # the five exits (ran out, non-finite scale, determinant, converged, loss rose), accepted steps, NaN losses and NaN corrections
    exits = [total[0] + total[1], total[7], total[2], total[3] + total[8], total[4] + total[5]]
    assert all(exits) and total[1] + total[3] + total[5] > 0 and total[6] > 0 and total[9] > 0, "\n" + text
    assert {(g["sim"], g["ib"], g["lambda"], g["iters"]) for g in map(O.load_golden, PINNED)} == \
        {(s, ib, lam, it) for s in Q.SIM_NAMES for ib, lam, it in ((1, 0, 5), (1, 1, 5), (2, 0.1, 0), (4, 1, 3))}


@pytest.mark.parametrize("name", PINNED)
def test_oracle_reproduces_the_reference_on_hostile_rows(name):
    """centroid, codes and corrections as the reference computed them, bit for bit (NaNs canonicalised: JS has one NaN)"""
    g = O.load_golden(name)
    base, _ = O.golden_inputs(g)
    codes, corr, cen = O.build_index(base, O.SIMS[g["sim"]], g["lambda"], g["iters"], g["ib"])
    np.testing.assert_array_equal(Q.canon32(cen), Q.canon32(O.dec(g["centroid_f32"], "<f4")))
    np.testing.assert_array_equal(codes.ravel(), O.dec(g["codes_u8"], "u1"))
    np.testing.assert_array_equal(canon64(corr.ravel()), canon64(O.dec(g["corr_f64"], "<f8")))
