"""CPU: the compact layout's score bound as the RANGE call uses it (bbq_range_kernels.hip: compact_bound_passes in front of the exact
score, with nothing behind it - a row the bound wrongly rejects is missing from the answer), over the hostile recipe of
tests/range_hostile.py, for the keys bbq_range_key makes of any f32 a caller likes.

The model is the numpy restatement the sweep's bound already has - upper_bound (test_bound_math_cpu.py), images / bound_z / z_image
(test_bound_f32_cpu.py), range_answer (test_range_key_cpu.py) - plus what the range kernel puts around it: the tile's additive end
(tile_add_bound over bbq_tile_add_range_kernel's {min, max} as f32, both NaN where a row's is NaN) and the f64 form's verdict
(f64_bound_passes: the bound as f32, NaN passes, else its key against the range key).

Dominance: every row in the oracle's answer passes both forms, for every threshold of the table - rows scoring +0 included, which
test_bound_f32_cpu.py leaves out.  The recipe's conditions: the inputs reach the bound, from the model and the oracle alone.  The z image
at the edge keys: -inf exactly where it must accept everything, otherwise finite and below the threshold's exact inversion and the z of
every row of the answer.  Every comparison is exact."""
import fractions
import functools

import numpy as np
import pytest

import range_hostile as H
from test_bound_math_cpu import FBS, bf16_trunc, upper_bound
from test_bound_f32_cpu import F32, NEG, bits_of_key, bound_z, images, key_of_bits, passes, z_f64, z_image
from test_range_key_cpu import range_answer
from bbqlib import bbq_amd as B

FLT_MAX = float(np.finfo(F32).max)
SUB = 2.0 ** -149
CASES = [(f, s) for f in H.FAMILIES for s in H.SIMS]
IDS = ["%s-%s" % (f.name, ("euc", "cos", "mip")[s]) for f, s in CASES]
WITH_IMAGES = (0, 1, 2, 3)      # the queries at the ordinary scale and x 30; queries 4 and 5 (x 1e60, x 1e-60) have no f32 images


def tile_add(add, sim):
    """per row, what tile_add_bound hands the bound: the f32 of the minimum (EUCLIDEAN) or maximum of additionalCorrection over the valid
    rows of the row's tile, NaN where one of them is NaN"""
    n = len(add)
    nt = -(-n // H.TILE)
    a = np.full(nt * H.TILE, np.nan)
    a[:n] = add
    a = a.reshape(nt, H.TILE)
    valid = (np.arange(nt * H.TILE) < n).reshape(nt, H.TILE)
    with np.errstate(all="ignore"):
        end = np.where(valid, a, np.inf).min(axis=1) if sim == 0 else np.where(valid, a, -np.inf).max(axis=1)
        end = np.where((valid & np.isnan(a)).any(axis=1), np.nan, end).astype(F32)
    return np.repeat(end, H.TILE)[:n]


def plain_of(fam):
    """MAXIMUM_INNER_PRODUCT undivided, centroidDP 0: the per-row scorer's form, which answers for multi-bit rows (queryBits 4 here)"""
    return fam.index_bits > 1


class Query:
    """the bound of one query over the family's rows: both forms, every row, ahead of any threshold"""

    def __init__(self, fam, sim, codes, corr, qc, d, s32):
        dim, ib = fam.dim, fam.index_bits
        self.sim, self.plain = sim, plain_of(fam)
        self.qadd, self.cdp = qc[2], (0.0 if self.plain else H.CDP)
        self.s32 = np.asarray(s32, F32)
        x1 = H.code_sums(codes, ib)
        ly = (qc[1] - qc[0]) * FBS
        aadd = tile_add(corr[:, 2], sim)
        with np.errstate(all="ignore"):      # (1e300 has no f32)
            al, au = bf16_trunc(corr[:, 0]), bf16_trunc(corr[:, 1])
            u32 = upper_bound(np.asarray(d, np.float64), al, au, aadd.astype(np.float64), x1, qc[0], ly, qc[3], qc[2], self.cdp, float(dim), sim,
                              self.plain).astype(F32)
        self.ub_nan, self.ub_key = np.isnan(u32), key_of_bits(u32.view(np.uint32))
        vmax = (1 << ib) - 1
        self.im = images(qc[0], ly, qc[3], float(dim), sim, dim * vmax, dim * vmax * 15)
        self.zup = None if self.im is None else {fused: bound_z(np.asarray(d), al, au, aadd, x1, self.im, fused) for fused in (True, False)}
        # the row's own z from its exact corrections, in extended precision: z = cs s + ca add (bbq_kernel_common.h, z_threshold)
        L = np.longdouble
        with np.errstate(all="ignore"):
            lo, lx = corr[:, 0].astype(L), corr[:, 1].astype(L) - corr[:, 0].astype(L)
            s = lo * L(qc[0]) * L(dim) + L(qc[0]) * lx * x1.astype(L) + lo * L(ly) * L(qc[3]) + lx * L(ly) * np.asarray(d).astype(L)
            self.z_row = 2 * s - corr[:, 2].astype(L) if sim == 0 else s + corr[:, 2].astype(L)

    def in_answer(self, t):
        m = np.zeros(len(self.s32), bool)
        m[range_answer(self.s32, t)] = True
        return m

    def passes_f64(self, key):
        """f64_bound_passes"""
        return self.ub_nan | (self.ub_key > np.uint32(key))

    def zth(self, key):
        return z_image(np.array([key], np.uint32), self.qadd, self.cdp, self.sim, self.plain)[0]

    def passes_f32(self, key, fused=True):
        """fast_bound_passes"""
        return passes(self.zup[fused], self.zth(key))

    def passes_default(self, key):
        """compact_bound_passes under the default options: the f32 form where the query has images"""
        return self.passes_f64(key) if self.im is None else self.passes_f32(key)


@functools.lru_cache(maxsize=None)
def model(fam, sim):
    codes, corr = H.rows(fam)
    qq, qc = H.queries(fam, sim)
    return tuple(Query(fam, sim, codes, corr, qc[q], s[0], s[2]) for q, s in enumerate(H.scores(fam, sim)))


@functools.lru_cache(maxsize=None)
def table(fam, sim, q):
    """[(threshold, range key)] of one query"""
    return tuple((t, B.range_key(t)) for t in H.thresholds_of(H.scores(fam, sim)[q][2]))


def rows_of_kind(fam, *kinds):
    m = np.zeros(fam.n, bool)
    for t, k in enumerate(H.tile_kinds(fam)):
        if k in kinds:
            m[H.tile_rows(fam, t)] = True
    return m


# ---- the recipe is what it says ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fam", H.FAMILIES, ids=[f.name for f in H.FAMILIES])
def test_recipe_layout(fam):
    kinds = H.tile_kinds(fam)
    codes, corr = H.rows(fam)
    assert len(kinds) == -(-fam.n // H.TILE) and fam.n > 2 * H.CHUNK and fam.n % H.TILE
    assert {"ordinary", "hostile", "mixed", "last"} | set(H.PLANTED) <= set(kinds)
    for kind, v in H.ADD_PLANTS.items():
        r = H.tile_rows(fam, H.tile_of(fam, kind))
        special = ~np.isfinite(corr[r, 2]) | (np.abs(corr[r, 2]) > 1.0)
        assert special.sum() == 1 and special[H.PLANT_LANE] and np.array_equal(corr[r[H.PLANT_LANE], 2], v, equal_nan=True)
    r = H.tile_rows(fam, H.tile_of(fam, "lu_nonfinite"))
    assert (~np.isfinite(corr[r, :2]) | (np.abs(corr[r, :2]) > 1.0)).sum() == 4
    for t, k in enumerate(kinds):
        r = H.tile_rows(fam, t)
        if k == "ordinary":
            assert (np.abs(corr[r, :2]) < 0.05).all() and (np.abs(corr[r, 2]) <= 1e-4).all() and (corr[r, 0] < corr[r, 1]).all()
    last = H.tile_rows(fam, len(kinds) - 1)
    assert last[-1] == fam.n - 1 and (len(last) == 1 or np.abs(corr[last[:-1], :2]).max() < 0.05)
    hostile_row = H._hostile_rows(H._seed(fam) + 7, fam.n, fam)[1][fam.n - 1]
    assert (corr[fam.n - 1] == hostile_row).all()
    qq, qc = H.queries(fam, 1)
    for sim in H.SIMS:
        m = model(fam, sim)
        assert [x.im is not None for x in m] == [True, True, True, True, False, False]     # two queries of six keep the f64 bound
        nt = [len(table(fam, sim, q)) for q in range(6)]
        assert all(len(H.FIXED) <= c <= len(H.FIXED) + 21 for c in nt)
        _, _, ths, who = H.pairs(fam, sim)
        assert len(ths) == sum(nt) == len(who) and len(ths) < 1024 and not np.isnan(ths).any()


# ---- dominance ----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def tally(fam, sim):
    """over every (row, threshold) pair of the family's table: how many the bound rejected, how many passed it and failed the exact
    test, how many are in the answer - under the default options and with fast_bound 0; and the in-answer rows scoring +0"""
    out = dict(pairs=0, rejected=0, passed_not_in=0, in_answer=0, rejected_f64=0, passed_not_in_f64=0, zero_rows_in_answer=0)
    for q, m in enumerate(model(fam, sim)):
        valid = ~np.isnan(m.s32)                 # a NaN-scored row is in no answer whatever the bound says
        for t, key in table(fam, sim, q):
            ans = m.in_answer(t)
            for name, p in (("", m.passes_default(key)), ("_f64", m.passes_f64(key))):
                out["rejected" + name] += int((~p).sum())
                out["passed_not_in" + name] += int((p & ~ans).sum())
            out["pairs"] += fam.n
            out["in_answer"] += int(ans.sum())
            out["zero_rows_in_answer"] += int((ans & (m.s32.view(np.uint32) == 0)).sum())
            assert not (ans & ~valid).any()
    return out


@pytest.mark.parametrize("fam,sim", CASES, ids=IDS)
def test_every_row_of_the_answer_passes_the_bound(fam, sim):
    for q, m in enumerate(model(fam, sim)):
        for t, key in table(fam, sim, q):
            ans = m.in_answer(t)
            where = "%s sim %d query %d threshold %r (key %#x)" % (fam.name, sim, q, t, key)
            lost = ans & ~m.passes_f64(key)
            assert not lost.any(), "%s: the f64 form rejects %d rows of the answer, first row %d" % (where, lost.sum(), np.flatnonzero(lost)[0])
            if m.im is None:
                continue
            zth = m.zth(key)
            for fused in (True, False):
                for z in (zth, np.nextafter(zth, F32(-np.inf))):
                    lost = ans & ~passes(m.zup[fused], z)
                    assert not lost.any(), "%s: the f32 form (fused %s, image %r) rejects %d rows of the answer, first row %d" % (
                        where, fused, z, lost.sum(), np.flatnonzero(lost)[0])
    c = tally(fam, sim)
    assert c["in_answer"] > 0 and (sim == 2 or c["zero_rows_in_answer"] > 0)      # (a MIP score is +0 only where its f32 underflows)


# ---- the inputs exercise the bound --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fam,sim", CASES, ids=IDS)
def test_the_inputs_reach_the_bound(fam, sim):
    ms = model(fam, sim)
    ordinary = rows_of_kind(fam, "ordinary")
    assert ordinary.sum() >= 4 * H.TILE
    # at the query's third-best score the bound rejects more than half of the rows of the ordinary-only tiles, in each form the query
    # has.  (All but query 4: x 1e60 a row's f32 score is +inf or - clamped, or underflowed - 0, so its third-best finite score is 0, a
    # threshold that accepts everything.  Query 5, x 1e-60, keeps the f64 form in the launch with a bound that bites.)
    for q in (0, 1, 2, 3, 5):
        key = B.range_key(H.own_thresholds(ms[q].s32)["third"])
        forms = [("f64", ms[q].passes_f64(key))]
        if q in WITH_IMAGES:
            forms += [("f32", ms[q].passes_f32(key)), ("f32 unfused", ms[q].passes_f32(key, False))]
        for form, p in forms:
            assert (~p[ordinary]).sum() > ordinary.sum() / 2, "query %d, %s form: %d of %d" % (q, form, (~p[ordinary]).sum(), ordinary.sum())
    c = tally(fam, sim)
    assert c["passed_not_in"] > 0 and c["passed_not_in_f64"] > 0 and c["rejected"] > 0 and c["rejected_f64"] > 0
    # a tile whose additive end - the one this similarity reads: the minimum under EUCLIDEAN, else the maximum - is NaN or infinite as
    # f32 rejects nothing.  (The other end of an infinite tile is an ordinary value: there the bound holds and rejects, as it should.)
    open_kinds = ("add_nan", "add_ninf") if sim == 0 else ("add_nan", "add_pinf", "add_1e300")
    open_rows = rows_of_kind(fam, *open_kinds)
    assert open_rows.sum() == len(open_kinds) * H.TILE
    other_rows = rows_of_kind(fam, *(set(H.ADD_PLANTS) - set(open_kinds)))
    rejected_elsewhere = 0
    for q, m in enumerate(ms):
        for t, key in table(fam, sim, q):
            forms = [m.passes_f64(key)] + ([] if m.im is None else [m.passes_f32(key), m.passes_f32(key, False)])
            for p in forms:
                assert p[open_rows].all(), "query %d threshold %r" % (q, t)
                rejected_elsewhere += int((~p[other_rows]).sum())
    assert rejected_elsewhere > 0
    # the oracle shows: +0 (EUCLIDEAN, COSINE), +inf or above 1e30, NaN; and an in-answer row in every planted tile above -inf
    s = np.stack([m.s32 for m in ms])
    if sim != 2:
        assert (s.view(np.uint32) == 0).any()
    with np.errstate(invalid="ignore"):
        assert (s > 1e30).any() and np.isnan(s).any()
    for kind in H.PLANTED:
        r = rows_of_kind(fam, kind)
        assert any((m.in_answer(t) & r).any() for q, m in enumerate(ms) for t, _ in table(fam, sim, q) if t > -np.inf), kind
    if sim == 0:
        assert ms[0].s32[H.EUC_INF_ROW] == np.inf      # the planted row: 1 + e is exactly 0


@pytest.mark.parametrize("sim", H.SIMS)
def test_the_update_flips_its_two_tiles(sim):
    """H.update: the ordinary tile that receives additionalCorrection 1e300 rejected rows and, where the similarity reads the maximum,
    rejects none afterwards; the NaN-additive tile whose NaN row is replaced rejected none and rejects afterwards"""
    fam = H.BY_NAME["main"]
    ords, _, _, codes, corr = H.update(fam)
    qq, qc = H.queries(fam, sim)
    gets_1e300, loses_nan = (H.tile_rows(fam, o // H.TILE) for o in ords)
    rejected = {(when, tile): 0 for when in "ba" for tile in "xn"}
    for q, before in enumerate(model(fam, sim)):
        d, _, s32 = H.score(fam, codes, corr, qq[q], qc[q], sim)
        after = Query(fam, sim, codes, corr, qc[q], d, s32)
        for t in H.thresholds_of(s32):
            key = B.range_key(t)
            for when, m in (("b", before), ("a", after)):
                for p in [m.passes_f64(key)] + ([] if m.im is None else [m.passes_f32(key)]):
                    rejected[when, "x"] += int((~p[gets_1e300]).sum())
                    rejected[when, "n"] += int((~p[loses_nan]).sum())
            assert not (after.in_answer(t) & ~(after.passes_f64(key) & after.passes_default(key))).any()
    assert rejected["b", "x"] > 0 and rejected["b", "n"] == 0 and rejected["a", "n"] > 0
    assert (rejected["a", "x"] > 0) if sim == 0 else (rejected["a", "x"] == 0)


# ---- the z image at the edge keys -----------------------------------------------------------------------------------------------------
def exact_inversion(th, qadd, cdp, sim, plain):
    """the z at which the similarity transform, in exact arithmetic, gives exactly th (a positive float; under COSINE also 0): a rational"""
    Fr = fractions.Fraction
    th, off = Fr(float(th)), Fr(float(qadd)) - Fr(float(cdp))
    if sim == 1:
        return 2 * th - 1 - off
    if sim == 2:
        sc = Fr(1) if plain else Fr(FBS)
        return ((th - 1) if th >= 1 else (1 - 1 / th)) * sc - off
    return Fr(float(qadd)) + 1 - 1 / th


@pytest.mark.parametrize("fam,sim", CASES, ids=IDS)
def test_z_image_at_the_edge_keys(fam, sim):
    """-inf (from -DBL_MAX) for range_key(-inf), every t <= 0 under COSINE and every t <= 2^-149 under EUCLIDEAN and both MIP forms
    (the 1-bit families divide by FOUR_BIT_SCALE, the multi-bit family does not); finite everywhere else, below the exact inversion of
    the float the key stands for and below the z of every row of the answer"""
    seen = {"open": 0, "finite": 0}
    for q, m in enumerate(model(fam, sim)):
        for t, key in table(fam, sim, q):
            where = "%s sim %d query %d threshold %r (key %#x)" % (fam.name, sim, q, t, key)
            z64 = float(z_f64(np.array([key], np.uint32), m.qadd, m.cdp, sim, m.plain)[0])
            zi = m.zth(key)
            if t == -np.inf or (t <= 0.0 if sim == 1 else t <= SUB):
                assert z64 == NEG and zi == -np.inf and np.signbit(zi), where
                seen["open"] += 1
                continue
            seen["finite"] += 1
            assert np.isfinite(z64) and np.isfinite(zi) and float(zi) <= z64, where
            th = bits_of_key(np.array([key], np.uint32)).view(F32)[0]
            with np.errstate(over="ignore"):      # (the float above FLT_MAX)
                assert (th > 0 or (sim == 1 and th == 0)) and th < t and np.nextafter(th, F32(np.inf)) == t, where
            assert fractions.Fraction(z64) < exact_inversion(th, m.qadd, m.cdp, sim, m.plain), where
            ans = m.in_answer(t)
            with np.errstate(invalid="ignore"):
                below = np.longdouble(zi) < m.z_row[ans]
            assert below.all(), "%s: the image %r is not below the z of row %d" % (where, zi, np.flatnonzero(ans)[~below][0])
    # of FIXED alone: -inf, -FLT_MAX, -1, -FLT_MIN, -2^-149 and both zeros are open, and +2^-149 except under COSINE
    assert seen["open"] >= 6 * (7 if sim == 1 else 8) and seen["finite"] >= 6 * 9


# ---- what the model counted -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sim", H.SIMS)
def test_report(sim):
    total = dict.fromkeys(tally(H.FAMILIES[0], sim), 0)
    for fam in H.FAMILIES:
        for k, v in tally(fam, sim).items():
            total[k] += v
    print("sim %d: %d (row, threshold) pairs - default options: rejected by the bound %d, passed it and failed the exact test %d; "
          "fast_bound 0: rejected %d, passed and failed %d; in the answer %d (scoring +0: %d)" % (
              sim, total["pairs"], total["rejected"], total["passed_not_in"], total["rejected_f64"], total["passed_not_in_f64"],
              total["in_answer"], total["zero_rows_in_answer"]))
    # every pair is rejected, in the answer, or passed in vain (a NaN-scored row that passed among them): the answer lost no row
    assert total["rejected"] + total["passed_not_in"] + total["in_answer"] == total["pairs"]
    assert total["rejected"] > total["pairs"] // 10 and total["in_answer"] > total["pairs"] // 10
