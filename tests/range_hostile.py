"""The hostile recipe of the range search tests: rows, queries and thresholds for bbq_count_range_batch / bbq_search_range_batch, whose
compact-layout score bound IS the answer (a row the bound rejects is missing: no heap replay, no dense fallback, no status) and whose
threshold is any f32 the caller likes.  Numpy, the CPU oracle and the host-only bbq_range_key: nothing here touches a device.
tests/test_range_hostile_cpu.py holds the recipe to its conditions and the bound's numpy model to the oracle over it;
tests/test_gpu_range_hostile.py runs it, bit for bit.

A family is (dim, index_bits, query_bits, n): the smallest shapes with more than one chunk of 512 rows, a partial last tile and each of
the range kernel's load arms.  The rows are laid out by tile (64 rows), so that the per-tile range of the additive correction
(add_range: {min, max} as f32, both NaN where a row's is NaN) takes every shape - see KINDS."""
import collections
import functools

import numpy as np

import orclib as O
from test_gpu_fast_bound import _hostile, _queries, _rows

F32 = np.float32
TILE, CHUNK = 64, 512
CDP = 0.0009
SIMS = (0, 1, 2)

Family = collections.namedtuple("Family", "name dim index_bits query_bits n")
FAMILIES = (Family("main", 96, 1, 4, 4 * 512 + 512 + 37),      # W = 1: four chunks, then a chunk, then a ragged tail tile
            Family("wide", 768, 1, 4, 1024 + 65),              # W = 6, the arm that reads row_sums
            Family("generic", 200, 1, 4, 1024 + 65),           # the run-time width
            Family("multibit", 64, 2, 4, 1024 + 65))           # code sums as x1
BY_NAME = {f.name: f for f in FAMILIES}

# what a full tile holds, in tile order; behind the 17 tiles every family has, the main family goes round CYCLE
#   ordinary      the corrections a real COSINE index shows (test_gpu_fast_bound._rows)
#   hostile       corrections over 1e-12 .. 1e6, zeros, upper < lower (test_gpu_fast_bound._hostile)
#   mixed         a seeded half of each
#   add_*         ordinary, and at lane PLANT_LANE a row whose additionalCorrection is NaN / +inf / -inf / 1e300
#   lu_nonfinite  ordinary, and at LU_LANES rows whose lower is NaN, upper +inf, lower -inf, upper 1e300
# The partial last tile ("last") is ordinary with a hostile row in its last valid lane.
KINDS = ("ordinary", "hostile", "mixed", "add_nan", "ordinary", "add_pinf", "hostile", "add_ninf", "mixed", "add_1e300", "ordinary",
         "lu_nonfinite", "hostile", "mixed", "ordinary", "ordinary", "hostile")
CYCLE = ("ordinary", "hostile", "mixed")
ADD_PLANTS = {"add_nan": np.nan, "add_pinf": np.inf, "add_ninf": -np.inf, "add_1e300": 1e300}
PLANT_LANE = 17
LU_LANES = ((5, 0, np.nan), (21, 1, np.inf), (40, 0, -np.inf), (59, 1, 1e300))      # (lane, column of corr, value)
EUC_INF_ROW = TILE + 33    # in tile 1 (hostile): zero intervals and the additionalCorrection that makes EUCLIDEAN query 0's 1 + e exactly 0: score +inf
PLANTED = tuple(ADD_PLANTS) + ("lu_nonfinite",)


def tile_kinds(fam):
    """the kind of every tile of the family, the partial last one included"""
    full = fam.n // TILE
    kinds = list(KINDS) + [CYCLE[i % 3] for i in range(full - len(KINDS))]
    assert fam.n % TILE and len(kinds) == full
    return tuple(kinds) + ("last",)


def tile_of(fam, kind):
    """the first tile of that kind"""
    return tile_kinds(fam).index(kind)


def tile_rows(fam, tile):
    return np.arange(tile * TILE, min((tile + 1) * TILE, fam.n))


def code_sums(codes, index_bits):
    return (np.unpackbits(codes, axis=1).sum(axis=1) if index_bits == 1 else codes.sum(axis=1, dtype=np.int64)).astype(np.float64)


# a family whose default seed misses a condition of tests/test_range_hostile_cpu.py gets another one here (multibit: under EUCLIDEAN the
# bound of a query x 30 rejected 66 of the 320 rows of the ordinary tiles at the query's third-best score, and more than half are asked)
SEEDS = {"multibit": 9132}


def _seed(fam):
    return SEEDS.get(fam.name, 9100 + 10 * FAMILIES.index(fam))


@functools.lru_cache(maxsize=None)
def queries(fam, sim):
    """six queries per similarity: two at the ordinary scale, two with the interval x 30, and one each x 1e60 and x 1e-60 - the last two
    have no f32 images (fast_bound_images refuses them), so they keep the f64 bound inside a launch whose other queries use the f32 form"""
    qq, qc = _queries(_seed(fam) + 1 + sim, 6, fam.dim, fam.query_bits)
    qc[2:4, :2] *= 30.0
    qc[4, :2] *= 1e60
    qc[5, :2] *= 1e-60
    for a in (qq, qc):
        a.setflags(write=False)
    return qq, qc


def _ordinary(seed, n, fam):
    return _rows(seed, n, fam.dim, fam.index_bits)


def _hostile_rows(seed, n, fam):
    codes, corr = _hostile(seed, n, fam.dim, 0)
    if fam.index_bits > 1:          # that recipe's corrections over this family's codes
        codes = np.random.default_rng(seed + 5).integers(0, 1 << fam.index_bits, size=(n, fam.dim), dtype=np.uint8)
        corr[:, 3] = code_sums(codes, fam.index_bits)
    return codes, corr


def _euclidean_inf_add(qadd):
    """the additionalCorrection x with 1 + (qadd + x) == 0 as f64 evaluates it: of a row with zero intervals (raw score 0), whose
    EUCLIDEAN score 1 / (1 + e) is then 1 / +0 = +inf"""
    x = -1.0 - qadd
    for c in (x, np.nextafter(x, 0.0), np.nextafter(x, -2.0)):
        if 1.0 + (qadd + c) == 0.0:
            return c
    raise AssertionError("no additionalCorrection cancels 1 + qadd exactly")


@functools.lru_cache(maxsize=None)
def rows(fam):
    """(codes, corr [n, 4]) of the family: seeded, read-only"""
    seed = _seed(fam)
    n = fam.n
    codes, corr = _ordinary(seed, n, fam)
    hcodes, hcorr = _hostile_rows(seed + 7, n, fam)
    rng = np.random.default_rng(seed + 8)
    hostile = np.zeros(n, bool)
    for t, kind in enumerate(tile_kinds(fam)):
        r = tile_rows(fam, t)
        if kind == "hostile":
            hostile[r] = True
        elif kind == "mixed":
            hostile[r] = rng.random(len(r)) < 0.5
        elif kind == "last":
            hostile[r[-1]] = True
    codes[hostile], corr[hostile] = hcodes[hostile], hcorr[hostile]
    for t, kind in enumerate(tile_kinds(fam)):
        if kind in ADD_PLANTS:
            corr[t * TILE + PLANT_LANE, 2] = ADD_PLANTS[kind]
        elif kind == "lu_nonfinite":
            for lane, col, v in LU_LANES:
                corr[t * TILE + lane, col] = v
    corr[EUC_INF_ROW, :3] =0.0, 0.0, _euclidean_inf_add(queries(fam, 0)[1][0, 2])
    assert (corr[:, 3] == code_sums(codes, fam.index_bits)).all()      # every row's sum is its code sum: the compact layout holds it
    for a in (codes, corr):
        a.setflags(write=False)
    return codes, corr


def score(fam, codes, corr, qq, qc, sim):
    """(qcDist, f64 score, f32 score) of every row: the oracle's"""
    return O.score_all(codes, corr, fam.dim, qq, qc, fam.query_bits, sim, CDP, ib=fam.index_bits)


@functools.lru_cache(maxsize=None)
def scores(fam, sim):
    """per query (qcDist, f64, f32) over rows(fam): computed once, read-only"""
    codes, corr = rows(fam)
    qq, qc = queries(fam, sim)
    out = tuple(score(fam, codes, corr, qq[q], qc[q], sim) for q in range(len(qq)))
    for s in out:
        for a in s:
            a.setflags(write=False)
    return out


# ------------------------------------------------------------------------------------------------ thresholds

_ONE, _INF = F32(1.0), F32(np.inf)
_SUB, _MIN, _MAX = F32(2.0 ** -149), np.finfo(F32).tiny, np.finfo(F32).max
FIXED = np.array([-_INF, _INF, 0.0, -0.0, _SUB, -_SUB, _MIN, -_MIN, _MAX, -_MAX, _ONE, np.nextafter(_ONE, _INF), np.nextafter(_ONE, -_INF),
                  0.5, 2.0, -1.0, 1e-30, 1e30], F32)


def _with_neighbours(v):
    with np.errstate(over="ignore"):
        return [np.nextafter(F32(v), -_INF), F32(v), np.nextafter(F32(v), _INF)]


def own_thresholds(s32):
    """{name: score} of the query's own scores a threshold is put on: among its finite scores the minimum, the best, 3rd and 300th
    best and the median; and of every special row present +0, +inf and the largest finite score (the best)"""
    s32 = np.asarray(s32, F32)
    fin = np.sort(s32[np.isfinite(s32)])
    own = {}
    if len(fin):
        own.update(minimum=fin[0], best=fin[-1], third=fin[-min(3, len(fin))], three_hundredth=fin[-min(300, len(fin))], median=fin[len(fin) // 2])
    if (s32.view(np.uint32) == 0).any():
        own["zero"] = F32(0.0)
    if (s32 == _INF).any():
        own["inf"] = _INF
    return own


def thresholds_of(s32):
    """the threshold table of one query, from the oracle's f32 scores of that query: FIXED, then own_thresholds each with its two
    neighbours; duplicates (by bit pattern: +0 and -0 are two thresholds) removed.  No NaN: a NaN threshold is refused"""
    ths = list(FIXED)
    for v in own_thresholds(s32).values():
        ths += _with_neighbours(v)
    ths = np.array(ths, F32)
    _, first = np.unique(ths.view(np.uint32), return_index=True)
    ths = ths[np.sort(first)]
    assert not np.isnan(ths).any()
    return ths


@functools.lru_cache(maxsize=None)
def pairs(fam, sim):
    """every (query, threshold) pair as the queries of ONE batched call: (qq [P, dim], qc [P, 4], thresholds [P], query of each pair [P])"""
    qq, qc = queries(fam, sim)
    who, ths = [], []
    for q, s in enumerate(scores(fam, sim)):
        t = thresholds_of(s[2])
        who += [q] * len(t)
        ths.append(t)
    who, ths = np.array(who), np.concatenate(ths)
    out = (np.ascontiguousarray(qq[who]), np.ascontiguousarray(qc[who]), ths, who)
    for a in out:
        a.setflags(write=False)
    return out


# ------------------------------------------------------------------------------------------------ filters and the update

def accept_sets(fam):
    """a random half; and whole tiles cleared - the NaN-additive tile, the partial last tile, a chunk's first tile and an inner one"""
    n = fam.n
    cleared = np.ones(n, bool)
    for t in (0, tile_of(fam, "add_nan"), CHUNK // TILE, tile_of(fam, "last")):
        cleared[t * TILE:(t + 1) * TILE] = False
    return {"a random half": np.random.default_rng(_seed(fam) + 9).random(n) < 0.5, "whole tiles cleared": cleared}


UPDATE_ORDINARY_TILE = 4       # KINDS[4]: an ordinary tile - one of its rows becomes a row with additionalCorrection 1e300


@functools.lru_cache(maxsize=None)
def update(fam):
    """(ords, codes, corr) of an update_rows call, and (codes, corr) of the index after it: a row of an ordinary tile gets
    additionalCorrection 1e300 (its tile's maximum becomes +inf as f32: the tile must stop rejecting under COSINE and MIP), and the NaN
    row of the NaN-additive tile becomes an ordinary row (both ends of its tile become finite: the tile must start rejecting)"""
    assert KINDS[UPDATE_ORDINARY_TILE] == "ordinary"
    codes, corr = rows(fam)
    ords = np.array([UPDATE_ORDINARY_TILE * TILE + 50, tile_of(fam, "add_nan") * TILE + PLANT_LANE], np.int32)
    ncodes, ncorr = _ordinary(_seed(fam) + 11, 2, fam)
    ncorr[0, 2] = 1e300
    after_codes, after_corr = codes.copy(), corr.copy()
    after_codes[ords], after_corr[ords] = ncodes, ncorr
    for a in (ords, ncodes, ncorr, after_codes, after_corr):
        a.setflags(write=False)
    return ords, ncodes, ncorr, after_codes, after_corr
