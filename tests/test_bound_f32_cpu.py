"""CPU: the f32 form of the compact layout's score bound (bbq_kernel_common.h: fast_bound_passes), the threshold's z image
(z_threshold_f32) and the host's decision to use them (bbq_query.cpp: fast_bound_images), restated in numpy with the same IEEE
operations.

Dominance: a row whose exact f32 score beats a threshold must pass the bound against that threshold's z image - checked for every
row against the threshold ONE KEY below its own score, over hostile magnitudes, all similarities, 1-bit and multi-bit rows, with the
fused multiply-adds evaluated fused and unfused, and with the z image one ulp lower.  Rows whose score is +0 are left out: one key
below +0 is -0.0, and a threshold is always the key of a real score, or 0.  (True of the sweep.  A range search's key comes from any
f32 the caller likes: tests/test_range_hostile_cpu.py covers those keys, +0 rows included.)
Tightness: on the benchmark's distributions the f32 bound passes at most 1.25 x the rows the f64 bound passes, + 2."""
import functools

import numpy as np
import pytest

import orclib as O
from test_bound_math_cpu import bf16_trunc, upper_bound

F32 = np.float32
FBS = 1.0 / 15.0
K1 = F32(0.0078125 * (1.0 + 1.0 / 65536.0) * (1.0 + 1.0 / 262144.0))
ADD_REL = F32(2.0 ** -21)
FLT_MIN, FLT_MAX = float(np.finfo(F32).tiny), float(np.finfo(F32).max)


# ---- the host side: fast_bound_images ---------------------------------------------------------------------------------------------
def f32_up(v):
    f = F32(v)
    return f if float(f) >= v else np.nextafter(f, F32(np.inf))


def image_ok(v, f):
    f = float(f)
    return np.isfinite(v) and abs(f) <= FLT_MAX and ((v == 0.0) if f == 0.0 else abs(f) >= FLT_MIN)


def images(ay, ly, y1, dim, sim, x1max, qcmax):
    """the f32 images of a query, or None where the query keeps the f64 bound (fast_bound = 0)"""
    with np.errstate(all="ignore"):
        c1 = np.float64(ay) * dim + np.float64(ly) * y1
        M = (abs(ay) * dim + abs(np.float64(ly) * y1) + 2.0 * (abs(ay) * x1max + abs(ly) * qcmax)) * 1.000001
        ayf, lyf, c1f = F32(ay), F32(ly), F32(c1)
    if not (image_ok(ay, ayf) and image_ok(ly, lyf) and image_ok(c1, c1f) and M >= 2.0 ** -80 and M <= 2.0 ** 100):
        return None
    return dict(ayf=ayf, lyf=lyf, c1f=c1f, k2mf=f32_up(M * 2.0 ** -20), tinyf=f32_up(max(2.0 ** -100, M * 2.0 ** -120)),
                csf=F32(2.0 if sim == 0 else 1.0), caf=F32(-1.0 if sim == 0 else 1.0))


# ---- the device side ------------------------------------------------------------------------------------------------------------
def fma(a, b, c, fused):
    if fused:   # the product of two floats is exact in f64; one rounding of the sum to f64 in front of the one to f32
        return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(F32)
    return (np.asarray(a, F32) * np.asarray(b, F32)).astype(F32) + np.asarray(c, F32)


def bound_z(qc, al, au, aadd, ones, im, fused=True):
    """zup of fast_bound_passes: the row passes unless zup <= z image"""
    with np.errstate(all="ignore"):
        al, au, aadd = al.astype(F32), au.astype(F32), aadd.astype(F32)
        g = fma(im["lyf"], qc.astype(F32), im["ayf"] * ones.astype(F32), fused)
        A = im["c1f"] - g
        pa, pb = al * A, au * g
        s = pa + pb
        e = np.abs(pa) + np.abs(pb)
        w = np.abs(al) + np.abs(au)
        slack = fma(K1, e, fma(w, im["k2mf"], im["tinyf"], fused), fused)
        zc = fma(im["csf"], s, im["caf"] * aadd, fused)
        zs = fma(im["csf"], slack, ADD_REL * np.abs(aadd), fused)
        z0 = zc + zs
        return fma(ADD_REL, np.abs(z0), z0, fused)


def key_of_bits(b):
    b = np.asarray(b, np.uint32)
    return np.where(b & np.uint32(0x80000000), ~b, b | np.uint32(0x80000000)).astype(np.uint32)


def bits_of_key(k):
    k = np.asarray(k, np.uint32)
    return np.where(k & np.uint32(0x80000000), k & np.uint32(0x7FFFFFFF), ~k).astype(np.uint32)


NEG = -np.finfo(np.float64).max


def z_f64(key, qadd, cdp, sim, plain):
    """z_threshold for an array of keys - any keys, the NaN patterns a range key of -inf is included: the conservative lower edge in
    z-space of "score > the float of the key", in f64 (-DBL_MAX accepts everything)"""
    key = np.asarray(key, np.uint32)
    with np.errstate(all="ignore"):
        th = bits_of_key(key).view(F32).astype(np.float64)
        if sim == 1:
            z = np.where(th < 0.0, NEG, (2.0 * th - 1.0) - (qadd - cdp))
        elif sim == 2:
            sc = 1.0 if plain else FBS
            t = np.where(th >= 1.0, (th - 1.0) * sc, np.where(th > 0.0, (1.0 - 1.0 / th) * sc, NEG))
            z = np.where(t == NEG, NEG, t - (qadd - cdp))
        else:
            z = np.where(th > 0.0, qadd + 1.0 - 1.0 / th, NEG)
        z = np.where((key == 0) | np.isnan(th) | ~(np.abs(z) <= -NEG), NEG, z)
        return np.where(z == NEG, NEG, z - 1e-9 * (np.abs(z) + abs(qadd) + abs(cdp) + 1.0))


def z_image(key, qadd, cdp, sim, plain):
    """z_threshold_f32 for an array of keys: z_threshold in f64, rounded down to f32 (-inf accepts everything)"""
    z = z_f64(key, qadd, cdp, sim, plain)
    with np.errstate(all="ignore"):
        zf = z.astype(F32)
        return np.where(zf.astype(np.float64) > z, np.nextafter(zf, F32(-np.inf)), zf).astype(F32)


def passes(zup, zth):
    with np.errstate(all="ignore"):
        return ~(zup <= zth)


# ---- dominance ------------------------------------------------------------------------------------------------------------------
def hostile_rows(rng, n, dim, ib):
    """test_bound_math_cpu.py's rows: corrections over 1e-12 .. 1e8, some of them zero"""
    if ib == 1:
        codes = rng.integers(0, 256, size=(n, dim // 8), dtype=np.uint8)
        x1 = np.unpackbits(codes, axis=1).sum(axis=1)
    else:
        codes = rng.integers(0, 1 << ib, size=(n, dim), dtype=np.uint8)
        x1 = codes.sum(axis=1)
    corr = np.zeros((n, 4))
    scale = 10.0 ** rng.uniform(-12, 6, n)
    corr[:, 0] = rng.standard_normal(n) * scale
    corr[:, 1] = rng.standard_normal(n) * scale * 10.0 ** rng.uniform(-2, 2, n)
    corr[:, 2] = rng.standard_normal(n) * 10.0 ** rng.uniform(-10, 6, n)
    corr[::101, 0] = 0
    corr[::103, 1] = 0
    corr[::107, 2] = 0
    corr[:, 3] = x1
    return codes, corr, x1


QUERY_SCALES = ([-0.15, 0.148, -0.0028], [-30.0, 55.0, 4.0], [1e-5, 2e-5, 0.0])


def check_dominance(codes, corr, x1, dim, qq, qb, sim, ib, cdp):
    n = len(corr)
    one_bit = qb == 1
    vmax = (1 << ib) - 1
    qmax = ((1 << qb) - 1) if ib == 1 else (255 if qb > 4 else 15)
    checked = 0
    for scale in QUERY_SCALES:
        qc = np.array(scale + [float(qq.sum())])
        d, s64, s32 = O.score_all(codes, corr, dim, qq, qc, qb, sim, cdp, ib=ib)
        ly = (qc[1] - qc[0]) if one_bit else (qc[1] - qc[0]) * FBS
        im = images(qc[0], ly, qc[3], float(dim), sim, dim * vmax, dim * vmax * qmax)
        assert im is not None, "an ordinary query takes the f32 bound"
        s32 = np.asarray(s32, F32)
        bits = s32.view(np.uint32)
        use = np.isfinite(s32) & (bits != 0)          # finite scores, +0 left out
        keys = (key_of_bits(bits) - np.uint32(1)).astype(np.uint32)   # one key below the row's own score
        zth = z_image(keys, qc[2], cdp, sim, one_bit or ib > 1)
        al, au = bf16_trunc(corr[:, 0]), bf16_trunc(corr[:, 1])
        aadd = corr[:, 2].astype(F32)
        for fused in (True, False):
            zup = bound_z(np.asarray(d), al, au, aadd, x1, im, fused)
            for z in (zth, np.nextafter(zth, F32(-np.inf))):
                rejected = use & ~passes(zup, z)
                assert not rejected.any(), "sim %d qb %d ib %d fused %s: %d of %d rows rejected below their own score, first row %d" % (
                    sim, qb, ib, fused, rejected.sum(), use.sum(), np.flatnonzero(rejected)[0])
        checked += int(use.sum())
    assert checked > 2 * n   # most rows have a finite, nonzero score


@pytest.mark.parametrize("sim", [0, 1, 2])
@pytest.mark.parametrize("qb", [1, 4, 8])
def test_f32_bound_never_rejects_a_row_below_its_own_score(sim, qb):
    rng = np.random.default_rng(7 * sim + qb)
    n, dim = 200000, 128
    codes, corr, x1 = hostile_rows(rng, n, dim, 1)
    qq = rng.integers(0, 1 << qb, dim).astype(np.uint8)
    check_dominance(codes, corr, x1, dim, qq, qb, sim, 1, 0.0009)


@pytest.mark.parametrize("sim", [0, 1, 2])
def test_f32_bound_multibit_rows(sim):
    """codes < 4, x1 = the code sum: the magnitudes scale by 2^indexBits - 1 (the per-row scorer's form: centroidDP 0, MIP undivided)"""
    rng = np.random.default_rng(100 + sim)
    n, dim, ib, qb = 50000, 128, 2, 4
    codes, corr, x1 = hostile_rows(rng, n, dim, ib)
    qq = rng.integers(0, 1 << qb, dim).astype(np.uint8)
    check_dominance(codes, corr, x1, dim, qq, qb, sim, ib, 0.0)


# ---- the fallback flag -------------------------------------------------------------------------------------------------------------
def test_queries_outside_f32_keep_the_f64_bound():
    dim, x1max, qcmax = 768.0, 768.0, 768.0 * 15
    assert images(-0.15, 0.02, 5000.0, dim, 1, x1max, qcmax) is not None
    assert images(0.0, 0.02, 5000.0, dim, 1, x1max, qcmax) is not None          # a zero image is an exact image
    for ay, ly, y1 in ((1e60, 0.02, 5000.0), (-0.15, 1e60, 5000.0), (-0.15, 0.02, 1e60),        # overflow f32 / the magnitude limit
                       (1e-60, 0.02, 5000.0), (-0.15, 1e-60, 5000.0), (1e-60, 1e-60, 5000.0),    # nonzero below the normal range
                       (np.nan, 0.02, 5000.0), (-0.15, np.inf, 5000.0), (-0.15, 0.02, np.nan),
                       (1e-30, 1e-30, 1.0)):                                                     # images fine, magnitude below 2^-80
        assert images(ay, ly, y1, dim, 1, x1max, qcmax) is None, (ay, ly, y1)
    # c1 = ay dim + ly y1 cancels below the normal range while both terms are ordinary
    assert images(1.0, -768.0 * (1 + 2.0 ** -52), 1.0, dim, 1, x1max, qcmax) is not None  # (c1 = -768 * 2^-52: normal)
    assert images(2.0 ** -85, -(2.0 ** -85) * 768.0 * (1 + 2.0 ** -52), 1.0, dim, 1, x1max, qcmax) is None


def test_threshold_image_of_key_zero_and_reset_word():
    """key 0 <-> -inf, and the stored form (bits XOR the bits of -inf) of that pair is all zero: what the host resets the control words to"""
    z = z_image(np.array([0], np.uint32), -0.002, 0.0009, 1, False)
    assert z[0] == -np.inf
    assert (z.view(np.uint32) ^ np.uint32(0xFF800000))[0] == 0
    assert passes(np.array([-3.0e38], F32), z).all()


# ---- tightness on the benchmark's distributions -------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def bench_like():
    """synth_rows / synth_queries of bench.py: 768-d, uniform random bits, corrections around a real COSINE index's values"""
    rng = np.random.default_rng(11)
    n, dim, qb = 204800, 768, 4
    codes = rng.integers(0, 256, size=(n, dim // 8), dtype=np.uint8)
    u = rng.random((n, 3))
    corr = np.empty((n, 4))
    corr[:, 0] = -0.04 * (0.9 + 0.2 * u[:, 0])
    corr[:, 1] = 0.04 * (0.9 + 0.2 * u[:, 1])
    corr[:, 2] = 1e-4 * (2 * u[:, 2] - 1)
    x1 = np.unpackbits(codes, axis=1).sum(axis=1)
    corr[:, 3] = x1
    qq = rng.integers(0, 1 << qb, dim).astype(np.uint8)
    qc = np.array([-0.15 * (0.9 + 0.2 * rng.random()), 0.148 * (0.9 + 0.2 * rng.random()), -0.0028 * rng.random(), float(qq.sum())])
    for a in (codes, corr, x1, qq, qc):
        a.setflags(write=False)
    return codes, corr, x1, qq, qc


@pytest.mark.parametrize("sim", [0, 1, 2])
def test_f32_bound_is_as_tight_as_the_f64_bound(sim):
    codes, corr, x1, qq, qc = bench_like()
    n, dim, qb, cdp = len(corr), 768, 4, 0.0009
    d, s64, s32 = O.score_all(codes, corr, dim, qq, qc, qb, sim, cdp)
    s32 = np.asarray(s32, F32)
    ly = (qc[1] - qc[0]) * FBS
    im = images(qc[0], ly, qc[3], float(dim), sim, dim, dim * 15)
    assert im is not None
    al, au = bf16_trunc(corr[:, 0]), bf16_trunc(corr[:, 1])
    # the tile's additive bound as the kernels take it: min (EUCLIDEAN) or max of the tile's 64 rows, as f32
    add = corr[:, 2].reshape(-1, 64)
    aadd = np.repeat((add.min(axis=1) if sim == 0 else add.max(axis=1)).astype(F32), 64)
    zup = bound_z(np.asarray(d), al, au, aadd, x1, im)
    u64 = upper_bound(np.asarray(d, np.float64), al, au, aadd.astype(np.float64), x1.astype(np.float64), qc[0], ly, qc[3], qc[2], cdp,
                      float(dim), sim, False).astype(F32)
    order = np.sort(key_of_bits(s32.view(np.uint32)))[::-1]
    for rank in (4, 40):
        key = order[rank - 1]
        n32 = int(passes(zup, z_image(np.array([key], np.uint32), qc[2], cdp, sim, False)[0]).sum())
        n64 = int((np.isnan(u64) | (key_of_bits(u64.view(np.uint32)) > key)).sum())
        print("sim %d rank %d: f32 bound passes %d rows, f64 bound %d, above the threshold %d" % (sim, rank, n32, n64, rank - 1))
        assert n64 >= rank - 1 and n32 >= rank - 1
        assert n32 <= 1.25 * n64 + 2
