"""CPU: the folded form of the f32 score bound that the sweeps with several tiles per wave evaluate (bbq_scan_body.h: folded_bound_passes,
tile_threshold), restated in numpy with the same IEEE operations, next to test_bound_f32_cpu.py's restatement of fast_bound_passes.

    row side   g = ly D + b sum (D = qc - 4 sum, the digit counts' integer; b = fl(4 lyf + ayf)),  r = s + (K1 e + k2m w)
    tile side  T = ((zth - ca aadd) - pad) / cs,  pad = 2^-21 |aadd| + 2^-21 |zth - ca aadd| + cs tiny;   the row passes unless r <= T

Dominance: a row whose exact f32 score beats a threshold passes the folded test against that threshold's z image - every row against the
threshold ONE KEY below its own score, over test_bound_f32_cpu's hostile rows and query scales, all three similarities, fused and unfused,
the z image one ulp lower as well; and, for z images that no such key reaches (0, +-tiny, +-inf, negative ones), every row whose exact
z = cs s + ca add, evaluated in f64, lies above the image.  aadd of both signs and zero is in the hostile set; rows with al == au and
queries whose images overflow (they keep the f64 bound: the loop's threshold image is NaN and every row passes) are added here.
Pass count: on 2^18 rows of the benchmark's synthetic distribution, threshold at the 100th best key, the rows passing the old form and
the folded form are counted and printed (DESIGN section 7 quotes them); the folded form passes every row the exact score requires."""
import numpy as np
import pytest

import orclib as O
from test_bound_math_cpu import bf16_trunc
from test_bound_f32_cpu import (ADD_REL, F32, FBS, K1, QUERY_SCALES, bound_z, fma, hostile_rows, images, key_of_bits, passes, z_image)


def tile_threshold(zth, aadd, im, fused):
    with np.errstate(all="ignore"):
        zth, aadd = np.asarray(zth, F32), np.asarray(aadd, F32)
        num = zth - im["caf"] * aadd
        pad = fma(ADD_REL, np.abs(aadd), fma(ADD_REL, np.abs(num), im["csf"] * im["tinyf"], fused), fused)
        return ((num - pad) * F32(0.5 if im["csf"] == 2 else 1.0)).astype(F32)


def folded_r(qc, al, au, ones, im, fused):
    with np.errstate(all="ignore"):
        al, au = al.astype(F32), au.astype(F32)
        d = (np.asarray(qc, np.int64) - 4 * np.asarray(ones, np.int64)).astype(F32)   # exact: |D| < 2^24
        bf = fma(F32(4.0), im["lyf"], im["ayf"], True)                                 # fmaf on the device
        g = fma(im["lyf"], d, bf * ones.astype(F32), fused)
        A = im["c1f"] - g
        pa, pb = al * A, au * g
        s = pa + pb
        e = np.abs(pa) + np.abs(pb)
        w = np.abs(al) + np.abs(au)
        return s + fma(K1, e, w * im["k2mf"], fused)


def folded_passes(qc, al, au, aadd, ones, im, zth, fused):
    with np.errstate(all="ignore"):
        return ~(folded_r(qc, al, au, ones, im, fused) <= tile_threshold(zth, aadd, im, fused))


def hostile(seed, n=100000, dim=128):
    rng = np.random.default_rng(seed)
    codes, corr, x1 = hostile_rows(rng, n, dim, 1)
    corr[::97, 1] = corr[::97, 0]          # al == au
    qq = rng.integers(0, 16, dim).astype(np.uint8)
    return codes, corr, x1, qq, dim


@pytest.mark.parametrize("sim", [0, 1, 2])
def test_folded_bound_never_rejects_a_row_below_its_own_score(sim):
    codes, corr, x1, qq, dim = hostile(31 + sim)
    cdp, checked = 0.0009, 0
    al, au = bf16_trunc(corr[:, 0]), bf16_trunc(corr[:, 1])
    aadd = corr[:, 2].astype(F32)
    assert (aadd > 0).any() and (aadd < 0).any() and (aadd == 0).any() and (al == au).any()
    for scale in QUERY_SCALES:
        qc = np.array(scale + [float(qq.sum())])
        d, s64, s32 = O.score_all(codes, corr, dim, qq, qc, 4, sim, cdp)
        ly = (qc[1] - qc[0]) * FBS
        im = images(qc[0], ly, qc[3], float(dim), sim, dim, dim * 15)
        assert im is not None
        s32 = np.asarray(s32, F32)
        bits = s32.view(np.uint32)
        use = np.isfinite(s32) & (bits != 0)
        zth = z_image((key_of_bits(bits) - np.uint32(1)).astype(np.uint32), qc[2], cdp, sim, False)
        # the exact z in f64: s = lower A + upper B (bbq_kernel_common.h), z = cs s + ca add
        x1d, qd = x1.astype(np.float64), np.asarray(d, np.float64)
        with np.errstate(all="ignore"):
            s_raw = corr[:, 0] * (qc[0] * (dim - x1d) + ly * (qc[3] - qd)) + corr[:, 1] * (qc[0] * x1d + ly * qd)
            z_exact = float(im["csf"]) * s_raw + float(im["caf"]) * corr[:, 2]
        tiny = float(np.finfo(F32).tiny)
        special = [0.0, tiny, -tiny, 2.0 ** -140, -(2.0 ** -140), -np.inf, np.inf, -1.0, -1e-3, -1e6, 1e-3, 1.0] + list(np.quantile(z_exact[np.isfinite(z_exact)], [0.5, 0.9, 0.999]))
        for fused in (True, False):
            for z in (zth, np.nextafter(zth, F32(-np.inf))):
                rejected = use & ~folded_passes(np.asarray(d), al, au, aadd, x1, im, z, fused)
                assert not rejected.any(), "sim %d fused %s: %d rows rejected below their own score, first row %d" % (sim, fused, rejected.sum(), np.flatnonzero(rejected)[0])
            for zs in special:
                need = np.isfinite(z_exact) & (z_exact > zs)
                rejected = need & ~folded_passes(np.asarray(d), al, au, aadd, x1, im, np.full(len(aadd), zs, F32), fused)
                assert not rejected.any(), "sim %d fused %s z image %r: %d rows rejected" % (sim, fused, zs, rejected.sum())
            # a threshold image of -inf or NaN (a query without f32 images) passes every row; so does a non-finite additive bound
            for zs in (-np.inf, np.nan):
                assert folded_passes(np.asarray(d), al, au, aadd, x1, im, np.full(len(aadd), zs, F32), fused).all()
            for a in (np.inf, -np.inf, np.nan):
                assert folded_passes(np.asarray(d)[:1000], al[:1000], au[:1000], np.full(1000, a, F32), x1[:1000], im, zth[:1000], fused).all()
        checked += int(use.sum())
    assert checked > 2 * len(corr)


def test_queries_whose_images_overflow_keep_the_f64_bound():
    for ay, ly in ((1e60, 0.02), (-0.15, 1e60), (np.inf, 0.02)):
        assert images(ay, ly, 5000.0, 768.0, 1, 768.0, 768.0 * 15) is None   # fast_bound 0: the loop's threshold image is NaN


def synth(n, dim, seed):
    """bench.py's synth_rows / synth_queries, restated: uniform random bits, corrections around a real COSINE index's values"""
    rng = np.random.default_rng(seed)
    codes = rng.integers(0, 256, size=(n, dim // 8), dtype=np.uint8)
    u = rng.random((n, 3))
    corr = np.empty((n, 4))
    corr[:, 0] = -0.04 * (0.9 + 0.2 * u[:, 0])
    corr[:, 1] = 0.04 * (0.9 + 0.2 * u[:, 1])
    corr[:, 2] = 1e-4 * (2 * u[:, 2] - 1)
    x1 = np.unpackbits(codes, axis=1).sum(axis=1)
    corr[:, 3] = x1
    qq = rng.integers(0, 16, dim).astype(np.uint8)
    qc = np.array([-0.15 * (0.9 + 0.2 * rng.random()), 0.148 * (0.9 + 0.2 * rng.random()), -0.0028 * rng.random(), float(qq.sum())])
    return codes, corr, x1, qq, qc


@pytest.mark.parametrize("sim", [0, 1, 2])
def test_pass_counts_on_the_benchmarks_rows(sim):
    n, dim, cdp = 1 << 18, 768, 0.0009
    codes, corr, x1, qq, qc = synth(n, dim, 11)
    d, s64, s32 = O.score_all(codes, corr, dim, qq, qc, 4, sim, cdp)
    s32 = np.asarray(s32, F32)
    im = images(qc[0], (qc[1] - qc[0]) * FBS, qc[3], float(dim), sim, dim, dim * 15)
    al, au = bf16_trunc(corr[:, 0]), bf16_trunc(corr[:, 1])
    add = corr[:, 2].reshape(-1, 64)
    aadd = np.repeat((add.min(axis=1) if sim == 0 else add.max(axis=1)).astype(F32), 64)   # the tile's additive bound
    keys = key_of_bits(s32.view(np.uint32))
    key = np.sort(keys)[::-1][99]                                                          # the 100th best key
    zth = z_image(np.array([key], np.uint32), qc[2], cdp, sim, False)[0]
    old = passes(bound_z(np.asarray(d), al, au, aadd, x1, im), zth)
    new = folded_passes(np.asarray(d), al, au, aadd, x1, im, np.full(n, zth, F32), True)
    need = keys > key
    print("sim %d: of %d rows the old form passes %d, the folded form %d, the exact score requires %d" % (sim, n, old.sum(), new.sum(), need.sum()))
    assert need.sum() == 99 and (new | ~need).all() and (old | ~need).all()
