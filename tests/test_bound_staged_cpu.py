"""CPU: stage one of the staged twins of the many-tile digit sweep (bbq_scan_body.h: sweep_wave_tiles' STG; bbq_query.cpp: staged_bound_words),
restated in numpy f32 next to test_bound_folded_cpu.py's restatement of folded_bound_passes.

    stage one  the folded bound's row side at D' = D_res + m, m = floor((U - L) / 2), with k2m' = 3 k2m + h |ly| (1 + 2 K1) (rounded up),
               h = U - m, where U = pop(P0) and L = pop(N0) over the row's last n dwords and D_res is D without their unit digit plane
    stage two  folded_bound_passes at the true D with k2m: unchanged

Dominance: no row that folded_bound_passes passes is rejected by stage one - for 4 dwords, the twin that is built, and 8, the three similarities,
fused and unfused, over test_bound_f32_cpu's hostile rows (huge, subnormal, NaN and infinite corrections) and query scales, against the
threshold one key below each row's own score, one ulp lower, and the special images 0, +-tiny, +-inf, NaN (+inf as the kernel has it: it
turns a tile threshold of +inf into NaN for both stages).  Excepted, as the budget above staged_bound_words says: a row whose r is NOT
finite at D (a product or sum overflowed f32) while r' at D' is finite - stage one's r' is then a valid bound computed without overflow.
The stage-one constants of the restatement are the LIBRARY's: bbq_staged_bound_words (host only) runs fill_query_digits and
staged_bound_words, and its K', k2m', K - K' and h are what stage_one_r computes with.
The words: on the masks the library stages - at 768-d, at 1000-d (24 padding positions in the last chunk) and at 200-d (56, more than a
dword) - U, L are counted bit by bit on P0 and N0 of the last n dwords, K on N0 and N1 of all, and the library's K', K - K', h and k2m' must
equal m = floor((U - L) / 2), K - L - m, L + m, U - m and the float at or above 3 k2m + h |ly| (1 + 2 K1); the padding positions must be
staged in N0 and N1 and nowhere else; a query without f32 images gets k2m' = 0."""
import numpy as np
import pytest

import orclib as O
from bbqlib import capi
from test_bound_math_cpu import bf16_trunc
from test_bound_f32_cpu import F32, FBS, K1, QUERY_SCALES, fma, images, key_of_bits, z_image
from test_bound_folded_cpu import folded_r, hostile, tile_threshold

NS = (4, 8)          # dwords: 4 is the staged twin that is built (one chunk); 8 was measured and dropped


def unit_digits(qq):
    """the unit balanced-ternary digit of q - 4 per dimension: -1, 0, 1"""
    return ((qq.astype(np.int64) - 3) % 3) - 1


def staged_words(qq, dim, n, im):
    """the library's stage-one words for the query (bbq_staged_bound_words): m, h, k2m' and the unit digits per position (padding: -1)"""
    masks, K, words = capi.staged_bound_words(qq, im["lyf"], im["k2mf"], 1, n // 4)
    w16 = (dim + 127) // 128
    p0, n0 = np.unpackbits(masks[:, 0, :].reshape(-1)), np.unpackbits(masks[:, 1, :].reshape(-1))
    assert not (p0 & n0).any()
    d0 = p0.astype(np.int64) - n0.astype(np.int64)
    assert (d0[:dim] == unit_digits(qq)).all() and len(d0) == w16 * 128
    tail = d0[w16 * 128 - 32 * n:]
    U, L = int((tail == 1).sum()), int((tail == -1).sum())
    rest, h = int(words[2]), int(words[3])
    m = rest - L
    assert int(words[0]) == (K - rest) % 2 ** 32
    return U, L, m, h, words[1:2].view(F32)[0], d0


def stage_one_r(codes, d, al, au, ones, im, words, dim, n, fused):
    U, L, m, h, k2, d0 = words
    bits = np.unpackbits(codes, axis=1)[:, :len(d0)].astype(np.int64)
    tail_at = len(d0) - 32 * n
    tail = bits[:, tail_at:dim] @ d0[tail_at:dim]                      # the row's own contribution of the unresolved dwords: in [-L, U]
    assert (tail >= -L).all() and (tail <= U).all()
    d_mid = np.asarray(d, np.int64) - tail + m
    assert (np.abs(np.asarray(d, np.int64) - d_mid) <= h).all()
    im1 = dict(im)
    im1["k2mf"] = k2
    return folded_r(d_mid, al, au, ones, im1, fused)


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("sim", [0, 1, 2])
def test_stage_one_rejects_no_row_the_bound_passes(sim, n):
    codes, corr, x1, qq, dim = hostile(41 + sim, 30000, 768)
    cdp, checked = 0.0009, 0
    al, au = bf16_trunc(corr[:, 0]), bf16_trunc(corr[:, 1])
    aadd = corr[:, 2].astype(F32)
    for scale in QUERY_SCALES:
        qc = np.array(scale + [float(qq.sum())])
        d, s64, s32 = O.score_all(codes, corr, dim, qq, qc, 4, sim, cdp)
        ly = (qc[1] - qc[0]) * FBS
        im = images(qc[0], ly, qc[3], float(dim), sim, dim, dim * 15)
        assert im is not None
        words = staged_words(qq, dim, n, im)
        s32 = np.asarray(s32, F32)
        zth = z_image((key_of_bits(s32.view(np.uint32)) - np.uint32(1)).astype(np.uint32), qc[2], cdp, sim, False)
        tiny = float(np.finfo(F32).tiny)
        images_z = [zth, np.nextafter(zth, F32(-np.inf))] + [np.full(len(aadd), z, F32) for z in (0.0, tiny, -tiny, -np.inf, np.inf, np.nan, -1.0, 1.0, 1e-3, -1e6)]
        for fused in (True, False):
            with np.errstate(all="ignore"):
                r2 = folded_r(np.asarray(d), al, au, x1, im, fused)
                r1 = stage_one_r(codes, d, al, au, x1, im, words, dim, n, fused)
                overflowed = ~np.isfinite(r2) & np.isfinite(r1)     # the budget's one exception
            for z in images_z:
                with np.errstate(all="ignore"):
                    T = tile_threshold(z, aadd, im, fused)
                    T = np.where(T == np.inf, F32(np.nan), T)                  # the kernel's clamp, for both stages
                    two, one = ~(r2 <= T), ~(r1 <= T)
                rejected = two & ~one & ~overflowed
                assert not rejected.any(), "sim %d n %d fused %s: %d rows pass the bound and fail stage one, first row %d" % (sim, n, fused, rejected.sum(), np.flatnonzero(rejected)[0])
                checked += int(two.sum())
    assert checked > len(corr)


@pytest.mark.parametrize("dim,n", [(768, 4), (768, 8), (1000, 4), (1000, 8), (200, 4)])
def test_words_equal_a_direct_count_on_the_masks(dim, n):
    w16 = (dim + 127) // 128
    rng = np.random.default_rng(dim + n)
    for trial in range(8):
        qq = rng.integers(0, 16, dim).astype(np.uint8)
        if trial == 1:
            qq[:] = 5      # unit digit +1 everywhere: U - L as large as it gets
        if trial == 2:
            qq[:] = 3      # -1 everywhere: m negative
        lyf, k2mf = F32(0.0198 * (1 + trial)), F32(3.1e-4 * (1 + trial))
        masks, K, words = capi.staged_bound_words(qq, lyf, k2mf, 1, n // 4)
        bits = np.unpackbits(masks, axis=2).transpose(1, 0, 2).reshape(5, w16 * 128).astype(np.int64)   # [mask][position]
        P0, N0, P1, N1, P2 = bits
        # the masks are the digits of q - 4, and a padding position is the value 0: bits in N0 and N1 alone
        v = qq.astype(np.int64) - 4
        assert ((P0 - N0 + 3 * (P1 - N1) + 9 * P2)[:dim] == v).all()
        assert (N0[dim:] == 1).all() and (N1[dim:] == 1).all() and not P0[dim:].any() and not P1[dim:].any() and not P2[dim:].any()
        assert K == int(N0.sum() + 3 * N1.sum())
        last = slice(w16 * 128 - 32 * n, w16 * 128)
        U, L = int(P0[last].sum()), int(N0[last].sum())
        assert L >= min(32 * n, w16 * 128 - dim)
        m = (U - L) // 2                    # floor, also for a negative difference
        h = U - m
        assert h == max(U - m, m + L) and h - (U + L) / 2 in (0.0, 0.5)
        assert int(words[0]) == (K - L - m) % 2 ** 32 and int(words[2]) == (L + m) % 2 ** 32 and int(words[3]) == h
        k2 = float(words[1:2].view(F32)[0])
        need = 3.0 * float(k2mf) + h * float(lyf) * (1.0 + 2.0 * float(K1))
        assert need <= k2 <= need * (1 + 2.0 ** -10), (k2, need)
        # a query without f32 images: k2m' = 0, like its k2m
        assert int(capi.staged_bound_words(qq, 0.0, 0.0, 0, n // 4)[2][1]) == 0
