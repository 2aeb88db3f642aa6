"""The expected value of every append test: quantizeVectors' per-row part on the ORACLE's functions.  quantizeVectors computes the
centroid and then calls scalarQuantize(v, dest, indexBits, centroid) row by row (src/binaryQuantizationFormat.ts:214-249), so "the
rows of V2 quantized against the centroid the index was built with" is orc_normalize (COSINE), orc_scalar_quantize(row, centroid) and,
for 1-bit rows, orc_pack_binary.  tests/test_append_cpu.py holds the recipe to the oracle's own build (orc_build_index*)."""
import numpy as np

import orclib as O


def oracle_rows(vectors, cen, sim, ib, lam=0.1, iters=5):
    """the per-row recipe of the issue, straight on the oracle's C functions"""
    v = np.ascontiguousarray(vectors, np.float32)
    cen = np.ascontiguousarray(cen, np.float32)
    n, dim = v.shape
    L = O.lib()
    codes = np.zeros((n, (dim + 7) // 8 if ib == 1 else dim), np.uint8)
    corr = np.zeros((n, 4), np.float64)
    row, dest, packed = np.zeros(dim, np.float32), np.zeros(dim, np.uint8), np.zeros((dim + 7) // 8, np.uint8)
    for i in range(n):
        if sim == 1:
            L.orc_normalize(O.f32p(v[i]), dim, O.f32p(row))
        else:
            row[:] = v[i]
        L.orc_scalar_quantize(O.f32p(row), dim, ib, O.f32p(cen), sim, lam, iters, O.u8p(dest), O.f64p(corr[i]))
        if ib == 1:
            L.orc_pack_binary(O.u8p(dest), dim, O.u8p(packed))
            codes[i] = packed
        else:
            codes[i] = dest
    return codes, corr
