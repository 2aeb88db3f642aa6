#!/usr/bin/env python3
"""CPU model of the staged unit digit plane (docs/dropped.md, "staged bound"): on bench.py's own synthetic rows and queries, how many rows and
how many 64-row tiles pass the sweep's row bound when the unit-weight digit plane of the LAST n dwords of a row is left unresolved and
replaced by its interval [-L, U] (U = pop(P0), L = pop(N0) over those dwords).

The bound's row side r = s + K1 e + k2m w is increasing in D wherever al <= 0 <= au and ly > 0 (every row and query of the benchmark), so the
midpoint form with the half-width folded into k2m passes exactly the rows whose r at the interval's upper end D + (U - tail) passes: that is
what is counted here, in f64, with bf16-truncated corrections and the K1 and k2m allowances of bbq_kernel_common.h.  The threshold of a
query is its k-th best exact score over a PREFIX of the index, as the launch behind that prefix sees it.

    python scripts/staged_bound_model.py [--prefix 2000000] [--rows 262144] [--queries 32] [--dim 768] [--sim COSINE] [--json out.json]
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import bench  # noqa: E402  (synth_rows, synth_queries: the benchmark's own generators)

K1 = 0.0078125 * (1 + 2.0 ** -16) * (1 + 2.0 ** -18)
FBS = 1.0 / 15.0
NS = (0, 4, 6, 8, 12)


def bf16_trunc(x):
    b = np.asarray(x, np.float32).view(np.uint32) & np.uint32(0xFFFF0000)
    return b.view(np.float32).astype(np.float64)


def unit_digit(q):
    """the unit balanced-ternary digit of q - 4 (bbq_device.h, kDigitTable): -1, 0 or 1"""
    return ((q.astype(np.int64) - 4 + 1) % 3) - 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--prefix", type=int, default=2_000_000)
    ap.add_argument("--rows", type=int, default=262_144)
    ap.add_argument("--queries", type=int, default=32)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--sim", default="COSINE", choices=["EUCLIDEAN", "COSINE", "MAXIMUM_INNER_PRODUCT"])
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    dim, pb, nq = a.dim, a.dim // 8, a.queries
    sim = {"EUCLIDEAN": 0, "COSINE": 1, "MAXIMUM_INNER_PRODUCT": 2}[a.sim]
    cs, ca = (2.0, -1.0) if sim == 0 else (1.0, 1.0)
    qq, qc = bench.synth_queries(2, nq, dim)
    ay, ly, y1 = qc[:, 0], (qc[:, 1] - qc[:, 0]) * FBS, qc[:, 3]
    qf = qq.T.astype(np.float32)                       # [dim, nq]
    d0 = unit_digit(qq)                                # [nq, dim]
    tails = {n: slice(dim - 32 * n, dim) for n in NS if n}
    U = {n: (d0[:, tails[n]] == 1).sum(axis=1) for n in tails}
    L = {n: (d0[:, tails[n]] == -1).sum(axis=1) for n in tails}
    M = (np.abs(ay) * dim + np.abs(ly * y1) + 2 * (np.abs(ay) * dim + np.abs(ly) * dim * 15)) * 1.000001
    k2m = M * 2.0 ** -20

    def block(r0, r1):
        codes, corr = bench.synth_rows(1, r0, r1, pb)
        bits = np.unpackbits(codes, axis=1).astype(np.float32)     # MSB first, as the rows are packed
        x1 = corr[:, 3][:, None]
        qcd = (bits @ qf).astype(np.float64)                       # exact: at most 15 dim
        tail = {n: (bits[:, tails[n]] @ d0[:, tails[n]].T.astype(np.float32)).astype(np.float64) for n in tails}
        return corr, x1, qcd, tail

    def z_exact(corr, x1, qcd):
        s = corr[:, :1] * (ay * (dim - x1) + ly * (y1 - qcd)) + corr[:, 1:2] * (ay * x1 + ly * qcd)
        return cs * s + ca * corr[:, 2:3]

    def r_side(corr, x1, qcd):
        al, au = bf16_trunc(corr[:, 0])[:, None], bf16_trunc(corr[:, 1])[:, None]
        pa, pb_ = al * (ay * (dim - x1) + ly * (y1 - qcd)), au * (ay * x1 + ly * qcd)
        return pa + pb_ + K1 * (np.abs(pa) + np.abs(pb_)) + k2m * (np.abs(al) + np.abs(au))

    out = {"rows": a.rows, "queries": nq, "dim": dim, "sim": a.sim, "k": a.k, "n": list(NS), "prefixes": {}}
    B = 65536
    prefixes = sorted({a.prefix, max(a.k, a.prefix // 8)})
    best = np.full((a.k, nq), -np.inf)
    th, done = {}, 0
    for p in prefixes:
        for r0 in range(done, p, B):
            corr, x1, qcd, _ = block(r0, min(p, r0 + B))
            best = np.sort(np.concatenate([best, z_exact(corr, x1, qcd)]), axis=0)[-a.k:]
        done = p
        th[p] = best[0].copy()
    # the rows behind the largest prefix: what the launch with that prefix's thresholds sweeps
    stats = {p: {n: [0, 0] for n in NS} for p in prefixes}
    need = {p: 0 for p in prefixes}
    for r0 in range(prefixes[-1], prefixes[-1] + a.rows, B):
        corr, x1, qcd, tail = block(r0, min(prefixes[-1] + a.rows, r0 + B))
        aadd = np.repeat((corr[:, 2].reshape(-1, 64).min(axis=1) if sim == 0 else corr[:, 2].reshape(-1, 64).max(axis=1)), 64)[:, None]
        z = z_exact(corr, x1, qcd)
        for p in prefixes:
            T = (th[p] - ca * aadd) / cs
            need[p] += int((z > th[p]).sum())
            for n in NS:
                up = qcd if n == 0 else qcd - tail[n] + U[n]
                ps = r_side(corr, x1, up) > T
                stats[p][n][0] += int(ps.sum())
                stats[p][n][1] += int(ps.reshape(-1, 64, nq).any(axis=1).sum())
    pairs, tiles = a.rows * nq, a.rows // 64 * nq
    for p in prefixes:
        print("thresholds of the first %d rows (the %d-th best exact score per query); %d rows x %d queries behind them; %d pairs beat the threshold" % (p, a.k, a.rows, nq, need[p]))
        o = out["prefixes"][str(p)] = {"pairs_above_threshold": need[p], "by_n": {}}
        for n in NS:
            r, t = stats[p][n]
            h = 0 if n == 0 else float(np.mean(U[n] + L[n])) / 2
            print("  n = %2d  half-width %5.1f units  rows passing %.5f  tiles with a passing row %.4f" % (n, h, r / pairs, t / tiles))
            o["by_n"][str(n)] = {"mean_half_width": h, "row_share": r / pairs, "tile_share": t / tiles}
    if a.json:
        json.dump(out, open(a.json, "w"), indent=1)


if __name__ == "__main__":
    main()
