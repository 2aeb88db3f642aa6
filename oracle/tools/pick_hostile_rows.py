#!/usr/bin/env python3
"""Picks the 48 rows of dimension 13 that gen_fixtures.js records the reference on as quant_hostile_* (TEST INFRASTRUCTURE).

The rows come from the batches of tests/quant_hostile.py: the head of `mixed` (every kind of row it holds) and two f32-denormal rows
of `extreme`; the last row is the f32 centroid of the others, which is then the centroid of all 48 as well - the row that `identical`
is made of: a zero centred vector under EUCLIDEAN and MAXIMUM_INNER_PRODUCT.  With the oracle's trace the script checks that, over the
cases gen_fixtures.js runs them through, every exit of optimizeIntervals is taken and some rows carry NaN corrections, and writes
oracle/tools/quant_hostile_rows.json (inputs only: f32 rows and two queries, base64 of little-endian bytes).

Usage: python3 oracle/tools/pick_hostile_rows.py
"""
import base64
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "..", "tests"))
import orclib as O            # noqa: E402
import quant_hostile as Q     # noqa: E402

N, DIM = 48, 13
PIN_GRID = ((1, 0.0, 5), (1, 1.0, 5), (2, 0.1, 0), (4, 1.0, 3))


def main():
    rows = np.concatenate([Q.batch("mixed", 601, DIM)[:N - 3], Q.batch("extreme", 601, DIM)[[0, 5]]]).astype(np.float32)
    cen = np.zeros(DIM, np.float32)
    O.lib().orc_centroid(O.f32p(rows), len(rows), DIM, O.f32p(cen))
    rows = np.ascontiguousarray(np.concatenate([rows, cen[None, :]]))
    assert rows.shape == (N, DIM)
    for _ in range(50):   # f32 rounding can move the centroid when it joins the rows: settle on a fixed point
        O.lib().orc_centroid(O.f32p(rows), N, DIM, O.f32p(cen))
        if (cen == rows[-1]).all():
            break
        rows[-1] = cen
    assert (cen == rows[-1]).all(), "the centroid does not settle"
    queries = np.stack([rows[np.flatnonzero(rows.any(axis=1))[0]], Q.benign(1, DIM, 1)[0]])
    table, total = [], np.zeros(len(Q.CLASSES), np.int64)
    for sn in Q.SIM_NAMES:
        for ib, lam, iters in PIN_GRID:
            cen = O.build_index(rows, O.SIMS[sn], lam, iters, ib)[2]
            _, corr, trace = O.quantize_trace(rows, cen, O.SIMS[sn], ib, lam, iters)
            cnt = Q.classify(trace, corr)
            table.append(("%s ib=%d lambda=%g iters=%d" % (sn, ib, lam, iters), cnt))
            total += cnt
    table.append(("all", total))
    print(Q.table(table))
    exits = [total[0] + total[1], total[7], total[2], total[3] + total[8], total[4] + total[5]]
    assert all(exits) and total[1] + total[3] + total[5] > 0 and total[6] > 0 and total[9] > 0, "an exit is missing from the picked rows"
    out = {"n": N, "dim": DIM, "base_f32": base64.b64encode(rows.astype("<f4").tobytes()).decode(),
           "queries_f32": base64.b64encode(queries.astype("<f4").tobytes()).decode()}
    with open(os.path.join(HERE, "quant_hostile_rows.json"), "w") as f:
        json.dump(out, f)


if __name__ == "__main__":
    main()
