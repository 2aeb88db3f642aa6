#!/usr/bin/env python3
"""Replacing rows at size: what bbq_index_update costs next to an append of the same rows and next to what a user had to do before.
768-d COSINE, 1-bit index.  Prints ONE JSON line (profiles/index_update.json).

  python scripts/bench_update.py                                   # N = 1 M and 10 M, B = 1 K / 64 K / 1 M
  python scripts/bench_update.py --sizes 1000000 --blocks 1000,65536 --runs 3

Per (N, B), host clock around the call, no host copies, medians of --runs, the legs interleaved run by run in one process:
  update_random      bbq_index_update of B raw fp32 rows at B random ords (duplicates as they fall)
  update_contiguous  ... at the B ords from N / 3 on
  append             bbq_index_append of the same rows into reserved room: the yardstick - the same upload and quantization; an update
                     adds the staged form (quantize into scratch, untile) and the scatter.  The index it runs on grows by B per run,
                     inside its reservation: an append into reserved room writes the new rows alone, whatever the size.
  remove_append      bbq_index_remove_rows of B ords + bbq_index_append of B rows: what replacing rows took before (it renumbers the rows
                     behind, invalidates the filters and gathers the whole index out of place)
One query per update leg is held to the oracle: the block's rows as bbq_index_update returns them, scored by the oracle, against
bbq_score_rows of the updated ords."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "better-binary-quantization_amd", "python")):
    if p not in sys.path:
        sys.path.insert(0, p)

DIM, SIM, QB = 768, 1, 4


def raw_rows(seed, n):
    return np.random.default_rng([seed, 99]).standard_normal((n, DIM)).astype(np.float32)


def med_ms(ts):
    return round(float(np.median(ts)) * 1e3, 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1000000,10000000", help="N: rows of the index")
    ap.add_argument("--blocks", default="1000,65536,1000000", help="B: rows per update")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--no-remove-append", action="store_true", help="skip the remove_rows + append leg")
    args = ap.parse_args()
    sizes = [int(x) for x in args.sizes.split(",") if x]
    blocks = [int(x) for x in args.blocks.split(",") if x]

    import torch  # noqa: F401  (first: one HIP runtime for torch and libbbq, as bench.py does)
    import bench
    import orclib as O
    import bbq_amd as B
    if B.device_count() < 1:
        raise SystemExit("bench_update: no HIP device - nothing here can be measured without one")
    cen = bench.synth_centroid(DIM)
    cdp = float(B.centroid_dp(cen))
    qq, qc = bench.synth_queries(55, 1, DIM, QB)
    out = {"what": "bbq_index_update at 768-d COSINE, 1-bit; host clock, ms, medians of %d runs, legs interleaved" % args.runs, "dim": DIM,
           "runs": args.runs, "update": {}, "held_to_oracle": {}}

    warm = B.Index(*bench.synth_rows(1, 0, 4096, DIM // 8), DIM, cdp)   # context, code objects, allocator: not timed
    warm.update(np.arange(2000) % 4096, raw_rows(1, 2000), cen, SIM, want_host_copy=False)
    warm.append(raw_rows(1, 2000), cen, SIM, want_host_copy=False)
    warm.remove_rows(np.arange(100))
    warm.close()
    new_rows = {b: raw_rows(7, b) for b in blocks}
    for n in sizes:
        codes, corr = bench.synth_rows(1, 0, n, DIM // 8)
        upd = B.Index(codes, corr, DIM, cdp)
        app = B.Index(codes, corr, DIM, cdp)
        app.reserve(n + (args.runs + 1) * sum(blocks))
        rem = None if args.no_remove_append else B.Index(codes, corr, DIM, cdp)
        del codes, corr
        rng = np.random.default_rng([11, n])
        per_n = {}
        for b in blocks:
            if b > n:
                continue
            t = {"update_random": [], "update_contiguous": [], "append": [], "remove_append": []}
            contiguous = np.arange(n // 3, n // 3 + b, dtype=np.int64)
            for _ in range(args.runs):
                random_ords = rng.integers(0, n, b)
                t0 = time.perf_counter()
                upd.update(random_ords, new_rows[b], cen, SIM, want_host_copy=False)
                t["update_random"].append(time.perf_counter() - t0)
                t0 = time.perf_counter()
                app.append(new_rows[b], cen, SIM, want_host_copy=False)
                t["append"].append(time.perf_counter() - t0)
                t0 = time.perf_counter()
                upd.update(contiguous, new_rows[b], cen, SIM, want_host_copy=False)
                t["update_contiguous"].append(time.perf_counter() - t0)
                if rem is not None:
                    t0 = time.perf_counter()
                    rem.remove_rows(random_ords)
                    rem.append(new_rows[b][:n - rem.n], cen, SIM, want_host_copy=False)   # as many rows as the distinct ords removed
                    t["remove_append"].append(time.perf_counter() - t0)
                    assert rem.n == n
            assert upd.n == n
            e = {k + "_ms": med_ms(v) for k, v in t.items() if v}
            e.update({k + "_runs_ms": [round(x * 1e3, 3) for x in v] for k, v in t.items() if v})
            e["update_random_over_append"] = round(e["update_random_ms"] / e["append_ms"], 3)
            e["update_contiguous_over_append"] = round(e["update_contiguous_ms"] / e["append_ms"], 3)
            if rem is not None:
                e["remove_append_over_update_random"] = round(e["remove_append_ms"] / e["update_random_ms"], 3)
            per_n[str(b)] = e
        out["update"][str(n)] = per_n
        # one query per update leg against the oracle, on a block of 1000 rows
        m = min(1000, n)
        held = {}
        for leg, ords in (("random", rng.permutation(n)[:m]), ("contiguous", np.arange(n // 2, n // 2 + m))):
            bc, br = upd.update(ords, new_rows[blocks[-1]][:m] if blocks[-1] >= m else raw_rows(7, m), cen, SIM)
            want = O.score_all(bc, br, DIM, qq[0], qc[0], QB, SIM, cdp)
            lo, hi = int(ords.min()), int(ords.max()) + 1
            got = upd.score_rows(qq[0], qc[0], QB, SIM, lo, hi - lo)
            held[leg] = bool(all((np.asarray(g)[ords - lo].view(np.uint8) == np.asarray(w).view(np.uint8)).all() for g, w in zip(got, want)))
        out["held_to_oracle"][str(n)] = held
        for h in (upd, app, rem):
            if h is not None:
                h.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
