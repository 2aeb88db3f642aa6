#!/usr/bin/env python3
"""The exact search at size: bbq_vectors_search_batch beside the only exact way a caller had without it, for the same request, in one
process, the ways interleaved call by call so that drift of the box hits both alike.  Prints ONE JSON line (profiles/exact_search.json).

  python scripts/bench_exact.py              # 1 M x 768 fp32 rows, 64 queries per call, COSINE

Ways:
  (y)   the yardstick: bbq_rerank_scores over each query's accepted rows - the list 0 .. n-1, or the filter's rows - and a stable
        descending sort of each query's scores on the host, first k; the row lists, offsets and score buffers are made once and reused
  (n)   bbq_vectors_search_batch
The bytes of (y) and (n) - rows and f64 scores - are compared on every leg before anything is timed.
Legs: k = 10 and k = 100, each without a filter, under a random filter that accepts 10 % of the rows, and under one that accepts 1 000
rows.  Per leg the ways run three times in alternation, each run the median of the timed calls (host clock around calls that return
with their results).  The claim per leg: the slowest of (n)'s three runs beats the fastest of (y)'s by more than (y)'s spread (its
slowest run minus its fastest)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "scripts"), os.path.join(ROOT, "better-binary-quantization_amd", "python")):
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--queries", type=int, default=64, help="queries per call")
    ap.add_argument("--true-sim", type=int, default=1)
    ap.add_argument("--steps", type=int, default=7, help="timed calls per run and way (at least 7)")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--runs", type=int, default=3, help="alternating runs per leg")
    ap.add_argument("--only-new", type=int, default=0, help="1: time the new call alone, unfiltered (for a kernel trace, or a size the yardstick cannot take)")
    ap.add_argument("--slab-rows", type=int, default=0, help="exact_slab_rows")
    ap.add_argument("--device", type=int, default=0)
    args = ap.parse_args()
    if args.steps < 7:
        raise SystemExit("bench_exact: a median of fewer than 7 calls is not reported")
    import torch  # noqa: F401  (first: one HIP runtime for torch and libbbq, as bench.py does)
    import bench
    import bbq_amd as B
    from bbq_amd import capi
    if B.device_count() < 1:
        raise SystemExit("bench_exact: no HIP device - nothing here can be measured without one")
    n, dim, nq, SIM = args.rows, args.dim, args.queries, args.true_sim
    rng = np.random.default_rng(73)
    ix = None
    if not args.only_new:  # the filters hang on an index of n rows; the search reads the fp32 rows alone
        codes, corr = bench.synth_rows(1, 0, n, (dim + 7) // 8)
        ix = B.Index(codes, corr, dim, float(B.centroid_dp(bench.synth_centroid(dim))), device=args.device, corrections="compact")
        del codes, corr
    V = None
    piece = 100_000
    for r0 in range(0, n, piece):  # embedding-like rows, appended piece by piece: the host never holds them all
        block = rng.standard_normal((min(piece, n - r0), dim), dtype=np.float32)
        if V is None:
            V = capi.Vectors(block, device=args.device)
        else:
            V.append(block)
    V.set_option("exact_slab_rows", args.slab_rows)
    print("bench_exact: %d x %d fp32 rows resident" % (n, dim), file=sys.stderr, flush=True)
    queries = np.ascontiguousarray(rng.standard_normal((nq, dim), dtype=np.float32))
    L = capi.lib()
    med = lambda t: float(np.median(t))  # noqa: E731

    res = {"metric": "exact_search_seconds_per_call", "rows": n, "dim": dim, "true_sim": SIM, "queries_per_call": nq, "exact_slab_rows": args.slab_rows,
           "timed_calls_per_run": args.steps, "runs_per_leg": args.runs, "legs": []}
    filters = (("none", None),) if args.only_new else (("none", None), ("random_10_percent", rng.random(n) < 0.1),
                                                       ("1000_rows", np.isin(np.arange(n), rng.choice(n, min(1000, n), replace=False))))
    for fname, accept in filters:
        flt = capi.Filter(ix, accept) if accept is not None else None
        rows = np.arange(n, dtype=np.int32) if accept is None else np.flatnonzero(accept).astype(np.int32)
        a = len(rows)
        if not args.only_new:  # the yardstick's lists and buffers, made once
            ords = np.ascontiguousarray(np.tile(rows, nq))
            ooff = (np.arange(nq + 1, dtype=np.int64) * a)
            c64 = np.empty(nq * a, np.float64)
        for k in (10, 100):
            kk = min(k, a)
            out = {w: (np.full((nq, k), -1, np.int32), np.zeros((nq, k), np.float64)) for w in "yn"}
            cnt = np.zeros(nq, np.int64)

            def way_n():
                t0 = time.perf_counter()
                rc = L.bbq_vectors_search_batch(V._h, flt._h if flt is not None else None, nq, queries.ctypes.data, SIM, k, out["n"][0].ctypes.data,
                                                out["n"][1].ctypes.data, cnt.ctypes.data)
                dt = time.perf_counter() - t0
                assert rc == 0, L.bbq_last_error().decode()
                return dt

            def way_y():
                t0 = time.perf_counter()
                rc = L.bbq_rerank_scores(V._h, nq, queries.ctypes.data, ooff.ctypes.data, ords.ctypes.data, SIM, c64.ctypes.data)
                assert rc == 0, L.bbq_last_error().decode()
                for q in range(nq):
                    s = c64[q * a:(q + 1) * a]
                    top = np.argsort(-s, kind="stable")[:kk]   # the rows are finite: no NaN; equal scores stay in row order
                    out["y"][0][q, :kk] = rows[top]
                    out["y"][1][q, :kk] = s[top]
                return time.perf_counter() - t0

            # the answers first: nothing is timed before the two ways agree
            way_n()
            assert (cnt == kk).all()
            if not args.only_new:
                way_y()
                assert out["y"][0].tobytes() == out["n"][0].tobytes() and out["y"][1].tobytes() == out["n"][1].tobytes(), \
                    "filter %s, k %d: the yardstick's bytes and the new call's differ" % (fname, k)
            ways = {"n": way_n} if args.only_new else {"y": way_y, "n": way_n}
            runs = {w: [] for w in ways}
            for r in range(args.runs):
                t = {w: [] for w in ways}
                for c in range(args.warmup + args.steps):  # interleaved: one call of every way per round
                    for w, f in ways.items():
                        dt = f()
                        if c >= args.warmup:
                            t[w].append(dt)
                for w in ways:
                    runs[w].append(med(t[w]))
            rec = {"filter": fname, "accepted_rows": a, "k": k, "pairs_per_call": nq * a, "fma_per_call": nq * a * dim,
                   "new_s_per_call_runs": [round(x, 6) for x in runs["n"]], "new_s_per_call": round(med(runs["n"]), 6),
                   "new_pairs_per_s": round(nq * a / med(runs["n"]), 1)}
            if not args.only_new:
                y_fast, y_slow, n_slow = min(runs["y"]), max(runs["y"]), max(runs["n"])
                rec.update({"yardstick_s_per_call_runs": [round(x, 6) for x in runs["y"]], "yardstick_s_per_call": round(med(runs["y"]), 6),
                            "new_speedup_over_yardstick": round(med(runs["y"]) / med(runs["n"]), 2),
                            "new_slowest_beats_yardstick_fastest_by_more_than_its_spread": bool(n_slow < y_fast - (y_slow - y_fast)),
                            "bytes_agree": True})
            res["legs"].append(rec)
            print("bench_exact: filter %s k %d done" % (fname, k), file=sys.stderr, flush=True)
        if flt is not None:
            flt.close()
    V.close()
    if ix is not None:
        ix.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
