#!/usr/bin/env python3
"""Range search with the count pass on the matrix-core shared sweep (sweep_share 32) beside the per-query count (sweep_share 1) - the
same handle, the same request, in one process, the two ways interleaved call by call so that drift of the box hits both alike.  Prints
ONE JSON line (profiles/range_search_shared.json).

  python scripts/bench_range_shared.py                 # 1 M x 768 synthetic rows, compact layout, queryBits 4
  python scripts/bench_range_shared.py --rows 10000000 --queries 64

Legs: thresholds at each query's 100th-best score, at 0.1 % and at 10 % of the rows; 1, 8, 32, 64 and 256 queries per call; no filter, a
random 50 % and a random 1 % filter; bbq_count_range_batch alone and bbq_search_range_batch.  Per leg and way: three runs, each the
median of `--steps` calls (host clock around calls that return with their results), the runs of the two ways alternating.  A leg is a win
for a way when the slowest of its three runs beats the other way's fastest by more than the other way's spread; every leg is reported.
The counts of the two ways are compared, exactly."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--queries", default="1,8,32,64,256", help="queries per call")
    ap.add_argument("--steps", type=int, default=7, help="timed calls per run")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--filters", default="0,0.5,0.01", help="share of the rows a random filter accepts (0: no filter)")
    ap.add_argument("--device", type=int, default=0)
    args = ap.parse_args()
    import torch  # noqa: F401  (first: one HIP runtime for torch and libbbq, as bench.py does)
    import bench
    import bbq_amd as B
    from bbq_amd import capi
    if B.device_count() < 1:
        raise SystemExit("bench_range_shared: no HIP device - nothing here can be measured without one")
    n, dim, QB, SIM = args.rows, args.dim, 4, 1
    counts_nq = [int(x) for x in args.queries.split(",")]
    codes, corr = bench.synth_rows(1, 0, n, (dim + 7) // 8)
    cdp = float(B.centroid_dp(bench.synth_centroid(dim)))
    ix = B.Index(codes, corr, dim, cdp, device=args.device, corrections="compact")
    qq, qc = bench.synth_queries(2, max(counts_nq), dim, QB)
    qq, qc = np.ascontiguousarray(qq, np.uint8), np.ascontiguousarray(qc, np.float64)
    ranks = {"100th_best": 100, "0.1_percent": max(1, n // 1000), "10_percent": max(1, n // 10)}
    ths = {name: np.zeros(len(qq), np.float32) for name in ranks}
    for q in range(len(qq)):  # every query's thresholds from its dense device scores
        s32 = ix.score_rows(qq[q], qc[q], QB, SIM)[2]
        for name, r in ranks.items():
            ths[name][q] = np.partition(s32, n - r)[n - r]
    L = capi.lib()
    rng = np.random.default_rng(53)

    def timed(fn):
        t0 = time.perf_counter()
        fn()
        return time.perf_counter() - t0

    res = {"metric": "range_search_seconds_per_call", "rows": n, "dim": dim, "query_bits": QB, "layout": "compact", "timed_calls_per_run": args.steps,
           "runs": args.runs, "legs": []}
    for share_of_rows in [float(x) for x in args.filters.split(",")]:
        flt = capi.Filter(ix, rng.random(n) < share_of_rows) if share_of_rows else None
        fh = flt._h if flt is not None else None
        for name in ranks:
            for nq in counts_nq:
                th = np.ascontiguousarray(ths[name][:nq])
                cnt = {w: np.zeros(nq, np.int64) for w in (32, 1)}

                def count(w):
                    rc = L.bbq_count_range_batch(ix._h, fh, nq, qq.ctypes.data, qc.ctypes.data, QB, SIM, th.ctypes.data, cnt[w].ctypes.data)
                    assert rc == 0, L.bbq_last_error().decode()

                count(1)
                cap = int(cnt[1].sum())
                off, oi, osc = np.zeros(nq + 1, np.int64), np.zeros(max(cap, 1), np.int32), np.zeros(max(cap, 1), np.float32)

                def search(w):
                    rc = L.bbq_search_range_batch(ix._h, fh, nq, qq.ctypes.data, qc.ctypes.data, QB, SIM, th.ctypes.data, cap, off.ctypes.data, oi.ctypes.data,
                                                  osc.ctypes.data)
                    assert rc == 0, L.bbq_last_error().decode()

                rec = {"filter": share_of_rows, "threshold": name, "queries_per_call": nq, "entries": cap}
                for what, call in (("count", count), ("search", search)):
                    runs = {32: [], 1: []}
                    for _ in range(args.runs):  # alternating runs, each the median of `steps` calls behind one warm-up call
                        for w in (32, 1):
                            ix.set_option("sweep_share", w)
                            call(w)
                            runs[w].append(float(np.median([timed(lambda: call(w)) for _ in range(args.steps)])))
                    assert (cnt[32] == cnt[1]).all(), "%s: the two ways count differently" % rec
                    a, b = runs[32], runs[1]
                    verdict = "shared" if max(a) < min(b) - (max(b) - min(b)) else "per_query" if max(b) < min(a) - (max(a) - min(a)) else "none"
                    rec[what] = {"shared_s": [round(x, 6) for x in a], "per_query_s": [round(x, 6) for x in b],
                                 "ratio_of_medians": round(float(np.median(b) / np.median(a)), 2), "win": verdict}
                res["legs"].append(rec)
        if flt is not None:
            flt.close()
    ix.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
