#!/usr/bin/env python3
"""Filtered search at size: q/s of bbq_search_filtered_batch against bbq_search_batch on the same index, in one process, the legs
interleaved call by call so that drift of the box hits all of them alike.  Prints ONE JSON line (profiles/filtered_search.json).

  python scripts/bench_filtered.py                 # 10 M x 768 synthetic rows, queryBits 4, k = 100, 256 queries per call
  python scripts/bench_filtered.py --rows 2000000 --steps 6 --check 1
  python scripts/bench_filtered.py --sweep-share 32   # every leg, the unfiltered one too, on the matrix-core shared sweep (profiles/filtered_search_shared.json)

Legs: (a) unfiltered, (b) all-ones filter = the cost of the mechanism, (c) random filters at 50 / 10 / 1 / 0.1 %, (d) a contiguous 10 %
block at the end of the index, (e) 1000 random rows.  Per leg: q/s (host clock around calls that return with their answers), the
call's dense_fallbacks and host_replays, the dominant launch's hipEvent time and rows (bbq_stats), and the share of 64-row tiles and
512-row chunks that hold an accepted row (an empty tile is not loaded at all).  --check N holds the first N queries of every filtered
leg to the oracle's heap over the accepted rows (CPU, ~10 s per query at 10 M rows)."""
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
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--queries", type=int, default=256, help="queries per call")
    ap.add_argument("--steps", type=int, default=8, help="timed calls per leg")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--check", type=int, default=1, help="queries per filtered leg held to the oracle (0: none)")
    ap.add_argument("--legs", default="", help="comma-separated subset of the legs (default: all), e.g. unfiltered,all_ones for a profiler run")
    ap.add_argument("--sweep-share", type=int, default=1, choices=(1, 32), help="the index's sweep_share option for every leg (1: the per-query sweeps)")
    ap.add_argument("--device", type=int, default=0)
    args = ap.parse_args()
    import torch  # noqa: F401  (first: one HIP runtime for torch and libbbq, as bench.py does)
    import bench
    import bbq_amd as B
    from bbq_amd import capi
    if B.device_count() < 1:
        raise SystemExit("bench_filtered: no HIP device - nothing here can be measured without one")
    n, dim, k, Q, QB, SIM = args.rows, args.dim, args.k, args.queries, 4, 1
    codes, corr = bench.synth_rows(1, 0, n, (dim + 7) // 8)
    cdp = float(B.centroid_dp(bench.synth_centroid(dim)))
    ix = B.Index(codes, corr, dim, cdp, device=args.device)
    if args.sweep_share != 1:
        ix.set_option("sweep_share", args.sweep_share)
    rng = np.random.default_rng(41)
    masks = {"all_ones": np.ones(n, bool)}
    for name, share in (("random_50pct", 0.5), ("random_10pct", 0.1), ("random_1pct", 0.01), ("random_0.1pct", 0.001)):
        masks[name] = rng.random(n) < share
    masks["block_last_10pct"] = np.arange(n) >= n - n // 10
    masks["rows_1000"] = np.zeros(n, bool)
    masks["rows_1000"][rng.choice(n, min(1000, n), replace=False)] = True
    if args.legs:
        masks = {name: m for name, m in masks.items() if name in args.legs.split(",")}
    filters = {name: capi.Filter(ix, m) for name, m in masks.items()}
    legs = ["unfiltered"] + list(masks)
    calls = args.warmup + args.steps
    qq_all, qc_all = bench.synth_queries(2, calls * Q, dim, QB)

    def run(leg, c):
        qq, qc = qq_all[c * Q:(c + 1) * Q], qc_all[c * Q:(c + 1) * Q]
        t0 = time.perf_counter()
        out = ix.search_batch(qq, qc, QB, SIM, k) if leg == "unfiltered" else ix.search_filtered_batch(qq, qc, QB, SIM, k, filters[leg])
        return time.perf_counter() - t0, out

    seconds = {leg: 0.0 for leg in legs}
    stats = {leg: {"dense_fallbacks": 0, "host_replays": 0, "scan_ms": [], "scan_rows": 0} for leg in legs}
    first = {}
    for c in range(calls):  # interleaved: one call of every leg per round
        for leg in legs:
            dt, out = run(leg, c)
            if c < args.warmup:
                continue
            seconds[leg] += dt
            st = ix.stats()
            s = stats[leg]
            s["dense_fallbacks"] += st["dense_fallbacks"]
            s["host_replays"] += st["host_replays"]
            s["scan_ms"].append(st["last_scan_ms"])
            s["scan_rows"] = st["last_scan_rows"]
            if c == args.warmup:
                first[leg] = out
    checked = 0
    if args.check > 0:
        import orclib as O
        c = args.warmup
        for qi in range(min(args.check, Q)):
            s32 = O.score_all(codes, corr, dim, qq_all[c * Q + qi], qc_all[c * Q + qi], QB, SIM, cdp)[2]
            for leg in legs:
                acc = np.arange(n) if leg == "unfiltered" else np.flatnonzero(masks[leg])
                pos, sc = O.heap_topk(s32[acc], k)
                idx, got, cnt = first[leg]
                assert cnt[qi] == pos.shape[0] and (idx[qi, :cnt[qi]] == acc[pos]).all() and \
                    (got[qi, :cnt[qi]].view(np.uint32) == sc.view(np.uint32)).all(), "%s: query %d differs from the oracle" % (leg, qi)
                checked += 1
    res = {"metric": "filtered_search_qps", "rows": n, "dim": dim, "k": k, "query_bits": QB, "queries_per_call": Q, "timed_calls_per_leg": args.steps,
           "bytes_per_row": ix.bytes_per_row, "answers_checked_against_oracle": checked, "legs": {}}
    if args.sweep_share != 1:
        res["sweep_share"] = args.sweep_share
    base = args.steps * Q / seconds["unfiltered"]
    for leg in legs:
        s = stats[leg]
        qps = args.steps * Q / seconds[leg]
        rec = {"qps": round(qps, 1), "vs_unfiltered": round(qps / base, 4), "dense_fallbacks": s["dense_fallbacks"], "host_replays": s["host_replays"],
               "dominant_launch_ms_median": round(float(np.median(s["scan_ms"])), 4), "dominant_launch_rows_x_queries": int(s["scan_rows"])}
        if leg != "unfiltered":
            m = masks[leg]
            pad = np.zeros((n + 511) // 512 * 512, bool)
            pad[:n] = m
            rec.update(accepted=int(m.sum()), nonempty_tile_share=round(float(pad.reshape(-1, 64).any(axis=1).mean()), 5),
                       nonempty_chunk_share=round(float(pad.reshape(-1, 512).any(axis=1).mean()), 5))
        res["legs"][leg] = rec
    for f in filters.values():
        f.close()
    ix.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
