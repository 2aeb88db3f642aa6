#!/usr/bin/env python3
"""Filtered span search at size: bbq_search_spans_filtered_batch beside what a caller had without it - bbq_search_ords_batch over the
accepted ords of the spans, and one bbq_filter of (filter AND spans) plus one filtered call per query - and beside bbq_search_spans_batch
on the same spans without a filter (against the all-ones filter: the price of the filter path itself), for the same request, in one
process, the ways interleaved call by call so that drift of the box hits all alike.  Prints ONE JSON line
(profiles/span_filtered_search.json).

  python scripts/bench_spans_filtered.py                 # 10 M x 768 synthetic rows, compact layout, queryBits 4, k = 100, 64 queries per call
  python scripts/bench_spans_filtered.py --rows 2000000 --steps 5

Legs: the span legs of bench_spans.py - 16 spans per query totalling 0.1 % / 1 % / 10 % of the rows, and one contiguous 1 % block per
query; every query has spans of its own - each under a random row filter accepting 100 % / 90 % / 50 % / 1 % of the rows.  The row filter
is resident (a store's deletions or a tenant: made once, not part of a request); the (filter AND spans) filters of the per-query way are
part of the request and their creation is timed, separately.  Per leg: seconds per call (host clock around calls that return with their
results; the median of the timed calls, and the slowest) for each way, the share of queries the host had to replay (out_status 1), the
answers compared bit for bit, and whether the new call is faster than the better of the two ways there were.  All sides write into host
buffers that are allocated and touched once (the C ABI called directly)."""
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

from bench_spans import draw_spans  # noqa: E402


def same_bits(a, b):
    return (a.view(np.uint32 if a.dtype == np.float32 else a.dtype) == b.view(np.uint32 if b.dtype == np.float32 else b.dtype)).all()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--queries", type=int, default=64, help="queries per call")
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--steps", type=int, default=7, help="timed calls per leg and way (at least 5)")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--legs", default="16:0.001,16:0.01,16:0.1,1:0.01", help="spans per query : share of the rows")
    ap.add_argument("--accept", default="1.0,0.9,0.5,0.01", help="share of the rows the random filter accepts")
    ap.add_argument("--only-new", type=int, default=0, help="1: time the filtered span search alone (for a kernel trace)")
    ap.add_argument("--device", type=int, default=0)
    args = ap.parse_args()
    if args.steps < 5:
        raise SystemExit("bench_spans_filtered: a median of fewer than 5 calls is not reported")
    import torch  # noqa: F401  (first: one HIP runtime for torch and libbbq, as bench.py does)
    import bench
    import bbq_amd as B
    from bbq_amd import capi
    if B.device_count() < 1:
        raise SystemExit("bench_spans_filtered: no HIP device - nothing here can be measured without one")
    n, dim, QB, SIM, k, nq = args.rows, args.dim, 4, 1, args.k, args.queries
    codes, corr = bench.synth_rows(1, 0, n, (dim + 7) // 8)
    cdp = float(B.centroid_dp(bench.synth_centroid(dim)))
    ix = B.Index(codes, corr, dim, cdp, device=args.device, corrections="compact")
    rng = np.random.default_rng(53)
    qq, qc = bench.synth_queries(2, nq, dim, QB)
    qq, qc = np.ascontiguousarray(qq, np.uint8), np.ascontiguousarray(qc, np.float64)
    L = capi.lib()
    ways = ("new", "spans", "ords", "filtered")
    out = {w: (np.ones((nq, k), np.int32), np.ones((nq, k), np.float32), np.ones(nq, np.int64)) for w in ways}
    status = {w: np.ones(nq, np.uint8) for w in ("new", "spans")}

    def by_spans(way, flt, off, flat):
        i, s, c = out[way]
        st = status[way]
        t0 = time.perf_counter()
        if flt is None:
            rc = L.bbq_search_spans_batch(ix._h, nq, qq.ctypes.data, qc.ctypes.data, QB, SIM, k, off.ctypes.data, flat.ctypes.data, i.ctypes.data,
                                          s.ctypes.data, c.ctypes.data, st.ctypes.data)
        else:
            rc = L.bbq_search_spans_filtered_batch(ix._h, flt._h, nq, qq.ctypes.data, qc.ctypes.data, QB, SIM, k, off.ctypes.data, flat.ctypes.data,
                                                   i.ctypes.data, s.ctypes.data, c.ctypes.data, st.ctypes.data)
        dt = time.perf_counter() - t0
        assert rc == 0, L.bbq_last_error().decode()
        return dt

    def by_ords(ooff, ords):
        i, s, c = out["ords"]
        t0 = time.perf_counter()
        rc = L.bbq_search_ords_batch(ix._h, nq, qq.ctypes.data, qc.ctypes.data, QB, SIM, k, ooff.ctypes.data, ords.ctypes.data, i.ctypes.data, s.ctypes.data, c.ctypes.data)
        dt = time.perf_counter() - t0
        assert rc == 0, L.bbq_last_error().decode()
        return dt

    def by_filters(masks):
        """one filter of (filter AND spans) and one filtered call per query; returns (seconds in all, seconds inside the filtered calls)"""
        i, s, c = out["filtered"]
        t0 = time.perf_counter()
        inside = 0.0
        for q in range(nq):
            with capi.Filter(ix, masks[q]) as flt:
                t1 = time.perf_counter()
                rc = L.bbq_search_filtered_batch(ix._h, flt._h, 1, qq[q].ctypes.data, qc[q].ctypes.data, QB, SIM, k, i[q].ctypes.data, s[q].ctypes.data, c[q:].ctypes.data)
                inside += time.perf_counter() - t1
                assert rc == 0, L.bbq_last_error().decode()
        return time.perf_counter() - t0, inside

    res = {"metric": "span_filtered_search_seconds_per_call", "rows": n, "dim": dim, "query_bits": QB, "k": k, "queries_per_call": nq, "layout": "compact",
           "timed_calls_per_leg": args.steps, "bytes_per_row": ix.bytes_per_row, "legs": []}
    med = lambda t: float(np.median(t))  # noqa: E731
    for leg in args.legs.split(","):
        m, share = int(leg.split(":")[0]), float(leg.split(":")[1])
        total = int(n * share)
        lists = [draw_spans(rng, n, m, total) for _ in range(nq)]
        off = np.arange(nq + 1, dtype=np.int64) * m
        flat = np.ascontiguousarray(np.concatenate(lists), np.int64)
        for acc in (float(a) for a in args.accept.split(",")):
            accept = np.ones(n, np.bool_) if acc >= 1.0 else rng.random(n) < acc
            flt = capi.Filter(ix, accept)
            t = {w: [] for w in ("new", "spans", "ords", "filtered", "filtered_inside")}
            if not args.only_new:
                per_query = [np.concatenate([np.arange(b, e, dtype=np.int32)[accept[b:e]] for b, e in sp]) for sp in lists]
                ooff = np.concatenate([[0], np.cumsum([len(o) for o in per_query])]).astype(np.int64)
                ords = np.ascontiguousarray(np.concatenate(per_query), np.int32)
                masks = np.zeros((nq, n), np.bool_)
                for q, sp in enumerate(lists):
                    for b, e in sp:
                        masks[q, b:e] = accept[b:e]
            for c in range(args.warmup + args.steps):  # interleaved: one call of every way per round
                d = {"new": by_spans("new", flt, off, flat)}
                if not args.only_new:
                    d["spans"] = by_spans("spans", None, off, flat)
                    d["ords"] = by_ords(ooff, ords)
                    d["filtered"], d["filtered_inside"] = by_filters(masks)
                if c >= args.warmup:
                    for w, v in d.items():
                        t[w].append(v)
            rec = {"spans_per_query": m, "share_of_rows": share, "rows_per_query": total, "filter_accepts": acc, "filter_count": flt.count,
                   "new_s_per_call": round(med(t["new"]), 6), "new_s_per_call_max": round(max(t["new"]), 6),
                   "new_visited_rows_per_s": round(nq * total / med(t["new"]), 1), "status1_share": round(float(status["new"].mean()), 4)}
            if not args.only_new:
                want_n = np.minimum(k, np.diff(ooff))
                assert (out["new"][2] == want_n).all(), "%s accept %g: answer lengths" % (leg, acc)
                for w in ("ords", "filtered"):  # the three ways agree, bit for bit, over the rows each answer holds
                    assert (out[w][2] == want_n).all(), "%s accept %g: answer lengths of the %s way" % (leg, acc, w)
                    for q in range(nq):
                        for a, b in zip(out["new"][:2], out[w][:2]):
                            assert same_bits(a[q, :want_n[q]], b[q, :want_n[q]]), "%s accept %g: the filtered span search and the %s way differ" % (leg, acc, w)
                if acc >= 1.0:
                    assert all(same_bits(a, b) for a, b in zip(out["new"], out["spans"])) and (status["new"] == status["spans"]).all()
                better = min(med(t["ords"]), med(t["filtered"]))
                rec.update({"spans_unfiltered_s_per_call": round(med(t["spans"]), 6), "ords_s_per_call": round(med(t["ords"]), 6),
                            "filtered_s_per_call": round(med(t["filtered"]), 6),
                            "filtered_s_per_call_without_filter_creation": round(med(t["filtered_inside"]), 6),
                            "new_over_spans_unfiltered": round(med(t["new"]) / med(t["spans"]), 3),
                            "speedup_over_ords": round(med(t["ords"]) / med(t["new"]), 2),
                            "speedup_over_filtered": round(med(t["filtered"]) / med(t["new"]), 2),
                            "speedup_over_filtered_without_filter_creation": round(med(t["filtered_inside"]) / med(t["new"]), 2),
                            "faster_than_the_better_earlier_way": bool(med(t["new"]) < better),
                            "faster_than_both_even_without_filter_creation": bool(med(t["new"]) < min(med(t["ords"]), med(t["filtered_inside"]))),
                            "answers_agree": True})
                del ords, masks, per_query
            flt.close()
            res["legs"].append(rec)
    ix.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
