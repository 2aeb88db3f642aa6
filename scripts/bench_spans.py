#!/usr/bin/env python3
"""Span search at size: bbq_search_spans_batch beside the two ways a caller had without it - bbq_search_ords_batch over the spans
expanded into ords, and one bbq_filter plus one filtered call per query - for the same request, in one process, the three interleaved
call by call so that drift of the box hits all alike.  Prints ONE JSON line (profiles/span_search.json).

  python scripts/bench_spans.py                 # 10 M x 768 synthetic rows, compact layout, queryBits 4, k = 100, 64 queries per call
  python scripts/bench_spans.py --rows 2000000 --steps 2

Legs: 16 spans per query totalling 0.1 % / 1 % / 10 % of the rows, and one contiguous 1 % block per query; every query has spans of its
own.  Per leg: seconds per call (host clock around calls that return with their results; the median of the timed calls, and the
slowest) for each way, the share of queries the host had to replay (out_status 1), and the three answers compared bit for bit.  The
filtered way is timed with and without the creation of its filters (a filter per query is part of the request: it differs from query to
query).  All sides write into host buffers that are allocated and touched once (the C ABI called directly)."""
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


def draw_spans(rng, n, m, total):
    """m ascending disjoint spans of `total` rows in all, spread over an index of n rows"""
    lens = np.full(m, total // m, np.int64)
    lens[:total - int(lens.sum())] += 1
    gaps = rng.multinomial(n - total, np.ones(m + 1) / (m + 1))
    begin = np.cumsum(gaps[:m]) + np.concatenate([[0], np.cumsum(lens)[:-1]])
    return np.stack([begin, begin + lens], 1).astype(np.int64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--queries", type=int, default=64, help="queries per call")
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--steps", type=int, default=5, help="timed calls per leg and way")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--legs", default="16:0.001,16:0.01,16:0.1,1:0.01", help="spans per query : share of the rows")
    ap.add_argument("--only-spans", type=int, default=0, help="1: time the span search alone (for a kernel trace)")
    ap.add_argument("--device", type=int, default=0)
    args = ap.parse_args()
    import torch  # noqa: F401  (first: one HIP runtime for torch and libbbq, as bench.py does)
    import bench
    import bbq_amd as B
    from bbq_amd import capi
    if B.device_count() < 1:
        raise SystemExit("bench_spans: no HIP device - nothing here can be measured without one")
    n, dim, QB, SIM, k, nq = args.rows, args.dim, 4, 1, args.k, args.queries
    codes, corr = bench.synth_rows(1, 0, n, (dim + 7) // 8)
    cdp = float(B.centroid_dp(bench.synth_centroid(dim)))
    ix = B.Index(codes, corr, dim, cdp, device=args.device, corrections="compact")
    rng = np.random.default_rng(47)
    qq, qc = bench.synth_queries(2, nq, dim, QB)
    qq, qc = np.ascontiguousarray(qq, np.uint8), np.ascontiguousarray(qc, np.float64)
    L = capi.lib()
    out = {w: (np.ones((nq, k), np.int32), np.ones((nq, k), np.float32), np.ones(nq, np.int64)) for w in ("spans", "ords", "filtered")}
    status = np.ones(nq, np.uint8)

    def by_spans(off, flat):
        i, s, c = out["spans"]
        t0 = time.perf_counter()
        rc = L.bbq_search_spans_batch(ix._h, nq, qq.ctypes.data, qc.ctypes.data, QB, SIM, k, off.ctypes.data, flat.ctypes.data, i.ctypes.data, s.ctypes.data,
                                      c.ctypes.data, status.ctypes.data)
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
        """one filter and one filtered call per query; returns (seconds in all, seconds inside the filtered calls)"""
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

    res = {"metric": "span_search_seconds_per_call", "rows": n, "dim": dim, "query_bits": QB, "k": k, "queries_per_call": nq, "layout": "compact",
           "timed_calls_per_leg": args.steps, "bytes_per_row": ix.bytes_per_row, "legs": []}
    for leg in args.legs.split(","):
        m, share = int(leg.split(":")[0]), float(leg.split(":")[1])
        total = int(n * share)
        lists = [draw_spans(rng, n, m, total) for _ in range(nq)]
        off = np.arange(nq + 1, dtype=np.int64) * m
        flat = np.ascontiguousarray(np.concatenate(lists), np.int64)
        t_sp, t_or, t_fl, t_fi = [], [], [], []
        if not args.only_spans:
            ords = np.ascontiguousarray(np.concatenate([np.arange(b, e, dtype=np.int32) for sp in lists for b, e in sp]))
            ooff = np.arange(nq + 1, dtype=np.int64) * total
            masks = np.zeros((nq, n), np.bool_)
            for q, sp in enumerate(lists):
                for b, e in sp:
                    masks[q, b:e] = True
        for c in range(args.warmup + args.steps):  # interleaved: one call of every way per round
            d_sp = by_spans(off, flat)
            if not args.only_spans:
                d_or = by_ords(ooff, ords)
                d_fl, d_fi = by_filters(masks)
            if c >= args.warmup:
                t_sp.append(d_sp)
                if not args.only_spans:
                    t_or.append(d_or), t_fl.append(d_fl), t_fi.append(d_fi)
        rec = {"spans_per_query": m, "share_of_rows": share, "rows_per_query": total, "spans_s_per_call": round(float(np.median(t_sp)), 6),
               "spans_s_per_call_max": round(max(t_sp), 6), "spans_rows_per_s": round(nq * total / float(np.median(t_sp)), 1),
               "status1_share": round(float(status.mean()), 4)}
        if not args.only_spans:
            for w in ("ords", "filtered"):  # the three ways agree, bit for bit
                for a, b in zip(out["spans"], out[w]):
                    assert (a.view(np.uint32 if a.dtype == np.float32 else a.dtype) == b.view(np.uint32 if b.dtype == np.float32 else b.dtype)).all(), \
                        "%s: the span search and the %s way differ" % (leg, w)
            assert (out["spans"][2] == min(k, total)).all()
            rec.update({"ords_s_per_call": round(float(np.median(t_or)), 6), "filtered_s_per_call": round(float(np.median(t_fl)), 6),
                        "filtered_s_per_call_without_filter_creation": round(float(np.median(t_fi)), 6),
                        "speedup_over_ords": round(float(np.median(t_or)) / float(np.median(t_sp)), 2),
                        "speedup_over_filtered": round(float(np.median(t_fl)) / float(np.median(t_sp)), 2), "answers_agree": True})
            del ords, masks
        res["legs"].append(rec)
    ix.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
