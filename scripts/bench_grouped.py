#!/usr/bin/env python3
"""Grouped search at size: bbq_search_grouped_batch beside the two ways a caller had without it, for the same request, in one process,
the ways interleaved call by call so that drift of the box hits all alike.  Prints ONE JSON line (profiles/grouped_search.json).

  python scripts/bench_grouped.py                    # 1 M x 768 synthetic rows, compact layout, queryBits 4, 64 queries per call
  python scripts/bench_grouped.py --rows 10000000

Ways:
  new   bbq_search_grouped_batch, with the grid in both orders (option l2_share: -1 = a chunk's queries dispatched next to each other,
        1 = the plain order); the faster of the two is the leg's figure
  (a)   bbq_score_rows per query over all rows, the group maximum (numpy, a few passes over the scores) and the reference's heap on the host: the only exact way there was -
        the answers are compared bit for bit and the new call has to beat it
  (b)   bbq_search_batch / bbq_search_filtered_batch with k x 8 rows, collapsed by group on the host: not exact - reported with the
        share of queries it leaves short of k groups, as context; it prunes, so it is expected to be faster
Legs: groups of 1..16 rows (8.5 on average) and groups of 1 000 rows; k = 10 and 100; without a filter and under a random filter that
accepts 90 % of the rows.  Per leg the median of the timed calls (host clock around calls that return with their results).  The first
leg also runs the new call under each scratch budget of --scratch (option group_scratch_mb).  Recorded besides: the dominant launch
of a plain sweep of the same rows for the same queries (bbq_get_stats after bbq_search_batch) and an upper bound of the global atomics
per call, counted on the host from the offsets (two per chunk whose edge cuts a group, times the queries)."""
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

CHUNK = 512


def group_maxima(s32, accept, starts):
    """way (a)'s reduction on the host, for scores without a NaN: the greatest accepted score of every group that has an accepted row,
    in group order, and which non-empty group each belongs to (three passes over the scores at most)"""
    best = np.maximum.reduceat(s32 if accept is None else np.where(accept, s32, -np.inf), starts)
    live_at = np.flatnonzero(best > -np.inf)
    return best[live_at], live_at


def atomics_at_most(off, n, nq):
    edges = np.arange(CHUNK, n, CHUNK)
    cut = ~np.isin(edges, off)                       # a chunk edge inside a group: one atomic on either side of it
    per_chunk = np.zeros((n + CHUNK - 1) // CHUNK, np.int64)
    per_chunk[:-1] += cut
    per_chunk[1:] += cut
    g = np.searchsorted(off, np.arange(0, n, CHUNK), side="right")
    g_last = np.searchsorted(off, np.minimum(np.arange(0, n, CHUNK) + CHUNK, n) - 1, side="right")
    per_chunk -= (per_chunk == 2) & (g == g_last)    # one group over both edges: one atomic
    return int(per_chunk.sum()) * nq


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--queries", type=int, default=64, help="queries per call")
    ap.add_argument("--ks", default="10,100")
    ap.add_argument("--steps", type=int, default=7, help="timed calls per leg and way (at least 7)")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--scratch", default="64,128,256,512", help="MiB of scratch per sub-batch tried on the first leg")
    ap.add_argument("--only-new", type=int, default=0, help="1: time the grouped search alone (for a kernel trace)")
    ap.add_argument("--device", type=int, default=0)
    args = ap.parse_args()
    if args.steps < 7:
        raise SystemExit("bench_grouped: a median of fewer than 7 calls is not reported")
    import torch  # noqa: F401  (first: one HIP runtime for torch and libbbq, as bench.py does)
    import bench
    import orclib as O
    import bbq_amd as B
    from bbq_amd import capi
    if B.device_count() < 1:
        raise SystemExit("bench_grouped: no HIP device - nothing here can be measured without one")
    n, dim, QB, SIM, nq = args.rows, args.dim, 4, 1, args.queries
    codes, corr = bench.synth_rows(1, 0, n, (dim + 7) // 8)
    cdp = float(B.centroid_dp(bench.synth_centroid(dim)))
    print("bench_grouped: %d rows made" % n, file=sys.stderr, flush=True)
    ix = B.Index(codes, corr, dim, cdp, device=args.device, corrections="compact")
    del codes, corr
    print("bench_grouped: index resident", file=sys.stderr, flush=True)
    rng = np.random.default_rng(57)
    qq, qc = bench.synth_queries(2, nq, dim, QB)
    qq, qc = np.ascontiguousarray(qq, np.uint8), np.ascontiguousarray(qc, np.float64)
    L = capi.lib()
    med = lambda t: float(np.median(t))  # noqa: E731

    sizes = rng.integers(1, 17, n // 4)
    off_small = np.concatenate([[0], np.cumsum(sizes)])
    off_small = np.append(off_small[off_small < n], n).astype(np.int64)
    off_big = np.unique(np.append(np.arange(0, n, 1000), n)).astype(np.int64)
    layouts = {"groups_of_1_to_16": off_small, "groups_of_1000": off_big}

    ix.reset_stats()
    ix.search_batch(qq, qc, QB, SIM, 10)
    ix.search_batch(qq, qc, QB, SIM, 10)
    st = ix.stats()
    res = {"metric": "grouped_search_seconds_per_call", "rows": n, "dim": dim, "query_bits": QB, "queries_per_call": nq, "layout": "compact",
           "timed_calls_per_leg": args.steps, "bytes_per_row": ix.bytes_per_row,
           "plain_sweep_dominant_launch_ms": round(st["last_scan_ms"], 4), "plain_sweep_dominant_launch_rows": int(st["last_scan_rows"]), "legs": []}

    first = True
    for lname, off in layouts.items():
        for acc in (1.0, 0.9):
            accept = np.ones(n, np.bool_) if acc >= 1.0 else rng.random(n) < acc
            flt = None if acc >= 1.0 else capi.Filter(ix, accept)
            groups = capi.Groups(ix, off, flt)
            nonempty = np.nonzero(np.diff(off) > 0)[0]
            starts, ends = off[nonempty], off[nonempty + 1]
            for k in (int(x) for x in args.ks.split(",")):
                idx, grp, sc = np.ones((nq, k), np.int32), np.ones((nq, k), np.int32), np.ones((nq, k), np.float32)
                cnt, status = np.ones(nq, np.int64), np.ones(nq, np.uint8)

                def new_call():
                    t0 = time.perf_counter()
                    rc = L.bbq_search_grouped_batch(ix._h, groups._h, nq, qq.ctypes.data, qc.ctypes.data, QB, SIM, k, idx.ctypes.data, grp.ctypes.data,
                                                    sc.ctypes.data, cnt.ctypes.data, status.ctypes.data)
                    dt = time.perf_counter() - t0
                    assert rc == 0, L.bbq_last_error().decode()
                    return dt

                a_idx, a_sc = np.zeros((nq, k), np.int32), np.zeros((nq, k), np.float32)

                def way_a():
                    t0 = time.perf_counter()
                    for q in range(nq):
                        s32 = ix.score_rows(qq[q], qc[q], QB, SIM)[2]
                        best, live_at = group_maxima(s32, accept if flt is not None else None, starts)
                        oi, osc = O.heap_topk(best, k)
                        for j, g in enumerate(live_at[oi]):  # the k winners' rows: the first accepted row of the group that scores its maximum
                            b, e = starts[g], ends[g]
                            hit = s32[b:e] == osc[j]
                            if flt is not None:
                                hit &= accept[b:e]
                            a_idx[q, j] = b + int(np.argmax(hit))
                        a_sc[q, :len(oi)] = osc
                    return time.perf_counter() - t0

                short = [0]

                def way_b():
                    t0 = time.perf_counter()
                    bi, _, bc = ix.search_batch(qq, qc, QB, SIM, 8 * k) if flt is None else ix.search_filtered_batch(qq, qc, QB, SIM, 8 * k, flt)
                    short[0] = 0
                    for q in range(nq):
                        g = np.searchsorted(off, bi[q, :bc[q]], side="right") - 1
                        _, firsts = np.unique(g, return_index=True)
                        short[0] += len(firsts) < min(k, groups.live)
                    return time.perf_counter() - t0

                t = {w: [] for w in ("new_l2", "new_plain", "a", "b")}
                for c in range(args.warmup + args.steps):  # interleaved: one call of every way per round
                    d = {}
                    ix.set_option("l2_share", -1)
                    d["new_l2"] = new_call()
                    ix.set_option("l2_share", 1)
                    d["new_plain"] = new_call()
                    ix.set_option("l2_share", -1)
                    if not args.only_new:
                        d["a"], d["b"] = way_a(), way_b()
                    if c >= args.warmup:
                        for w, v in d.items():
                            t[w].append(v)
                new = min(med(t["new_l2"]), med(t["new_plain"]))
                rec = {"groups": lname, "n_groups": int(groups.count), "live_groups": int(groups.live), "filter_accepts": acc, "k": k,
                       "new_s_per_call_queries_of_a_chunk_adjacent": round(med(t["new_l2"]), 6), "new_s_per_call_plain_grid": round(med(t["new_plain"]), 6),
                       "new_s_per_call": round(new, 6), "new_rows_per_s": round(nq * n / new, 1), "status1_share": round(float(status.mean()), 4),
                       "global_atomics_per_call_at_most": atomics_at_most(off, n, nq)}
                if not args.only_new:
                    want = min(k, groups.live)
                    assert (cnt == want).all()
                    assert (idx[:, :want] == a_idx[:, :want]).all() and (sc[:, :want].view(np.uint32) == a_sc[:, :want].view(np.uint32)).all(), \
                        "%s accept %g k %d: the grouped search and the host's reduction differ" % (lname, acc, k)
                    rec.update({"score_rows_and_host_reduce_s_per_call": round(med(t["a"]), 6), "speedup_over_score_rows_and_host_reduce": round(med(t["a"]) / new, 2),
                                "faster_than_the_exact_way": bool(new < med(t["a"])), "answers_agree": True,
                                "overfetch_8k_s_per_call": round(med(t["b"]), 6), "overfetch_8k_share_of_queries_short_of_k_groups": round(short[0] / nq, 4)})
                if first:  # the scratch budget of a sub-batch, on the first leg alone
                    series = {}
                    for mb in (int(x) for x in args.scratch.split(",")):
                        ix.set_option("group_scratch_mb", mb)
                        ts = [new_call() for _ in range(args.warmup + args.steps)][args.warmup:]
                        series[str(mb)] = {"s_per_call": round(med(ts), 6), "queries_per_sub_batch": int(max(1, min(nq, (mb << 20) // (16 * groups.live))))}
                    ix.set_option("group_scratch_mb", 256)
                    rec["scratch_mb_series"] = series
                    first = False
                res["legs"].append(rec)
                print("bench_grouped: %s accept %g k %d: %.6f s per call" % (lname, acc, k, new), file=sys.stderr, flush=True)
            groups.close()
            if flt is not None:
                flt.close()
    ix.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
