#!/usr/bin/env python3
"""MaxSim search at size: bbq_search_maxsim_batch under both score paths beside the only exact way a caller had without it, for the same
request, in one process, the ways interleaved call by call so that drift of the box hits all alike.  Prints ONE JSON line
(profiles/maxsim_search.json).

  python scripts/bench_maxsim.py                     # 1 M x 768 synthetic rows, compact layout, queryBits 4, 16 queries of 32 tokens per call

Ways:
  (a)   bbq_score_rows per token vector over all rows, the group maxima (numpy), bbq_maxsim_reduce and the reference's heap on the host
  (b)   bbq_search_maxsim_batch with maxsim_fused 0: the grouped search's score kernel, every token vector one of its queries
  (c)   bbq_search_maxsim_batch with maxsim_fused 1: the fused score kernel, a tile loaded once for all tokens of a query's block
The answers of the three ways are compared byte for byte on every leg.
Legs: groups of 1..16 rows (8.5 on average) and groups of 1 000 rows; k = 10 and 100; without a filter and under a random filter that
accepts 90 % of the rows.  Per leg, (b) and (c) run three times in alternation, each run the median of the timed calls (host clock around
calls that return with their results); (a) is timed in the first run only.  The rule for maxsim_fused -1: fused only if on EVERY leg the
slowest of (c)'s three runs beats the fastest of (b)'s by more than (b)'s spread (its slowest run minus its fastest)."""
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
    ap.add_argument("--queries", type=int, default=16, help="queries per call")
    ap.add_argument("--tokens", type=int, default=32, help="token vectors per query")
    ap.add_argument("--ks", default="10,100")
    ap.add_argument("--steps", type=int, default=7, help="timed calls per run and way (at least 7)")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--runs", type=int, default=3, help="alternating runs of (b) and (c) per leg")
    ap.add_argument("--skip-a", type=int, default=0, help="1: time the two score paths alone (for a kernel trace)")
    ap.add_argument("--device", type=int, default=0)
    args = ap.parse_args()
    if args.steps < 7:
        raise SystemExit("bench_maxsim: a median of fewer than 7 calls is not reported")
    import torch  # noqa: F401  (first: one HIP runtime for torch and libbbq, as bench.py does)
    import bench
    import orclib as O
    import bbq_amd as B
    from bbq_amd import capi
    if B.device_count() < 1:
        raise SystemExit("bench_maxsim: no HIP device - nothing here can be measured without one")
    n, dim, QB, SIM, nq, T = args.rows, args.dim, 4, 1, args.queries, args.tokens
    codes, corr = bench.synth_rows(1, 0, n, (dim + 7) // 8)
    cdp = float(B.centroid_dp(bench.synth_centroid(dim)))
    print("bench_maxsim: %d rows made" % n, file=sys.stderr, flush=True)
    ix = B.Index(codes, corr, dim, cdp, device=args.device, corrections="compact")
    del codes, corr
    print("bench_maxsim: index resident", file=sys.stderr, flush=True)
    rng = np.random.default_rng(58)
    nv = nq * T
    qq, qc = bench.synth_queries(2, nv, dim, QB)
    qq, qc = np.ascontiguousarray(qq, np.uint8), np.ascontiguousarray(qc, np.float64)
    voff = (np.arange(nq + 1, dtype=np.int64) * T)
    L = capi.lib()
    med = lambda t: float(np.median(t))  # noqa: E731

    sizes = rng.integers(1, 17, n // 4)
    off_small = np.concatenate([[0], np.cumsum(sizes)])
    off_small = np.append(off_small[off_small < n], n).astype(np.int64)
    off_big = np.unique(np.append(np.arange(0, n, 1000), n)).astype(np.int64)
    layouts = {"groups_of_1_to_16": off_small, "groups_of_1000": off_big}

    res = {"metric": "maxsim_search_seconds_per_call", "rows": n, "dim": dim, "query_bits": QB, "queries_per_call": nq, "tokens_per_query": T,
           "token_block": capi.maxsim_token_block(), "layout": "compact", "timed_calls_per_run": args.steps, "runs_per_leg": args.runs,
           "bytes_per_row": ix.bytes_per_row, "legs": []}
    fused_wins_everywhere = True
    for lname, off in layouts.items():
        for acc in (1.0, 0.9):
            accept = np.ones(n, np.bool_) if acc >= 1.0 else rng.random(n) < acc
            flt = None if acc >= 1.0 else capi.Filter(ix, accept)
            groups = capi.Groups(ix, off, flt)
            nonempty = np.nonzero(np.diff(off) > 0)[0]
            starts = off[nonempty]
            for k in (int(x) for x in args.ks.split(",")):
                out = {w: (np.ones((nq, k), np.int32), np.ones((nq, k), np.float32), np.ones(nq, np.int64), np.ones(nq, np.uint8)) for w in "abc"}

                def device_call(way):
                    grp, sc, cnt, status = out[way]
                    ix.set_option("maxsim_fused", 0 if way == "b" else 1)
                    t0 = time.perf_counter()
                    rc = L.bbq_search_maxsim_batch(ix._h, groups._h, nq, voff.ctypes.data, qq.ctypes.data, qc.ctypes.data, QB, SIM, k, grp.ctypes.data,
                                                   sc.ctypes.data, cnt.ctypes.data, status.ctypes.data)
                    dt = time.perf_counter() - t0
                    assert rc == 0, L.bbq_last_error().decode()
                    return dt

                def way_a():
                    grp, sc, cnt, _ = out["a"]
                    t0 = time.perf_counter()
                    for q in range(nq):
                        rep = None
                        for t in range(T):
                            v = q * T + t
                            s32 = ix.score_rows(qq[v], qc[v], QB, SIM)[2]
                            best = np.maximum.reduceat(s32 if flt is None else np.where(accept, s32, -np.inf), starts)
                            if rep is None:
                                live_at = np.flatnonzero(best > -np.inf)      # the same for every token
                                rep = np.zeros((T, len(live_at)), np.float32)
                            rep[t] = best[live_at]
                        S = capi.maxsim_reduce(rep)
                        oi, osc = O.heap_topk(S, k)
                        cnt[q] = len(oi)
                        grp[q, :len(oi)] = nonempty[live_at[oi]]
                        sc[q, :len(oi)] = osc
                    return time.perf_counter() - t0

                runs = {"b": [], "c": []}
                t_a = []
                for r in range(args.runs):
                    t = {"b": [], "c": [], "a": []}
                    for c in range(args.warmup + args.steps):  # interleaved: one call of every way per round
                        d = {"b": device_call("b"), "c": device_call("c")}
                        if r == 0 and not args.skip_a:
                            d["a"] = way_a()
                        if c >= args.warmup:
                            for w, v in d.items():
                                t[w].append(v)
                    runs["b"].append(med(t["b"]))
                    runs["c"].append(med(t["c"]))
                    if t["a"]:
                        t_a = t["a"]
                ix.set_option("maxsim_fused", -1)
                want = min(k, groups.live)
                ways = "bc" if args.skip_a else "abc"
                for w in ways:
                    assert (out[w][2] == want).all()
                    assert out[w][0][:, :want].tobytes() == out["b"][0][:, :want].tobytes() and out[w][1][:, :want].tobytes() == out["b"][1][:, :want].tobytes(), \
                        "%s accept %g k %d: way (%s) and way (b) differ" % (lname, acc, k, w)
                assert out["b"][3].tobytes() == out["c"][3].tobytes()
                b_fast, b_slow, c_slow = min(runs["b"]), max(runs["b"]), max(runs["c"])
                wins = c_slow < b_fast - (b_slow - b_fast)
                fused_wins_everywhere &= wins
                rec = {"groups": lname, "n_groups": int(groups.count), "live_groups": int(groups.live), "filter_accepts": acc, "k": k,
                       "unfused_s_per_call_runs": [round(x, 6) for x in runs["b"]], "fused_s_per_call_runs": [round(x, 6) for x in runs["c"]],
                       "unfused_s_per_call": round(med(runs["b"]), 6), "fused_s_per_call": round(med(runs["c"]), 6),
                       "fused_speedup_over_unfused": round(med(runs["b"]) / med(runs["c"]), 3),
                       "fused_slowest_beats_unfused_fastest_by_more_than_its_spread": bool(wins),
                       "status1_share": round(float(out["b"][3].mean()), 4), "answers_agree": True}
                if t_a:
                    best_new = min(med(runs["b"]), med(runs["c"]))
                    rec.update({"score_rows_and_host_reduce_s_per_call": round(med(t_a), 6),
                                "unfused_speedup_over_score_rows_and_host_reduce": round(med(t_a) / med(runs["b"]), 2),
                                "fused_speedup_over_score_rows_and_host_reduce": round(med(t_a) / med(runs["c"]), 2),
                                "faster_than_the_exact_way": bool(best_new < med(t_a))})
                res["legs"].append(rec)
                print("bench_maxsim: %s accept %g k %d: unfused %.6f fused %.6f s per call%s" % (lname, acc, k, med(runs["b"]), med(runs["c"]),
                                                                                              ", host way %.3f" % med(t_a) if t_a else ""), file=sys.stderr, flush=True)
            groups.close()
            if flt is not None:
                flt.close()
    res["maxsim_fused_auto_means_fused"] = bool(fused_wins_everywhere)
    ix.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
