#!/usr/bin/env python3
"""The exact MaxSim rerank at size: bbq_rerank_maxsim_groups_batch beside the only exact way a caller had without it, for the same
request, in one process, the ways interleaved call by call so that drift of the box hits all alike.  Prints ONE JSON line
(profiles/maxsim_rerank.json).

  python scripts/bench_maxsim_rerank.py              # 1 M x 768 fp32 rows, 16 queries of 32 tokens per call, COSINE

Ways:
  (y)   the yardstick: every candidate list expanded into its ords on the host, bbq_rerank_scores with every token vector as a query of
        its own over its query's rows, the group maxima (numpy) and bbq_maxsim_reduce_true on the host
  (n)   bbq_rerank_maxsim_groups_batch
The bytes of (y) and (n) are compared on every leg before anything is timed.
Legs: 1 000 candidates per query over groups of 1..16 rows, and 100 candidates per query over groups of 1 000 rows; without a filter and
under a random filter that accepts 90 % of the rows.  Per leg the ways run three times in alternation, each run the median
of the timed calls (host clock around calls that return with their results).  The claim per leg: the slowest of (n)'s three runs beats
the fastest of (y)'s by more than (y)'s spread (its slowest run minus its fastest)."""
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
    ap.add_argument("--true-sim", type=int, default=1)
    ap.add_argument("--steps", type=int, default=7, help="timed calls per run and way (at least 7)")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--runs", type=int, default=3, help="alternating runs per leg")
    ap.add_argument("--only-new", type=int, default=0, help="1: time the new call alone (for a kernel trace)")
    ap.add_argument("--device", type=int, default=0)
    args = ap.parse_args()
    if args.steps < 7:
        raise SystemExit("bench_maxsim_rerank: a median of fewer than 7 calls is not reported")
    import torch  # noqa: F401  (first: one HIP runtime for torch and libbbq, as bench.py does)
    import bench
    import bbq_amd as B
    from bbq_amd import capi
    if B.device_count() < 1:
        raise SystemExit("bench_maxsim_rerank: no HIP device - nothing here can be measured without one")
    n, dim, nq, T, SIM = args.rows, args.dim, args.queries, args.tokens, args.true_sim
    rng = np.random.default_rng(71)
    # the group sets and filters hang on an index of n rows; the rerank reads the fp32 rows alone
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
    print("bench_maxsim_rerank: %d x %d fp32 rows resident" % (n, dim), file=sys.stderr, flush=True)
    nv = nq * T
    tokens = np.ascontiguousarray(rng.standard_normal((nv, dim), dtype=np.float32))
    voff = (np.arange(nq + 1, dtype=np.int64) * T)
    L = capi.lib()
    med = lambda t: float(np.median(t))  # noqa: E731

    sizes = rng.integers(1, 17, n // 4)
    off_small = np.concatenate([[0], np.cumsum(sizes)])
    off_small = np.append(off_small[off_small < n], n).astype(np.int64)
    off_big = np.unique(np.append(np.arange(0, n, 1000), n)).astype(np.int64)
    legs = (("groups_of_1_to_16", off_small, 1000), ("groups_of_1000", off_big, 100))

    res = {"metric": "maxsim_rerank_seconds_per_call", "rows": n, "dim": dim, "true_sim": SIM, "queries_per_call": nq, "tokens_per_query": T,
           "token_block": capi.maxsim_token_block(), "timed_calls_per_run": args.steps, "runs_per_leg": args.runs, "legs": []}
    for lname, off, n_cand in legs:
        for acc in (1.0, 0.9):
            accept = np.ones(n, np.bool_) if acc >= 1.0 else rng.random(n) < acc
            flt = None if acc >= 1.0 else capi.Filter(ix, accept)
            groups = capi.Groups(ix, off, flt)
            live = np.flatnonzero(np.add.reduceat(accept.astype(np.int64), off[:-1]) * (np.diff(off) > 0) > 0)
            cands = [np.ascontiguousarray(rng.choice(live, min(n_cand, len(live)), replace=False), np.int32) for _ in range(nq)]
            coff = np.concatenate([[0], np.cumsum([len(c) for c in cands])]).astype(np.int64)
            cand = np.ascontiguousarray(np.concatenate(cands), np.int32)
            out = {w: np.full(len(cand), -1.0, np.float64) for w in "yn"}

            def way_n():
                t0 = time.perf_counter()
                rc = L.bbq_rerank_maxsim_groups_batch(V._h, groups._h, nq, voff.ctypes.data, tokens.ctypes.data, SIM, coff.ctypes.data, cand.ctypes.data,
                                                      out["n"].ctypes.data)
                dt = time.perf_counter() - t0
                assert rc == 0, L.bbq_last_error().decode()
                return dt

            def way_y():
                t0 = time.perf_counter()
                # the lists, expanded: query q's rows, once per token vector
                rows_of, starts_of = [], []
                for c in cands:
                    lens = (off[c.astype(np.int64) + 1] - off[c]).astype(np.int64)
                    starts = np.concatenate([[0], np.cumsum(lens)[:-1]])
                    rows_of.append((np.repeat(off[c] - starts, lens) + np.arange(int(lens.sum()))).astype(np.int32))
                    starts_of.append(starts)
                ords = np.ascontiguousarray(np.concatenate([np.tile(r, T) for r in rows_of]))
                ooff = np.concatenate([[0], np.cumsum(np.repeat([len(r) for r in rows_of], T))]).astype(np.int64)
                c64 = np.empty(len(ords), np.float64)
                rc = L.bbq_rerank_scores(V._h, nv, tokens.ctypes.data, ooff.ctypes.data, ords.ctypes.data, SIM, c64.ctypes.data)
                assert rc == 0, L.bbq_last_error().decode()
                for q in range(nq):
                    r = rows_of[q]
                    block = c64[ooff[q * T]:ooff[q * T + T]].reshape(T, len(r))
                    if flt is not None:
                        block = np.where(accept[r][None, :], block, -np.inf)   # the rows are finite: no NaN, no -Inf among the scores
                    rep = np.maximum.reduceat(block, starts_of[q], axis=1)
                    out["y"][coff[q]:coff[q + 1]] = capi.maxsim_reduce_true(rep)
                return time.perf_counter() - t0

            # the answers first: nothing is timed before the two ways agree
            way_n()
            if not args.only_new:
                way_y()
                assert out["y"].tobytes() == out["n"].tobytes(), "%s accept %g: the yardstick's bytes and the new call's differ" % (lname, acc)
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
            rows_per_query = int(np.mean([(off[c.astype(np.int64) + 1] - off[c]).sum() for c in cands]))
            rec = {"groups": lname, "n_groups": int(groups.count), "live_groups": int(groups.live), "filter_accepts": acc,
                   "candidates_per_query": int(len(cands[0])), "expanded_rows_per_query": rows_per_query,
                   "fma_per_call": int(nq) * T * rows_per_query * dim, "row_bytes_per_call": int(nq) * rows_per_query * dim * 4,
                   "new_s_per_call_runs": [round(x, 6) for x in runs["n"]], "new_s_per_call": round(med(runs["n"]), 6)}
            if not args.only_new:
                y_fast, y_slow, n_slow = min(runs["y"]), max(runs["y"]), max(runs["n"])
                rec.update({"yardstick_s_per_call_runs": [round(x, 6) for x in runs["y"]], "yardstick_s_per_call": round(med(runs["y"]), 6),
                            "new_speedup_over_yardstick": round(med(runs["y"]) / med(runs["n"]), 2),
                            "new_slowest_beats_yardstick_fastest_by_more_than_its_spread": bool(n_slow < y_fast - (y_slow - y_fast)),
                            "bytes_agree": True})
            res["legs"].append(rec)
            print("bench_maxsim_rerank: %s accept %g: %s" % (lname, acc, ", ".join("%s %.6f" % (w, med(v)) for w, v in runs.items())), file=sys.stderr, flush=True)
            groups.close()
            if flt is not None:
                flt.close()
    V.close()
    ix.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
