#!/usr/bin/env python3
"""Compacting an index at size: what bbq_index_compact costs, against the floor (a device-to-device copy of the bytes the compacted
index occupies), against what a user had to do before (bbq_index_export, a host selection, bbq_index_create), and what it buys: the
compacted index searched against its twin created whole and against the uncompacted index searched through the filter.  768-d COSINE,
1-bit index, compact layout.  Prints ONE JSON line (profiles/index_compact.json).

  python scripts/bench_compact.py                      # N = 10 M; random 99 / 90 / 50 / 10 % and the first 90 % as a block
  python scripts/bench_compact.py --rows 1000000 --runs 3 --today-runs 1 --steps 4

Host clock, medians of --runs; every leg of one keep share is timed in the same process, interleaved run by run.  Every compaction
starts from a fresh index of exactly N rows.  The pass condition is identity of answers, not a time: the compacted index must answer as
its twin does, bit for bit, and as the filtered search does once its ords are mapped through bbq_filter_kept_rows."""
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


def med_ms(ts):
    return round(float(np.median(ts)) * 1e3, 3)


def masks_of(n):
    rng = np.random.default_rng(17)
    u = rng.random(n)
    m = {"random_99": u < 0.99, "random_90": u < 0.90, "random_50": u < 0.50, "random_10": u < 0.10}
    m["first_90_block"] = np.arange(n) < int(0.9 * n)
    return m


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--today-runs", type=int, default=3, help="export + host selection + create per keep share (0: skip)")
    ap.add_argument("--steps", type=int, default=6, help="timed 256-query calls per index (0: skip the search comparison)")
    ap.add_argument("--singles", type=int, default=100, help="timed single-query calls per index")
    ap.add_argument("--shares", default="", help="comma-separated subset of the keep shares")
    args = ap.parse_args()

    import torch  # first: one HIP runtime for torch and libbbq, as bench.py does
    import bench
    import bbq_amd as B
    from bbq_amd import capi
    if B.device_count() < 1:
        raise SystemExit("bench_compact: no HIP device - nothing here can be measured without one")
    n = args.rows
    cen = bench.synth_centroid(DIM)
    cdp = float(B.centroid_dp(cen))
    codes, corr = bench.synth_rows(1, 0, n, DIM // 8)

    def fresh():
        return B.Index(codes, corr, DIM, cdp, corrections="compact")

    warm = B.Index(codes[:4096], corr[:4096], DIM, cdp, corrections="compact")   # context, code objects, allocator: not timed
    with capi.Filter(warm, np.arange(4096) % 2 == 0) as f:
        warm.compact(f)
    bpr = warm.bytes_per_row
    warm.close()

    out = {"what": "bbq_index_compact at %d x 768-d COSINE, 1-bit, compact layout; host clock, ms, medians of %d runs" % (n, args.runs),
           "rows": n, "dim": DIM, "runs": args.runs, "shares": {}}
    masks = masks_of(n)
    wanted = [s for s in args.shares.split(",") if s] or list(masks)
    k, Q = 100, 256
    for name in wanted:
        mask = masks[name]
        kept = capi.kept_rows(mask)
        m = len(kept)
        tiles = (m + 63) // 64
        nbytes = tiles * bpr * 64 + tiles * (64 * 32 + 8)   # tile records + exact corrections + add ranges
        src = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
        dst = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
        t_compact, t_floor, t_filter = [], [], []
        compacted = None
        for run in range(args.runs):
            ix = fresh()
            t0 = time.perf_counter()
            flt = capi.Filter(ix, mask)          # the accept words uploaded: part of what a caller pays, timed on its own
            t_filter.append(time.perf_counter() - t0)
            t0 = time.perf_counter()
            ix.compact(flt)
            t_compact.append(time.perf_counter() - t0)
            flt.close()
            assert ix.n == m
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            dst.copy_(src)
            torch.cuda.synchronize()
            t_floor.append(time.perf_counter() - t0)
            if run == args.runs - 1:
                compacted = ix
            else:
                ix.close()
        del src, dst
        rec = {"kept": m, "keep_share": round(m / n, 4), "bytes_after": nbytes,
               "compact_ms": med_ms(t_compact), "compact_runs_ms": [round(t * 1e3, 3) for t in t_compact],
               "filter_create_ms": med_ms(t_filter),
               "d2d_copy_floor_ms": med_ms(t_floor), "compact_over_floor": round(med_ms(t_compact) / max(med_ms(t_floor), 1e-6), 2),
               "compact_gb_per_s_written": round(nbytes / 1e9 / (med_ms(t_compact) / 1e3), 1)}
        # ---- what a user did before: the rows through host memory both ways
        twin = None
        t_today = []
        for run in range(max(args.today_runs, 1)):
            ix = fresh()
            t0 = time.perf_counter()
            c, r = ix.export()
            t = B.Index(c[kept], r[kept], DIM, cdp, corrections="compact")
            t_today.append(time.perf_counter() - t0)
            ix.close()
            del c, r
            if twin is None:
                twin = t
            else:
                t.close()
        if args.today_runs > 0:
            rec["export_select_create_ms"] = med_ms(t_today)
            rec["today_over_compact"] = round(med_ms(t_today) / med_ms(t_compact), 1)
        else:
            rec["export_select_create_ms"] = "not measured"
        # ---- the payoff: compacted against its twin created whole and against the uncompacted index searched through the filter
        if args.steps > 0 and m > 0:
            whole = fresh()
            flt = capi.Filter(whole, mask)
            legs = (("compacted", lambda qq, qc, kk: compacted.search_batch(qq, qc, QB, SIM, kk)),
                    ("twin", lambda qq, qc, kk: twin.search_batch(qq, qc, QB, SIM, kk)),
                    ("filtered", lambda qq, qc, kk: whole.search_filtered_batch(qq, qc, QB, SIM, kk, flt)))
            tb = {nm: [] for nm, _ in legs}
            same_twin = same_filtered = True
            for i in range(args.steps + 2):
                qq, qc = bench.synth_queries(100 + i, Q, DIM, QB)
                res = {}
                for j in range(3):
                    nm, fn = legs[(i + j) % 3]
                    t0 = time.perf_counter()
                    res[nm] = fn(qq, qc, k)
                    if i >= 2:
                        tb[nm].append(time.perf_counter() - t0)
                same_twin = same_twin and all((a.view(np.uint8) == b.view(np.uint8)).all() for a, b in zip(res["compacted"], res["twin"]))
                ci, cs, cc = res["compacted"]
                fi, fs, fc = res["filtered"]
                same_filtered = same_filtered and (cc == fc).all() and (kept[ci] == fi).all() and (cs.view(np.uint32) == fs.view(np.uint32)).all()
            qq, qc = bench.synth_queries(99, args.singles + 20, DIM, QB)
            t1 = {nm: [] for nm, _ in legs}
            for i in range(args.singles + 20):
                for j in range(3):
                    nm, fn = legs[(i + j) % 3]
                    t0 = time.perf_counter()
                    fn(qq[i:i + 1], qc[i:i + 1], k)
                    if i >= 20:
                        t1[nm].append(time.perf_counter() - t0)
            rec["search"] = {"k": k, "queries_per_call": Q, "steps": args.steps, "identical_to_twin": bool(same_twin),
                             "identical_to_filtered_through_kept_rows": bool(same_filtered),
                             "batch_qps": {nm: round(Q * len(tb[nm]) / sum(tb[nm]), 1) for nm in tb},
                             "single_p50_ms": {nm: med_ms(t1[nm]) for nm in t1}}
            rec["search"]["compacted_over_twin_qps"] = round(rec["search"]["batch_qps"]["compacted"] / rec["search"]["batch_qps"]["twin"], 4)
            rec["search"]["compacted_over_filtered_qps"] = round(rec["search"]["batch_qps"]["compacted"] / rec["search"]["batch_qps"]["filtered"], 3)
            flt.close()
            whole.close()
        compacted.close()
        twin.close()
        out["shares"][name] = rec
        print(json.dumps({name: rec}), file=sys.stderr, flush=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
