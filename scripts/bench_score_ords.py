#!/usr/bin/env python3
"""Scoring chosen rows at size: bbq_score_ords_batch beside what a caller had to do without it - bbq_score_rows over [min, max] of the
list, every row in between scored and copied to the host, the asked-for entries picked out there - for the same request, in one
process, the two interleaved call by call so that drift of the box hits both alike.  Prints ONE JSON line (profiles/score_ords.json).

  python scripts/bench_score_ords.py                 # 10 M x 768 synthetic rows, queryBits 4
  python scripts/bench_score_ords.py --rows 2000000 --steps 2 --lengths 64,1024

Legs: lists of 64 / 1 K / 64 K / 1 M ords x {drawn uniformly and left unsorted, the same draw sorted, one contiguous run} x {1, 64 queries
per call, each query with a list of its own}.  Per leg: seconds per call (host clock around calls that return with their results; the median of the timed calls, and the slowest) and
list entries scored per second, for both ways; the range the old way sweeps.  One list per leg is held to the oracle on the rows it
names.  All three outputs (qcDist, f64, f32) are asked for on both sides, and both sides write into host buffers that are allocated and
touched once (the C ABI called directly)."""
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
    ap.add_argument("--lengths", default="64,1024,65536,1048576")
    ap.add_argument("--queries", default="1,64", help="queries per call")
    ap.add_argument("--steps", type=int, default=5, help="timed calls per leg and side")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--check", type=int, default=1, help="1: one list per leg is held to the oracle")
    ap.add_argument("--device", type=int, default=0)
    args = ap.parse_args()
    import torch  # noqa: F401  (first: one HIP runtime for torch and libbbq, as bench.py does)
    import bench
    import bbq_amd as B
    from bbq_amd import capi
    if B.device_count() < 1:
        raise SystemExit("bench_score_ords: no HIP device - nothing here can be measured without one")
    n, dim, QB, SIM = args.rows, args.dim, 4, 1
    codes, corr = bench.synth_rows(1, 0, n, (dim + 7) // 8)
    cdp = float(B.centroid_dp(bench.synth_centroid(dim)))
    ix = B.Index(codes, corr, dim, cdp, device=args.device)
    rng = np.random.default_rng(43)
    lengths = [min(int(v), n) for v in args.lengths.split(",")]
    nqs = [int(v) for v in args.queries.split(",")]
    qq_all, qc_all = bench.synth_queries(2, max(nqs), dim, QB)
    qq_all, qc_all = np.ascontiguousarray(qq_all, np.uint8), np.ascontiguousarray(qc_all, np.float64)
    if args.check:
        import orclib as O

    # both ways write into buffers that are allocated and touched once: a fresh numpy array per call would put the host allocator's
    # page faults (first touch under the device-to-host copy) into the timings, differently from leg to leg
    L = capi.lib()
    cap = max(nqs) * max(lengths)
    gd, g64, g32 = np.ones(cap, np.int32), np.ones(cap, np.float64), np.ones(cap, np.float32)
    sd, s64_, s32_ = np.ones(n, np.int32), np.ones(n, np.float64), np.ones(n, np.float32)

    def gather(qq, qc, off, ords):
        t0 = time.perf_counter()
        rc = L.bbq_score_ords_batch(ix._h, len(off) - 1, qq.ctypes.data, qc.ctypes.data, QB, SIM, off.ctypes.data, ords.ctypes.data,
                                    gd.ctypes.data, g64.ctypes.data, g32.ctypes.data)
        dt = time.perf_counter() - t0
        assert rc == 0, L.bbq_last_error().decode()
        return dt

    def sweep_and_pick(qq, qc, lists):
        """the parent commit's way: per query, the dense sweep of [min, max] and a pick on the host"""
        t0 = time.perf_counter()
        out = []
        for q, ords in enumerate(lists):
            lo, hi = int(ords.min()), int(ords.max())
            rc = L.bbq_score_rows(ix._h, qq[q].ctypes.data, qc[q].ctypes.data, QB, SIM, lo, hi - lo + 1, sd.ctypes.data, s64_.ctypes.data, s32_.ctypes.data)
            assert rc == 0, L.bbq_last_error().decode()
            pos = ords - lo
            out.append((sd[pos], s64_[pos], s32_[pos]))
        return time.perf_counter() - t0, out

    res = {"metric": "score_ords_seconds_per_call", "rows": n, "dim": dim, "query_bits": QB, "timed_calls_per_leg": args.steps,
           "bytes_per_row": ix.bytes_per_row, "lists_checked_against_oracle": 0, "legs": []}
    for nq in nqs:
        qq, qc = qq_all[:nq], qc_all[:nq]
        for m in lengths:
            draws = [rng.integers(0, n, m) for _ in range(nq)]
            starts = rng.integers(0, n - m + 1, nq)
            shapes = {"uniform_unsorted": draws, "uniform_sorted": [np.sort(d) for d in draws],
                      "contiguous": [np.arange(s, s + m) for s in starts]}
            for shape, lists in shapes.items():
                lists = [np.ascontiguousarray(a, np.int32) for a in lists]
                off = np.zeros(nq + 1, np.int64)
                off[1:] = np.cumsum([len(a) for a in lists])
                flat = np.ascontiguousarray(np.concatenate(lists), np.int32)
                tgs, tss = [], []
                for c in range(args.warmup + args.steps):  # interleaved: one call of either side per round
                    dg = gather(qq, qc, off, flat)
                    ds, old = sweep_and_pick(qq, qc, lists)
                    if c >= args.warmup:
                        tgs.append(dg)
                        tss.append(ds)
                tg, ts = float(np.median(tgs)), float(np.median(tss))  # per call: the median of the timed calls
                d, s64, s32 = gd[:off[nq]], g64[:off[nq]], g32[:off[nq]]
                for q in range(nq):  # both ways agree, bit for bit
                    sl = slice(off[q], off[q + 1])
                    assert (d[sl] == old[q][0]).all() and (s64[sl].view(np.uint64) == old[q][1].view(np.uint64)).all() and \
                        (s32[sl].view(np.uint32) == old[q][2].view(np.uint32)).all(), "%s x %d: the two ways differ" % (shape, m)
                if args.check:
                    ords = lists[0]
                    od, o64, o32 = O.score_all(codes[ords], corr[ords], dim, qq[0], qc[0], QB, SIM, cdp)
                    sl = slice(off[0], off[1])
                    assert (d[sl] == od).all() and (s64[sl].view(np.uint64) == o64.view(np.uint64)).all() and \
                        (s32[sl].view(np.uint32) == o32.view(np.uint32)).all(), "%s x %d: differs from the oracle" % (shape, m)
                    res["lists_checked_against_oracle"] += 1
                swept = int(sum(int(a.max()) - int(a.min()) + 1 for a in lists))
                res["legs"].append({"queries": nq, "list_length": m, "shape": shape,
                                    "score_ords_s_per_call": round(tg, 6), "score_ords_s_per_call_max": round(max(tgs), 6),
                                    "score_ords_entries_per_s": round(nq * m / tg, 1),
                                    "sweep_and_pick_s_per_call": round(ts, 6), "sweep_and_pick_entries_per_s": round(nq * m / ts, 1),
                                    "rows_swept_by_sweep_and_pick": swept, "speedup": round(ts / tg, 2)})
    ix.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
