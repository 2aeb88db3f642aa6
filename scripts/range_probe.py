#!/usr/bin/env python3
"""Range search at size: bbq_search_range_batch and bbq_count_range_batch beside what a caller had without them - bbq_score_rows over
the whole index per query and a compare on the host - for the same request, in one process, the ways interleaved call by call so that
drift of the box hits all alike.  Prints a small table (profiles/range_search.txt).

  python scripts/range_probe.py                     # 1 M x 768 synthetic 1-bit COSINE rows, compact corrections, 64 queries, queryBits 4
  python scripts/range_probe.py --rows 200000 --steps 5

Per query the thresholds come from its own dense scores: its 100th-best score, the score 0.1 % of the rows reach and the score 10 % reach.
At each level the range answer is first held to the numpy restatement over the dense scores (indices, score bits, offsets, counts); then
the three ways are timed: a host clock around calls that return with their results, warm-up calls first, the median of the timed calls
and the fastest.  All ways write into host buffers that are allocated and touched once (the C ABI called directly)."""
import argparse
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
    ap.add_argument("--queries", type=int, default=64)
    ap.add_argument("--steps", type=int, default=20, help="timed calls per level and way")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--device", type=int, default=0)
    args = ap.parse_args()
    import torch  # noqa: F401  (first: one HIP runtime for torch and libbbq, as bench.py does)
    import bench
    import bbq_amd as B
    from bbq_amd import capi
    if B.device_count() < 1:
        raise SystemExit("range_probe: no HIP device - nothing here can be measured without one")
    n, dim, nq, QB, SIM = args.rows, args.dim, args.queries, 4, 1
    codes, corr = bench.synth_rows(1, 0, n, (dim + 7) // 8)
    cdp = float(B.centroid_dp(bench.synth_centroid(dim)))
    ix = B.Index(codes, corr, dim, cdp, device=args.device, corrections="compact")
    qq, qc = bench.synth_queries(2, nq, dim, QB)
    qq, qc = np.ascontiguousarray(qq, np.uint8), np.ascontiguousarray(qc, np.float64)
    L = capi.lib()
    dense = np.ones((nq, n), np.float32)
    for q in range(nq):
        assert L.bbq_score_rows(ix._h, qq[q].ctypes.data, qc[q].ctypes.data, QB, SIM, 0, n, None, None, dense[q].ctypes.data) == 0
    assert not np.isnan(dense).any()
    ranked = np.sort(dense, axis=1)
    levels = [("100th best", 100), ("0.1 % of the rows", max(n // 1000, 1)), ("10 % of the rows", max(n // 10, 1))]
    scratch = np.ones(n, np.float32)

    print("range_probe: %d x %d 1-bit COSINE rows, compact corrections (%d B/row), %d queries per call, queryBits %d; %d timed calls per way after %d warm-up calls"
          % (n, dim, ix.bytes_per_row, nq, QB, args.steps, args.warmup))
    print("seconds per call of %d queries: median (fastest).  workaround = bbq_score_rows over all rows per query + the compare on the host" % nq)
    print("%-20s %10s %24s %24s %24s %10s %10s" % ("threshold", "entries", "search_range_batch", "count_range_batch", "workaround", "wa/search", "wa/count"))
    for label, rank in levels:
        ths = np.ascontiguousarray(ranked[:, n - rank], np.float32)
        want = [np.flatnonzero(dense[q] >= ths[q]) for q in range(nq)]
        total = int(sum(len(w) for w in want))
        off, idx, sc, cnt = np.ones(nq + 1, np.int64), np.ones(total, np.int32), np.ones(total, np.float32), np.ones(nq, np.int64)

        def search():
            t0 = time.perf_counter()
            rc = L.bbq_search_range_batch(ix._h, None, nq, qq.ctypes.data, qc.ctypes.data, QB, SIM, ths.ctypes.data, total, off.ctypes.data,
                                          idx.ctypes.data, sc.ctypes.data)
            dt = time.perf_counter() - t0
            assert rc == 0, L.bbq_last_error().decode()
            return dt

        def count():
            t0 = time.perf_counter()
            rc = L.bbq_count_range_batch(ix._h, None, nq, qq.ctypes.data, qc.ctypes.data, QB, SIM, ths.ctypes.data, cnt.ctypes.data)
            dt = time.perf_counter() - t0
            assert rc == 0, L.bbq_last_error().decode()
            return dt

        def workaround():
            t0 = time.perf_counter()
            out = []
            for q in range(nq):
                rc = L.bbq_score_rows(ix._h, qq[q].ctypes.data, qc[q].ctypes.data, QB, SIM, 0, n, None, None, scratch.ctypes.data)
                assert rc == 0, L.bbq_last_error().decode()
                hit = np.flatnonzero(scratch >= ths[q])
                out.append((hit, scratch[hit]))
            return time.perf_counter() - t0, out

        # the answers are equal before anything is timed
        search(), count()
        _, old = workaround()
        np.testing.assert_array_equal(off, np.concatenate([[0], np.cumsum([len(w) for w in want])]))
        np.testing.assert_array_equal(cnt, [len(w) for w in want])
        for q in range(nq):
            sl = slice(off[q], off[q + 1])
            np.testing.assert_array_equal(idx[sl], want[q])
            np.testing.assert_array_equal(idx[sl], old[q][0])
            assert (sc[sl].view(np.uint32) == dense[q][want[q]].view(np.uint32)).all() and (sc[sl].view(np.uint32) == old[q][1].view(np.uint32)).all()
        ts, tc, tw = [], [], []
        for c in range(args.warmup + args.steps):   # interleaved: one call of every way per round
            a, b, (w, _) = search(), count(), workaround()
            if c >= args.warmup:
                ts.append(a), tc.append(b), tw.append(w)
        ms, mc, mw = float(np.median(ts)), float(np.median(tc)), float(np.median(tw))
        print("%-20s %10d %24s %24s %24s %10.2f %10.2f" % (label, total, "%.6f (%.6f)" % (ms, min(ts)), "%.6f (%.6f)" % (mc, min(tc)),
                                                         "%.6f (%.6f)" % (mw, min(tw)), mw / ms, mw / mc))
    ix.close()


if __name__ == "__main__":
    main()
