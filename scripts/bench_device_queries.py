#!/usr/bin/env python3
"""Query quantization on the device beside the host quantizer of the same process.  Prints ONE JSON line (profiles/device_queries.json).

  python scripts/bench_device_queries.py            # 768-d, queryBits 4, COSINE

Legs "quantize": n = 1, 64, 512, 4096 and 65536 raw queries per call, three ways interleaved call by call inside a run:
  (d)    bbq_quantize_queries_device - upload, kernel and download, from and to pageable host arrays
  (h16)  bbq_quantize_queries on 16 host threads        (h1)  on one
Leg "raw_batch": bbq_search_raw_batch over a 1 M x 768 1-bit index, 4096 raw queries per call, k = 10, sweep_share 32, 16 host threads,
option device_queries 0 against 1.
Per leg the ways run three times in alternation, each run the median of 7 timed calls (host clock around calls that return with their
results).  The bytes of the ways are compared before anything is timed.  --only-device N: N calls of (d) at 4096 queries and nothing
else, for a kernel trace."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "better-binary-quantization_amd", "python")):
    if p not in sys.path:
        sys.path.insert(0, p)


def timed_runs(ways, steps, warmup, runs):
    """ways: {name: call} -> {name: [median seconds of each run]}; inside a run the ways alternate call by call"""
    out = {name: [] for name in ways}
    for _ in range(runs):
        t = {name: [] for name in ways}
        for i in range(warmup + steps):
            for name, call in ways.items():
                t0 = time.perf_counter()
                call()
                if i >= warmup:
                    t[name].append(time.perf_counter() - t0)
        for name in ways:
            out[name].append(float(np.median(t[name])))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--rows", type=int, default=1_000_000, help="rows of the raw_batch leg's index (0: skip the leg)")
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--only-device", type=int, default=0)
    args = ap.parse_args()
    if args.steps < 7:
        raise SystemExit("bench_device_queries: a median of fewer than 7 calls is not reported")
    import torch  # noqa: F401  (first: one HIP runtime for torch and libbbq, as bench.py does)
    import bbq_amd as B
    if B.device_count() < 1:
        raise SystemExit("bench_device_queries: no HIP device - nothing here can be measured without one")
    dim, SIM, QB = args.dim, 1, 4
    rng = np.random.default_rng(91)
    cen = (rng.standard_normal(dim) * 0.05).astype(np.float32)
    small = B.Index(np.zeros((1, (dim + 7) // 8), np.uint8), np.zeros((1, 4)), dim, B.centroid_dp(cen))
    if args.only_device:
        q = rng.standard_normal((4096, dim)).astype(np.float32)
        for _ in range(args.only_device):
            small.quantize_queries(q, cen, SIM, QB)
        print(json.dumps({"only_device_calls": args.only_device, "queries": 4096, "dim": dim}))
        return
    legs = []
    for n in (1, 64, 512, 4096, 65536):
        q = rng.standard_normal((n, dim)).astype(np.float32)
        ways = {"d": lambda: small.quantize_queries(q, cen, SIM, QB), "h16": lambda: B.quantize_queries(q, cen, SIM, QB, n_threads=16),
                "h1": lambda: B.quantize_queries(q, cen, SIM, QB, n_threads=1)}
        want = ways["h16"]()
        for name in ("d", "h1"):
            got = ways[name]()
            assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes(), "n=%d: (%s) differs from (h16)" % (n, name)
        t = timed_runs(ways, args.steps, args.warmup, args.runs)
        legs.append({"leg": "quantize", "queries": n, "median_ms_per_run": {k: [round(x * 1e3, 4) for x in v] for k, v in t.items()},
                     "queries_per_s_best_run": {k: round(n / min(v)) for k, v in t.items()},
                     "device_wins_every_run": {k: bool(max(t["d"]) < min(t[k])) for k in ("h16", "h1")}})
        print("quantize n=%d: %s" % (n, legs[-1]["median_ms_per_run"]), file=sys.stderr, flush=True)
    small.close()
    if args.rows:
        n, nq, k = args.rows, 4096, 10
        base = rng.standard_normal((n, dim), dtype=np.float32)
        ix, _, _, bcen = B.Index.build(base, SIM, want_host_copy=False)
        del base
        ix.set_option("sweep_share", 32)
        q = rng.standard_normal((nq, dim)).astype(np.float32)

        def raw(v):
            ix.set_option("device_queries", v)
            return ix.search_raw_batch(q, bcen, SIM, QB, k, n_threads=16, want_quantized=True)
        want, got = raw(0), raw(1)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(got, want)), "raw_batch: device_queries 1 differs from 0"
        t = timed_runs({"device_queries_0": lambda: raw(0), "device_queries_1": lambda: raw(1)}, args.steps, args.warmup, args.runs)
        legs.append({"leg": "raw_batch", "rows": n, "queries": nq, "k": k, "sweep_share": 32, "host_threads": 16,
                     "median_ms_per_run": {k_: [round(x * 1e3, 3) for x in v] for k_, v in t.items()},
                     "queries_per_s_best_run": {k_: round(nq / min(v)) for k_, v in t.items()},
                     "device_wins_every_run": bool(max(t["device_queries_1"]) < min(t["device_queries_0"]))})
        ix.close()
    print(json.dumps({"what": "scripts/bench_device_queries.py", "dim": dim, "similarity": "COSINE", "query_bits": QB, "steps": args.steps,
                      "runs": args.runs, "host_cpus": os.cpu_count(), "legs": legs}))


if __name__ == "__main__":
    main()
