#!/usr/bin/env python3
"""Appending rows at size: what bbq_index_append costs, against what a user had to do before, and whether a grown index searches like
one created whole.  768-d COSINE, 1-bit index.  Prints ONE JSON line (profiles/index_append.json).

  python scripts/bench_append.py                                   # everything, N = 1 M and 10 M, B = 1 K / 64 K / 1 M
  python scripts/bench_append.py --parent-lib /path/to/libbbq.so   # ... with the build of B rows timed on that library as well
  python scripts/bench_append.py --sizes 1000000 --blocks 65536 --search-rows 0 --rebuild-runs 0

Sections:
  append    per (N, B): median of --runs appends of B raw fp32 rows to an index of N rows (host clock around bbq_index_append, no host
            copies), once into reserved capacity and once on an index without spare room, which has to grow (allocation +
            device-to-device copy of the N rows: timed on its own as bbq_index_reserve(N + B) on a fresh index, `grow_copy_ms`).
            Every run starts from a fresh index of exactly N rows.
  build     bbq_index_build of the same B rows alone - the same upload and quantization plus the centroid pass - in a child process
            per library: this tree's, and --parent-lib (the commit before appends existed) when given.  Raw ctypes, so that a library
            without the append symbols loads.
  rebuild   bbq_index_build over N + 64 K rows: what growing an index took before.  The fp32 rows are one random 1 M-row block repeated
            (the quantizer's work per row does not depend on its neighbours; generating 31 GB of fresh gaussians would take minutes).
  search    an index of --search-rows rows made as half of them + appends of 1 M rows, and a twin created whole: 256-query batches
            and single-query calls, interleaved call by call in one process (q/s, p50)."""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "better-binary-quantization_amd", "python")):
    if p not in sys.path:
        sys.path.insert(0, p)

DIM, SIM, QB = 768, 1, 4


def raw_rows(seed, n):
    return np.random.default_rng([seed, 99]).standard_normal((n, DIM)).astype(np.float32)


def med_ms(ts):
    return round(float(np.median(ts)) * 1e3, 3)


def build_leg(lib_path, blocks, runs):
    """bbq_index_build_opts of B raw rows, median of `runs`, through raw ctypes on the library at lib_path"""
    import torch  # noqa: F401  (first: one HIP runtime)
    L = C.CDLL(lib_path)
    vp, i32, i64, dbl = C.c_void_p, C.c_int32, C.c_int64, C.c_double
    L.bbq_index_build_opts.argtypes = [vp, i64, i32, i32, i32, dbl, i32, i32, vp, C.POINTER(vp), vp, vp, vp, vp, vp]
    L.bbq_index_destroy.argtypes = [vp]
    L.bbq_index_destroy.restype = None
    out = {}
    cen = np.zeros(DIM, np.float32)
    for b in [1000] + list(blocks):   # the first build of a process pays for the context and the code objects: not timed
        rows = raw_rows(5, b)
        ts = []
        for _ in range(runs + 1):
            h = vp()
            t0 = time.perf_counter()
            rc = L.bbq_index_build_opts(rows.ctypes.data, b, DIM, SIM, 1, 0.1, 5, 0, None, C.byref(h), cen.ctypes.data, None, None, None, None)
            ts.append(time.perf_counter() - t0)
            if rc != 0:
                raise SystemExit("bbq_index_build_opts failed: %d" % rc)
            L.bbq_index_destroy(h)
        out[str(b)] = {"build_ms": med_ms(ts[1:]), "runs_ms": [round(t * 1e3, 3) for t in ts[1:]]}
    if 1000 not in blocks:
        del out["1000"]
    print(json.dumps({"abi": L.bbq_abi_version(), "build": out}))


def rebuild_leg(n, runs):
    """bbq_index_build over n + 64 K raw rows: one random 1 M-row block repeated"""
    import torch  # noqa: F401
    import bbq_amd as B
    block = raw_rows(9, 1_000_000)
    total = n + 65536
    base = np.empty((total, DIM), np.float32)
    for i in range(0, total, block.shape[0]):
        m = min(block.shape[0], total - i)
        base[i:i + m] = block[:m]
    ts = []
    for _ in range(runs):
        t0 = time.perf_counter()
        ix, _, _, _ = B.Index.build(base, SIM, want_host_copy=False)
        ts.append(time.perf_counter() - t0)
        ix.close()
    print(json.dumps({"rows": total, "build_ms": med_ms(ts), "runs": runs}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1000000,10000000", help="N: rows of the index appended to")
    ap.add_argument("--blocks", default="1000,65536,1000000", help="B: rows per append")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--parent-lib", default="", help="a libbbq.so of the commit before appends: its bbq_index_build of B rows is the yardstick")
    ap.add_argument("--rebuild-runs", type=int, default=1, help="builds of N + 64 K rows per N (0: skip)")
    ap.add_argument("--search-rows", type=int, default=10_000_000, help="rows of the grown-against-whole search comparison (0: skip)")
    ap.add_argument("--steps", type=int, default=8, help="timed 256-query calls per index")
    ap.add_argument("--leg", default="", help="internal: 'build' runs the build section on --lib, 'rebuild' the rebuild of --sizes, and prints it")
    ap.add_argument("--lib", default="")
    args = ap.parse_args()
    sizes = [int(x) for x in args.sizes.split(",") if x]
    blocks = [int(x) for x in args.blocks.split(",") if x]
    if args.leg == "build":
        return build_leg(args.lib, blocks, args.runs)
    if args.leg == "rebuild":
        return rebuild_leg(sizes[0], args.rebuild_runs)

    import torch  # noqa: F401  (first: one HIP runtime for torch and libbbq, as bench.py does)
    import bench
    import bbq_amd as B
    from bbq_amd import capi
    if B.device_count() < 1:
        raise SystemExit("bench_append: no HIP device - nothing here can be measured without one")
    cen = bench.synth_centroid(DIM)
    cdp = float(B.centroid_dp(cen))
    out = {"what": "bbq_index_append at 768-d COSINE, 1-bit; host clock, ms, medians of %d runs" % args.runs, "dim": DIM, "runs": args.runs,
           "append": {}, "build": {}, "rebuild": {}, "search": None}

    # ---- build of B rows alone, per library, each in a process of its own
    libs = {"this": capi.LIB_PATH}
    if args.parent_lib:
        libs["parent"] = os.path.abspath(args.parent_lib)
    for name, path in libs.items():
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--leg", "build", "--lib", path, "--blocks", args.blocks, "--runs", str(args.runs)],
                           stdout=subprocess.PIPE, text=True, timeout=1200)
        if r.returncode != 0:
            raise SystemExit("the build leg failed on %s" % path)
        out["build"][name] = json.loads(r.stdout.strip().splitlines()[-1])

    # ---- appends
    warm = B.Index(*bench.synth_rows(1, 0, 4096, DIM // 8), DIM, cdp)
    warm.append(raw_rows(1, 2000), cen, SIM, want_host_copy=False)   # context, code objects, allocator: not timed
    warm.close()
    new_rows = {b: raw_rows(7, b) for b in blocks}
    for n in sizes:
        codes, corr = bench.synth_rows(1, 0, n, DIM // 8)
        per_n = {}
        for b in blocks:
            reserved, growing, copy = [], [], []
            for _ in range(args.runs):
                ix = B.Index(codes, corr, DIM, cdp)
                t0 = time.perf_counter()
                ix.reserve(n + b)                                       # allocation + device-to-device copy of the N rows
                copy.append(time.perf_counter() - t0)
                t0 = time.perf_counter()
                ix.append(new_rows[b], cen, SIM, want_host_copy=False)   # ... into the room that made
                reserved.append(time.perf_counter() - t0)
                assert ix.n == n + b
                ix.close()
                ix = B.Index(codes, corr, DIM, cdp)
                assert ix.capacity < n + b
                t0 = time.perf_counter()
                ix.append(new_rows[b], cen, SIM, want_host_copy=False)   # no room: the append grows the index itself
                growing.append(time.perf_counter() - t0)
                ix.close()
            per_n[str(b)] = {"reserved_ms": med_ms(reserved), "growing_ms": med_ms(growing), "grow_copy_ms": med_ms(copy),
                             "reserved_runs_ms": [round(t * 1e3, 3) for t in reserved], "growing_runs_ms": [round(t * 1e3, 3) for t in growing]}
            for lib in out["build"]:
                per_n[str(b)]["reserved_over_%s_build" % lib] = round(per_n[str(b)]["reserved_ms"] / out["build"][lib]["build"][str(b)]["build_ms"], 3)
        out["append"][str(n)] = per_n
        del codes, corr
    if len(sizes) > 1:
        lo, hi = str(min(sizes)), str(max(sizes))
        out["reserved_at_%s_over_%s" % (hi, lo)] = {str(b): round(out["append"][hi][str(b)]["reserved_ms"] / out["append"][lo][str(b)]["reserved_ms"], 3) for b in blocks}

    # ---- what a user did before: build over all N + B rows (a process of its own per N: 31 GB of host rows at N = 10 M)
    for n in sizes if args.rebuild_runs > 0 else []:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--leg", "rebuild", "--sizes", str(n), "--rebuild-runs", str(args.rebuild_runs)],
                           stdout=subprocess.PIPE, text=True, timeout=1800)
        out["rebuild"][str(n)] = json.loads(r.stdout.strip().splitlines()[-1]) if r.returncode == 0 else {"not_measured": "the child ended with status %d" % r.returncode}

    # ---- search after growth: grown against whole, interleaved
    if args.search_rows > 0:
        n = args.search_rows
        codes, corr = bench.synth_rows(1, 0, n, DIM // 8)
        whole = B.Index(codes, corr, DIM, cdp)
        grown = B.Index(codes[:n // 2], corr[:n // 2], DIM, cdp)
        for a in range(n // 2, n, 1_000_000):
            grown.append_rows(codes[a:min(a + 1_000_000, n)], corr[a:min(a + 1_000_000, n)])
        assert grown.n == whole.n == n
        k, Q = 100, 256
        batches = [bench.synth_queries(100 + i, Q, DIM, QB) for i in range(args.steps + 2)]
        tb = {"whole": [], "grown": []}
        same = True
        for i, (qq, qc) in enumerate(batches):
            res = {}
            for name, ix in (("whole", whole), ("grown", grown)) if i % 2 == 0 else (("grown", grown), ("whole", whole)):
                t0 = time.perf_counter()
                res[name] = ix.search_batch(qq, qc, QB, SIM, k)
                if i >= 2:
                    tb[name].append(time.perf_counter() - t0)
            same = same and all((a.view(np.uint8) == b.view(np.uint8)).all() for a, b in zip(res["whole"], res["grown"]))
        qq, qc = bench.synth_queries(99, 200, DIM, QB)
        t1 = {"whole": [], "grown": []}
        for i in range(200):
            for name, ix in (("whole", whole), ("grown", grown)) if i % 2 == 0 else (("grown", grown), ("whole", whole)):
                t0 = time.perf_counter()
                ix.search(qq[i], qc[i], QB, SIM, k)
                if i >= 20:
                    t1[name].append(time.perf_counter() - t0)
        out["search"] = {"rows": n, "k": k, "queries_per_call": Q, "steps": args.steps, "answers_identical": bool(same),
                         "batch_qps": {m: round(Q * len(tb[m]) / sum(tb[m]), 1) for m in tb},
                         "single_p50_ms": {m: med_ms(t1[m]) for m in t1},
                         "capacity_rows": {"whole": whole.capacity, "grown": grown.capacity}}
        out["search"]["grown_over_whole_qps"] = round(out["search"]["batch_qps"]["grown"] / out["search"]["batch_qps"]["whole"], 4)
        whole.close()
        grown.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
