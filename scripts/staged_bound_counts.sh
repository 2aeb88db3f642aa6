#!/bin/bash
# How many tiles of each sweep launch take stage two of the staged twin (bbq_scan_staged_kernel), and how many defer a row at all?
# A COUNTING BUILD of the library - the sources of this tree compiled with -DBBQ_COUNT_STAGES into a directory of its own, never the product's
# build: every kernel with several tiles per wave then counts its tiles, the tiles whose first ballot is non-zero (stage two, where the launch
# is staged; the bound's own ballot where it is not), the tiles that defer a row and the rows deferred, and every such launch waits for its
# end and prints the four on stderr.  This script builds it, runs the benchmark's timed step alone against it, and sums the lines per launch shape.
#   scripts/staged_bound_counts.sh <outdir> [bench args, e.g. --config c2]      BBQ_COUNT_LIB=<a counting build made elsewhere> skips the build
set -o pipefail
R=$PWD
OUT=$R/${1:?an output directory, relative to the repository root}; shift
mkdir -p $OUT
LIB=$BBQ_COUNT_LIB
if [ -z "$LIB" ]; then
  B=$(mktemp -d)
  mkdir -p $B/x/csrc && cp -r $R/include $B/include && cp $R/better-binary-quantization_amd/csrc/*.h $R/better-binary-quantization_amd/csrc/*.hip $R/better-binary-quantization_amd/csrc/*.cpp $R/better-binary-quantization_amd/csrc/Makefile $B/x/csrc/
  make -s -j16 -C $B/x/csrc CXXFLAGS="-O3 -std=c++17 -fPIC -ffp-contract=off -fno-fast-math -Wall -Wno-unused-result -DBBQ_COUNT_STAGES" || exit 1
  LIB=$B/x/lib/libbbq.so
fi
COMMON="--no-recall --no-cpu-baseline --no-parity --latency-calls 0 --shared-sweep 0 --no-configs --no-napi --no-raw --no-hbm-only --inprocess-shards 0 --no-shard-shape --no-c1 --steps 2 --warmup 1 --slots 1"
BBQ_LIB=$LIB timeout -k 10 ${COUNT_RUN_LIMIT:-400} python3 $R/bench.py "$@" $COMMON > $OUT/bench_counts.json 2> $OUT/counts.err || exit 1
python3 - $OUT <<'PY'
import collections, json, os, re, sys
out = sys.argv[1]
acc = collections.OrderedDict()
for line in open(os.path.join(out, "counts.err")):
    m = re.match(r"stage_counts chunks (\d+) queries (\d+) tiles_per_wave (\d+) staged (\d): tiles (\d+) first_ballot_nonzero (\d+) deferring (\d+) rows_deferred (\d+)", line)
    if m:
        v = [int(x) for x in m.groups()]
        a = acc.setdefault((v[0], v[2], v[3]), [0, 0, 0, 0, 0])
        a[0] += 1
        for i in range(4):
            a[1 + i] += v[4 + i]
res = []
for (chunks, tpw, staged), (n, tiles, first, deferring, rows) in acc.items():
    res.append({"chunks": chunks, "rows": chunks * 512, "tiles_per_wave": tpw, "staged": staged, "launches": n, "tile_waves": tiles,
                "first_ballot_nonzero_share": first / max(1, tiles), "deferring_tile_share": deferring / max(1, tiles), "rows_deferred_per_tile": rows / max(1, tiles)})
    print("launch of %7d chunks (%9d rows), %d tiles per wave, staged %d: %d launches, %d tile-waves; first ballot non-zero %.5f, tiles deferring %.5f, rows deferred per tile %.5f" % (
        chunks, chunks * 512, tpw, staged, n, tiles, first / max(1, tiles), deferring / max(1, tiles), rows / max(1, tiles)))
json.dump(res, open(os.path.join(out, "stage_counts.json"), "w"), indent=1)
PY
