#!/bin/bash
# one round's evidence: profiles of the headline and c2, the single-query timeline, the full bench line, the GPU tests
#   scripts/round_evidence.sh <outdir>      (outdir relative to the repository root; scripts/publish_profiles.py reads it back)
set -o pipefail
R=$(cd "$(dirname "$0")/.." && pwd)
OUT=$R/${1:?usage: scripts/round_evidence.sh <outdir>}
mkdir -p $OUT
cd $R
scripts/collect_profiles.sh headline > $OUT/collect_headline.log 2>&1 && echo "headline profiles ok"
scripts/collect_profiles.sh c2 --config c2 > $OUT/collect_c2.log 2>&1 && echo "c2 profiles ok"
( cd /tmp && export TMPDIR=/tmp && rm -rf /tmp/rp_lat && rocprofv3 --kernel-trace --output-format csv -d /tmp/rp_lat -- python3 $R/scripts/latency.py 10000000 only=1 > $OUT/latency_under_trace.txt 2>/dev/null && cp $(ls /tmp/rp_lat/*/*kernel_trace.csv | head -1) $OUT/latency_kernel_trace.csv ) && python3 scripts/trace_one_call.py $OUT/latency_kernel_trace.csv > $OUT/single_query_timeline.txt && cat $OUT/single_query_timeline.txt
timeout -k 10 400 python bench.py --full > $OUT/bench_default.json 2> $OUT/bench_default.err; echo "bench rc=$?"
timeout -k 10 600 python -m pytest tests -m gpu -q > $OUT/gpu_tests.log 2>&1; tail -3 $OUT/gpu_tests.log
