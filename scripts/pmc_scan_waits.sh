#!/bin/bash
# what are the waves of the largest scan launch waiting for?  The sibling of pmc_scan_valu.sh: a kernel trace for the launch's duration, then
# four counter runs of the same command, each a run of its own (a block takes about four counters per run: five TCC sums in one were refused,
# "exceeds the capabilities of the hardware to collect"):
#   1 wave time, clock   SQ_WAVE_CYCLES, busy / waiting for issue / waiting for anything, the vector ALUs' share, instructions per wave;
#                        GRBM_GUI_ACTIVE (summed over the 8 XCDs) / 8 / the launch's duration - reads high on short dispatches
#   2 L2                 TCC requests, hits, misses, tag stalls
#   3 L1 stalls          TCP pending and TCR stall cycles of the cycles the TCPs are gated on
#   4 L1 -> L2           TCP -> TCC read requests and their summed latency, TA busy
#   scripts/pmc_scan_waits.sh <outdir> [bench args, e.g. --config c2]        BBQ_LIB=<other build's libbbq.so> to measure that build
set -o pipefail
R=$PWD
OUT=$R/${1:?an output directory, relative to the repository root}; shift
mkdir -p $OUT
cd /tmp && export TMPDIR=/tmp
COMMON="--no-recall --no-cpu-baseline --no-parity --latency-calls 0 --shared-sweep 0 --no-configs --no-napi --no-raw --no-hbm-only --inprocess-shards 0 --steps 2 --warmup 1 --slots 1"
LIMIT=${PMC_RUN_LIMIT:-240}
rm -rf /tmp/rp_w0
timeout -k 10 $LIMIT rocprofv3 --kernel-trace --output-format csv -d /tmp/rp_w0 -- python3 $R/bench.py "$@" $COMMON > $OUT/bench_trace.json 2> $OUT/trace.err || exit 1
cp $(ls /tmp/rp_w0/*/*kernel_trace.csv | head -1) $OUT/kernel_trace.csv
pass() {
  n=$1; shift
  rm -rf /tmp/rp_w$n
  timeout -k 10 $LIMIT rocprofv3 --pmc "$@" --output-format csv -d /tmp/rp_w$n -- python3 $R/bench.py $BENCH_ARGS $COMMON > /dev/null 2> $OUT/pmc$n.err || exit 1
  cp $(ls /tmp/rp_w$n/*/*counter_collection.csv | head -1) $OUT/pmc$n.csv
}
BENCH_ARGS="$*"
pass 1 SQ_WAVE_CYCLES SQ_BUSY_CYCLES SQ_WAIT_ANY SQ_WAIT_INST_ANY SQ_ACTIVE_INST_ANY SQ_ACTIVE_INST_VALU SQ_INSTS_VALU SQ_WAVES GRBM_GUI_ACTIVE || exit 1
pass 2 TCC_REQ_sum TCC_HIT_sum TCC_MISS_sum TCC_TAG_STALL_sum || exit 1
pass 3 TCP_PENDING_STALL_CYCLES_sum TCP_TCR_TCP_STALL_CYCLES_sum TCP_GATE_EN1_sum || exit 1
pass 4 TCP_TCC_READ_REQ_sum TCP_TCC_READ_REQ_LATENCY_sum TA_TA_BUSY_sum || exit 1
python3 - $OUT <<'PY'
import csv, sys, os, collections
out = sys.argv[1]
tr = [r for r in csv.DictReader(open(os.path.join(out, "kernel_trace.csv"))) if "bbq_scan_kernel" in r["Kernel_Name"]]
def gsz(r): return int(r["Grid_Size_X"]) * int(r["Grid_Size_Y"]) if "Grid_Size_X" in r else int(r["Grid_Size"])
big = max(gsz(r) for r in tr)
d = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) for r in tr if gsz(r) == big]
name = [r["Kernel_Name"] for r in tr if gsz(r) == big][0]
dur = sum(d) / len(d) * 1e-9
pl = collections.defaultdict(list)
for i in range(1, 5):
    rows = [r for r in csv.DictReader(open(os.path.join(out, "pmc%d.csv" % i))) if "bbq_scan_kernel" in r["Kernel_Name"]]
    b = max(int(r["Grid_Size"]) for r in rows)
    for r in rows:
        if int(r["Grid_Size"]) == b: pl[r["Counter_Name"]].append(float(r["Counter_Value"]))
m = {k: sum(v) / len(v) for k, v in pl.items()}
g = lambda k: m.get(k, 0.0)
waves, wc = max(1.0, g("SQ_WAVES")), max(1.0, g("SQ_WAVE_CYCLES"))
clock = g("GRBM_GUI_ACTIVE") / 8 / dur
print("largest launch: %s" % name.split("(")[0])
print("duration under the trace: %.1f us (%d launches), waves %.0f" % (dur * 1e6, len(d), waves))
print("clock estimate GRBM_GUI_ACTIVE / 8 / duration: %.2f GHz (reads high on short dispatches)" % (clock / 1e9))
print("wave time: issuing %.3f  waiting for issue %.3f  waiting (any) %.3f" % (g("SQ_ACTIVE_INST_ANY") / wc, g("SQ_WAIT_INST_ANY") / wc, g("SQ_WAIT_ANY") / wc))
print("VALU active share of SIMD time (x4 quad-cycles): at 2.1 GHz %.3f, at the estimated clock %.3f" % (g("SQ_ACTIVE_INST_VALU") * 4 / (dur * 1024 * 2.1e9), g("SQ_ACTIVE_INST_VALU") * 4 / max(1.0, dur * 1024 * clock)))
print("per wave: VALU %.0f instructions; wave lifetime %.0f quad-cycles" % (g("SQ_INSTS_VALU") / waves, wc / waves))
print("L2: requests %.0f  hit rate %.3f  requests/s %.3g (= %.2f TB/s if every one were 128 B); tag stall %.0f" % (g("TCC_REQ_sum"), g("TCC_HIT_sum") / max(1.0, g("TCC_HIT_sum") + g("TCC_MISS_sum")), g("TCC_REQ_sum") / dur, g("TCC_REQ_sum") * 128 / dur / 1e12, g("TCC_TAG_STALL_sum")))
print("TCP: pending stall %.3f  TCR stall %.3f of the gated-on cycles (%.0f); read requests to the L2 %.0f, summed latency / request %.0f cycles; TA busy (sum) %.0f" % (g("TCP_PENDING_STALL_CYCLES_sum") / max(1.0, g("TCP_GATE_EN1_sum")), g("TCP_TCR_TCP_STALL_CYCLES_sum") / max(1.0, g("TCP_GATE_EN1_sum")), g("TCP_GATE_EN1_sum"), g("TCP_TCC_READ_REQ_sum"), g("TCP_TCC_READ_REQ_LATENCY_sum") / max(1.0, g("TCP_TCC_READ_REQ_sum")), g("TA_TA_BUSY_sum")))
print({k: round(v) for k, v in sorted(m.items())})
PY
