#!/usr/bin/env python3
"""Registers, occupancy and scratch of every bbq_scan_mfma_kernel instantiation, the unfiltered ones next to their filtered twins, from
the compiler's own remarks (no device needed; scan_resources.py does the same for bbq_scan_kernel).

  scripts/mfma_resources.py CSRC_DIR                  one line per <W, COMPACT, FP, G>: unfiltered | filtered
  scripts/mfma_resources.py BEFORE_DIR AFTER_DIR      the unfiltered instantiations of two trees side by side as well

CSRC_DIR is a copy of better-binary-quantization_amd/csrc.  profiles/mfma_filtered_resources.txt is the output of the second form with
the parent commit's csrc as BEFORE_DIR.
"""
import re
import subprocess
import sys

from scan_resources import FLAGS, HIPCC, fmt


def table(csrc):
    r = subprocess.run([HIPCC] + FLAGS + ["bbq_mfma_kernels.hip"], cwd=csrc, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if r.returncode != 0:
        sys.exit("compile of %s/bbq_mfma_kernels.hip failed:\n%s" % (csrc, r.stdout[-3000:]))
    out, name = {}, None
    for line in r.stdout.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            out[name] = {}
            continue
        m = re.search(r"remark:\s+(VGPRs|AGPRs|Occupancy \[waves/SIMD\]|ScratchSize \[bytes/lane\]): (\d+)", line)
        if m and name:
            out[name][m.group(1).split()[0]] = int(m.group(2))
    names = sorted(out)
    dem = subprocess.run(["c++filt"], input="\n".join(names), stdout=subprocess.PIPE, text=True).stdout.splitlines()
    res = {}
    for n, d in zip(names, dem):
        m = re.search(r"bbq_scan_mfma_kernel<(.*?)>\(", d)
        if not m:
            continue
        args = [x.strip() for x in m.group(1).replace("(bool)", "").split(",")]
        v = out[n]
        res[(int(args[0]), args[1], args[2], int(args[3]), len(args) > 4)] = (v["VGPRs"] + v.get("AGPRs", 0), v["Occupancy"], v["ScratchSize"])
    return res


def main():
    before = table(sys.argv[1]) if len(sys.argv) > 2 else None
    after = table(sys.argv[-1])
    print("registers (vector + accumulator) / occupancy (waves per SIMD) / scratch (bytes per lane)")
    head = "%-34s " % "bbq_scan_mfma_kernel<W, COMPACT, FP, G>"
    if before is not None:
        head += "%-18s " % "unfiltered before"
    print(head + "%-18s %-18s" % ("unfiltered", "filtered"))
    touched = lost = scratch = 0
    for key in sorted(k for k in after if not k[4]):
        plain, filt = after[key], after.get(key[:4] + (True,))
        line = "%-34s " % ("%d, %s, %s, %d" % key[:4])
        mark = []
        if before is not None:
            line += "%-18s " % fmt(before.get(key))
            if before.get(key) != plain:
                touched += 1
                mark.append("UNFILTERED CHANGED")
        if filt and filt[1] < plain[1]:
            lost += 1
            mark.append("a wave short")
        if filt and filt[2] > plain[2]:   # (every kernel has the frame of the prologue's QueryParams copy; more than that is a spill)
            scratch += 1
            mark.append("SPILLS")
        print(line + "%-18s %-18s %s" % (fmt(plain), fmt(filt), ", ".join(mark)))
    print("\nunfiltered instantiations that differ from before: %s; filtered ones a wave short of their twin: %d; filtered ones with more scratch than their twin (spills): %d"
          % (touched if before is not None else "n/a", lost, scratch))


if __name__ == "__main__":
    main()
