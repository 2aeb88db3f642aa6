#!/usr/bin/env python3
"""Registers, occupancy and scratch of EVERY bbq_scan_kernel instantiation, from the compiler's own remarks (no device needed).

  scripts/scan_resources.py CSRC_DIR                  one line per instantiation: VGPRs / occupancy (waves per SIMD) / scratch bytes per lane
  scripts/scan_resources.py BEFORE_DIR AFTER_DIR      the two side by side, the rows that differ marked, lost waves and new scratch counted

CSRC_DIR is a copy of better-binary-quantization_amd/csrc (e.g. `git archive HEAD better-binary-quantization_amd/csrc | tar -x -C DIR`
for the parent).  Compiles bbq_kernels.hip and bbq_filter_kernels.hip for the device only, with the Makefile's flags.
"""
import os
import re
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
FLAGS = "--offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -fno-fast-math -Rpass-analysis=kernel-resource-usage --cuda-device-only -c -o /dev/null".split()
FILES = ("bbq_kernels.hip", "bbq_filter_kernels.hip")


def remarks(csrc, f):
    r = subprocess.run([HIPCC] + FLAGS + [f], cwd=csrc, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if r.returncode != 0:
        sys.exit("compile of %s/%s failed:\n%s" % (csrc, f, r.stdout[-3000:]))
    return r.stdout


def table(csrc):
    with ThreadPoolExecutor(2) as ex:
        text = "".join(ex.map(lambda f: remarks(csrc, f), FILES))
    out, name = {}, None
    for line in text.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            out[name] = {}
            continue
        m = re.search(r"remark:\s+(VGPRs|Occupancy \[waves/SIMD\]|ScratchSize \[bytes/lane\]): (\d+)", line)
        if m and name:
            out[name][m.group(1).split()[0]] = int(m.group(2))
    names = sorted(out)
    dem = subprocess.run(["c++filt"], input="\n".join(names), stdout=subprocess.PIPE, text=True).stdout.splitlines()
    res = {}
    for n, d in zip(names, dem):
        m = re.search(r"bbq_scan_kernel<(.*?)>\(", d)
        if not m:
            continue
        v = out[n]
        key = m.group(1).replace("(bool)", "").replace("unsigned long const*", "accept")
        parts = key.split(", ")
        if len(parts) > 6 and parts[6] == "1":  # TPW = 1 is the kernel a tree without the parameter has: the same key for both
            del parts[6]
            key = ", ".join(parts)
        res[key] = (v["VGPRs"], v["Occupancy"], v["ScratchSize"])
    return res


def fmt(v):
    return "%d / %d / %d" % v if v else "-"


def main():
    if len(sys.argv) == 2:
        for k, v in sorted(table(sys.argv[1]).items()):
            print("%-44s %s" % (k, fmt(v)))
        return
    before, after = table(sys.argv[1]), table(sys.argv[2])
    lost = scratch = changed = 0
    print("%-44s %-16s %-16s" % ("bbq_scan_kernel<QB, W, MODE, SB, RS, DG[, TPW > 1][, accept]>", "before", "after"))
    for k in sorted(set(before) | set(after)):
        b, a = before.get(k), after.get(k)
        mark = ""
        if a != b:
            changed += 1
            mark = "changed"
            if a and b and a[1] < b[1]:
                lost += 1
                mark = "LOST A WAVE"
            if a and b and a[2] > b[2]:
                scratch += 1
                mark = "SCRATCH"
        print("%-44s %-16s %-16s %s" % (k, fmt(b), fmt(a), mark))
    print("\ninstantiations: %d before, %d after; changed: %d; lost a wave: %d; gained scratch: %d" % (len(before), len(after), changed, lost, scratch))


if __name__ == "__main__":
    main()
