#!/usr/bin/env python3
"""Registers, occupancy and scratch of EVERY bbq_scan_kernel instantiation, from the compiler's own remarks (no device needed).

  scripts/scan_resources.py CSRC_DIR                  one line per instantiation: VGPRs / occupancy (waves per SIMD) / scratch bytes per lane;
                                                      fails if a kernel with several tiles per wave exceeds its recorded registers / waves (TWIN_BUDGET) or has any v_pk_*_f32 left
  scripts/scan_resources.py BEFORE_DIR AFTER_DIR      the two side by side, the rows that differ marked, lost waves and new scratch counted
  scripts/scan_resources.py BEFORE_DIR AFTER_DIR --files A.hip,B.hip
                                                      the same for EVERY kernel of the named files, by demangled name: the code object's register,
                                                      scratch and LDS records and the occupancy remark, and the instruction counts; fails if the
                                                      two trees' kernel symbols or any record differ

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


def packed_f32_in_twins(csrc):
    """v_pk_*_f32 instructions in the kernels with several tiles per wave (bbq_kernels.hip): their bound is written so that the compiler does
    not pack it (tile_bound_passes, bbq_scan_body.h); name -> count"""
    flags = [f for f in FLAGS if not f.startswith("-Rpass")]
    flags[flags.index("-c")] = "-S"
    flags[flags.index("/dev/null")] = "-"
    r = subprocess.run([HIPCC] + flags + [FILES[0]], cwd=csrc, stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, text=True)
    if r.returncode != 0:
        sys.exit("compile of %s/%s to assembly failed" % (csrc, FILES[0]))
    out, name = {}, None
    for line in r.stdout.splitlines():
        m = re.match(r"(_ZN3bbq15bbq_scan_kernelILi\d+ELi\d+ELi\d+ELi\d+ELb1ELb1ELi([248])E\S*):", line)
        if m:
            name = m.group(1)
            out[name] = 0
        elif name and line.startswith("\t.size\t" + name):
            name = None
        elif name and re.match(r"\tv_pk_\w+_f32", line):
            out[name] += 1
    return out


# What the kernels with several tiles per wave came out of the compiler with when their tile loop was last changed (ROCm 7.2): vector
# registers and waves per SIMD by TPW, per chunks of a row.  Their loop holds values in place with empty asms and a scheduling barrier
# (per_tile, keep_unpacked, tile_digit_sums in bbq_scan_body.h), each of which pins what that compiler did: a twin above its line here - more
# registers, fewer waves, any scratch - means a later compiler does something else with them.
TWIN_BUDGET = {6: {2: (51, 8), 4: (51, 8), 8: (50, 8)}, 8: {2: (59, 8), 4: (59, 8), 8: (58, 8)}, 12: {2: (75, 6), 4: (75, 6), 8: (74, 6)}}


def twins_over_budget(res):
    over = []
    for key, (vgprs, waves, scratch) in res.items():
        parts = key.split(", ")
        if len(parts) < 7 or not parts[6].isdigit() or int(parts[6]) < 2:
            continue
        budget = TWIN_BUDGET.get(int(parts[1]), {}).get(int(parts[6]))
        if budget and (vgprs > budget[0] or waves < budget[1] or scratch > 0):
            over.append("%s: %d registers / %d waves / %d scratch, recorded %d / %d / 0" % (key, vgprs, waves, scratch, budget[0], budget[1]))
    return over


def fmt(v):
    return "%d / %d / %d" % v if v else "-"


RECORD = ("vgpr_count", "sgpr_count", "private_segment_fixed_size", "group_segment_fixed_size")


def kernel_records(csrc, f):
    """every kernel of one file, by demangled name: its code object's .vgpr_count / .sgpr_count / .private_segment_fixed_size /
    .group_segment_fixed_size, the compiler's Occupancy remark, and its instructions (lines of its text that are no label, directive or comment)"""
    flags = [x for x in FLAGS if x not in ("-c", "-o", "/dev/null")] + ["-S", "-o", "-"]
    r = subprocess.run([HIPCC] + flags + [f], cwd=csrc, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    if r.returncode != 0:
        sys.exit("compile of %s/%s failed:\n%s" % (csrc, f, r.stderr[-3000:]))
    occ, name = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
        m = re.search(r"remark:\s+Occupancy \[waves/SIMD\]: (\d+)", line)
        if m and name:
            occ[name] = int(m.group(1))
    meta, cur, insts, name = [], None, {}, None
    for line in r.stdout.splitlines():
        m = re.match(r"(  - |    )\.(\w+):\s+(\S+)$", line)       # a kernel's own keys in amdhsa.kernels (its arguments' lie deeper)
        if m:
            if m.group(1) == "  - ":
                cur = {}
                meta.append(cur)
            cur[m.group(2)] = m.group(3)
            continue
        m = re.match(r"(\w+):", line)
        if m and m.group(1) in occ:
            name = m.group(1)
            insts[name] = 0
        elif name and line.startswith("\t.size\t" + name):
            name = None
        elif name and re.match(r"\t[a-z]\w*(\s|$)", line):
            insts[name] += 1
    meta = {k["name"]: k for k in meta if "name" in k}
    assert set(meta) == set(occ) == set(insts), (f, sorted(set(meta) ^ set(occ)))
    names = sorted(meta)
    dem = subprocess.run(["c++filt"], input="\n".join(names), stdout=subprocess.PIPE, text=True).stdout.splitlines()
    return {re.sub(r"\(.*\)$", "", d.replace("void bbq::(anonymous namespace)::", "").replace("(bool)", "")):
            tuple(int(meta[n][k]) for k in RECORD) + (occ[n], insts[n]) for n, d in zip(names, dem)}


def compare_files(before_dir, after_dir, files):
    with ThreadPoolExecutor(4) as ex:
        before = list(ex.map(lambda f: kernel_records(before_dir, f), files))
        after = list(ex.map(lambda f: kernel_records(after_dir, f), files))
    print("per kernel: %s / occupancy [waves/SIMD]; then instructions before -> after" % " / ".join("." + k for k in RECORD))
    bad = 0
    for f, b, a in zip(files, before, after):
        differ = sorted(k for k in set(b) | set(a) if (b.get(k) or (None,))[:-1] != (a.get(k) or (None,))[:-1])
        bad += len(differ)
        print("\n%s: %d kernels before, %d after; the same symbols: %s; records that differ: %d; instructions %d -> %d" % (
            f, len(b), len(a), "yes" if set(b) == set(a) else "NO", len(differ), sum(v[-1] for v in b.values()), sum(v[-1] for v in a.values())))
        for k in sorted(set(b) | set(a)):
            vb, va = b.get(k), a.get(k)
            rec = lambda v: " / ".join(str(x) for x in v[:-1]) if v else "-"
            print("  %-64s %-24s %-24s %6s -> %-6s %s" % (k, rec(vb), rec(va), vb[-1] if vb else "-", va[-1] if va else "-", "DIFFERS" if k in differ else ""))
    if bad:
        sys.exit("%d kernels whose records differ" % bad)


def main():
    if len(sys.argv) == 5 and sys.argv[3] == "--files":
        return compare_files(sys.argv[1], sys.argv[2], sys.argv[4].split(","))
    if len(sys.argv) == 2:
        res = table(sys.argv[1])
        for k, v in sorted(res.items()):
            print("%-44s %s" % (k, fmt(v)))
        over = twins_over_budget(res)
        if over:
            sys.exit("kernels with several tiles per wave above their recorded resources:\n  " + "\n  ".join(over))
        pk = packed_f32_in_twins(sys.argv[1])
        print("\nv_pk_*_f32 in the %d kernels with several tiles per wave: %d" % (len(pk), sum(pk.values())))
        if sum(pk.values()):
            sys.exit("the twins' bound is packed again: see tile_bound_passes (bbq_scan_body.h)")
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
