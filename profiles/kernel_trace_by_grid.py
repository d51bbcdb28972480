#!/usr/bin/env python3
"""Totals of a rocprofv3 csv output directory per kernel name and grid size.

A kernel_stats table has one line per kernel name; the per-color DILU kernels
run on every level under one name, and their grid size tells the levels apart
(grid = rows of the color x lanes, rounded up to the workgroup). For a
--kernel-trace run the columns are calls and total ms; for a --pmc run (its
own run, no tracing) the mean of every counter per call.

    python profiles/kernel_trace_by_grid.py DIR [NAME_REGEX] > table.csv
"""
import collections
import csv
import glob
import re
import sys


def pick(row, *names):
    for n in names:
        if n in row and row[n] != "":
            return row[n]
    return None


def short(name):
    """Head of the kernel name (template arguments kept), no namespace."""
    return name.replace("void ", "").replace("amgx_hip::", "")[:80]


def main():
    root = sys.argv[1]
    want = re.compile(sys.argv[2]) if len(sys.argv) > 2 else None
    ms = collections.defaultdict(float)
    calls = collections.Counter()
    ctr = collections.defaultdict(lambda: collections.defaultdict(float))
    seen = collections.defaultdict(set)
    for path in glob.glob(root + "/**/*.csv", recursive=True):
        if "stats" in path or "agent_info" in path:
            continue
        with open(path, newline="") as fh:
            for row in csv.DictReader(fh):
                name = pick(row, "Kernel_Name", "kernel_name")
                grid = pick(row, "Grid_Size_X", "Grid_Size", "grid_size")
                if name is None or grid is None:
                    continue
                if want is not None and not want.search(name):
                    continue
                key = (short(name), int(float(grid)))
                cname = pick(row, "Counter_Name", "counter_name")
                if cname is not None:
                    ctr[key][cname] += float(pick(row, "Counter_Value",
                                                  "counter_value") or 0)
                    seen[key].add(pick(row, "Dispatch_Id", "dispatch_id"))
                    continue
                t0 = pick(row, "Start_Timestamp", "start_timestamp")
                t1 = pick(row, "End_Timestamp", "end_timestamp")
                if t0 is None or t1 is None:
                    continue
                ms[key] += (int(t1) - int(t0)) * 1e-6
                calls[key] += 1
    out = csv.writer(sys.stdout)
    if ctr:
        names = sorted({c for v in ctr.values() for c in v})
        out.writerow(["kernel", "grid", "calls"] + [c + "_per_call"
                                                    for c in names])
        for key in sorted(ctr, key=lambda k: (k[0], -k[1])):
            n = max(len(seen[key]), 1)
            out.writerow([key[0], key[1], n]
                         + [f"{ctr[key][c] / n:.1f}" for c in names])
        return
    out.writerow(["kernel", "grid", "calls", "total_ms", "mean_us"])
    for key in sorted(ms, key=lambda k: (k[0], -k[1])):
        out.writerow([key[0], key[1], calls[key], f"{ms[key]:.3f}",
                      f"{ms[key] / calls[key] * 1e3:.2f}"])


if __name__ == "__main__":
    main()
