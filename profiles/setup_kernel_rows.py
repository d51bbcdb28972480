#!/usr/bin/env python3
"""The setup rows of two per-kernel tables of a traced step side by side.

    python profiles/setup_kernel_rows.py r08/kernel_calls_256_parent.csv \
        r08/kernel_calls_256_branch.csv

The inputs have one line per kernel of a rocprofv3 kernel trace: kernel,
calls, total_ms, max_ms, first_ms, first_grid. Per row of the output: calls,
total ms and the longest call of each build. The "torch int64
chains" row adds up the torch and rocPRIM utility kernels of the setup phase
(sorts, histograms, index / scatter kernels, int64 adds, nonzero, arange and
integer fills); the native replacements are listed by name."""
import collections
import csv
import re
import sys

ROWS = [
    ("color_round_kernel", r"color_round_kernel"),
    ("agg_match_kernel", r"agg_match_kernel"),
    ("agg_propose_kernel", r"agg_propose_kernel"),
    ("agg_singleton_kernel", r"agg_singleton_kernel"),
    ("native orderings (key offsets, root flag / map, slab, int_max)",
     r"keys_to_offsets|root_flag|root_map|slab_lengths|slab_fill_kernel|"
     r"int_max_kernel|fill_int_kernel"),
    ("gather_kernel", r"amgx_hip::gather_kernel"),
    ("torch int64 chains and rocPRIM sorts / scans",
     r"rocprim|compute_cuda_kernel<long>|kernelHistogram1D|"
     r"index_elementwise_kernel|_scatter_gather_elementwise_kernel|"
     r"CUDAFunctor_add<long>|write_indices|arange_cuda_out|"
     r"FillFunctor<int>|FillFunctor<long>|radixSortKVInPlace|"
     r"bitonicSortKVInPlace|fill_reverse_indices|sort_postprocess"),
]


def table(path):
    out = collections.OrderedDict((name, [0, 0.0, 0.0]) for name, _ in ROWS)
    for r in csv.DictReader(open(path)):
        for name, pat in ROWS:
            if re.search(pat, r["kernel"]):
                e = out[name]
                e[0] += int(r["calls"])
                e[1] += float(r["total_ms"])
                e[2] = max(e[2], float(r["max_ms"]))
                break
    return out


def main():
    a, b = table(sys.argv[1]), table(sys.argv[2])
    print("| item | parent calls | ms | max call | branch calls | ms | max call |")
    print("|---|---|---|---|---|---|---|")
    for name in a:
        print("| %s | %d | %.1f | %.2f | %d | %.1f | %.2f |"
              % (name, *a[name], *b[name]))


if __name__ == "__main__":
    main()
