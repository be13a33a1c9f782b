#!/usr/bin/env python3
"""Summarises a `rocprofv3 --kernel-trace --output-format csv` run of one-row
aggregate steps (tools/c2_loop.py): per step, which kernels ran, how long each
took and how long the device stood idle between them.  A step starts at a
filter_agg_* kernel and takes the emit_agg / host_copy kernels that follow it.
Usage: trace_gaps.py DIR (searched for *kernel_trace.csv); prints JSON."""
import csv
import glob
import json
import statistics
import sys

KNOWN = ("filter_agg_hist_kernel", "filter_agg_lds_kernel", "emit_agg_kernel", "host_copy_kernel")


def short(name):
    for k in KNOWN:
        if k in name:
            return k
    return name.split("(")[0][:60]


files = glob.glob(sys.argv[1] + "/**/*kernel_trace.csv", recursive=True)
rows = []
for f in files:
    for r in csv.DictReader(open(f)):
        rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), short(r["Kernel_Name"])))
rows.sort()
dur, gap, span, per_step = {}, {}, [], []
i = 0
while i < len(rows):
    if not rows[i][2].startswith("filter_agg_"):
        i += 1
        continue
    j = i + 1
    while j < len(rows) and rows[j][2] in ("emit_agg_kernel", "host_copy_kernel") and j - i < 3:
        j += 1
    step = rows[i:j]
    per_step.append(len(step))
    for k, (a, b, n) in enumerate(step):
        dur.setdefault(n, []).append(b - a)
        if k:
            gap.setdefault(step[k - 1][2] + " -> " + n, []).append(a - step[k - 1][1])
    span.append(step[-1][1] - step[0][0])
    i = j


def med(v):
    return statistics.median(v) / 1000.0


print(json.dumps({"files": len(files), "kernels_total": len(rows), "steps": len(span),
                  "kernels_per_step_median": statistics.median(per_step) if per_step else None,
                  "kernel_duration_median_us": {k: med(v) for k, v in dur.items()},
                  "gap_median_us": {k: med(v) for k, v in gap.items()},
                  "first_kernel_start_to_last_kernel_end_median_us": med(span) if span else None}, indent=1))
