#!/usr/bin/env python3
"""Kernel and statement times of the window functions (csrc/window.cpp,
window_kernels.hip) from the statement profile.  GPU only.
Usage: window_bench.py [rows] [partitions,partitions,...]

t has `rows` rows (default 1e8) of two BIGINT columns: k uniform over
`partitions` values (default 1e5, and 1: a single partition) and v uniform
over 1e6 values.  Three window selects, each wrapped so that its column stays
on the device and only one row comes back:

  SELECT COUNT(x), MAX(x) FROM (SELECT <call> AS x FROM t) s

  ROW_NUMBER() OVER (PARTITION BY k ORDER BY v)
  SUM(v) OVER (PARTITION BY k ORDER BY v)
  SUM(v) OVER ()

Each runs REPS (default 5) times after a warm-up.  Prints one JSON line per
statement: per kernel name the launches, the median of the summed time, the
time per launch, the bytes the executor counts per launch and the GB/s that
makes; the other kernels' time; the statement's median, least and greatest
time.  First line: this device's ring-read ceiling from
duckdb_mbx_hbm_calibrate_ex.  A first measurement: nothing is tuned or
accepted against these figures."""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402

m = ge._load()
n = int(float(sys.argv[1])) if len(sys.argv) > 1 else 100_000_000
parts = [int(float(x)) for x in sys.argv[2].split(",") if x] if len(sys.argv) > 2 else [100_000, 1]
reps = max(3, int(os.environ.get("REPS", "5")))
CALLS = ("ROW_NUMBER() OVER (PARTITION BY k ORDER BY v)", "SUM(v) OVER (PARTITION BY k ORDER BY v)", "SUM(v) OVER ()")
WINDOW = ("radix_sort", "window_bounds", "window_scan_reduce", "window_scan_carry", "window_scan_apply", "window_emit")

cfg = m.Config.create()
assert hasattr(cfg.set("mbx_profile", "true"), "value")
c = m.connect_with_config(cfg).value
cal = c.hbm_calibrate()
print("calibrate", json.dumps({"ring_read_gbs": cal["ring_read_gbs"], "copy_gbs": cal["copy_gbs"]}), flush=True)


def must(sql):
    r = c.query(sql)
    assert hasattr(r, "value"), r.error.message
    return r.value


for np_ in parts:
    must("DROP TABLE IF EXISTS t")
    must(f"CREATE TABLE t AS SELECT mbx_synth(5, i, {np_}) AS k, mbx_synth(6, i, 1000000) AS v FROM range({n}) tbl(i)")
    for call in CALLS:
        sql = f"SELECT COUNT(x), MAX(x) FROM (SELECT {call} AS x FROM t) s"
        answer = must(sql).rows[0]  # (also the warm-up)
        runs = []
        for _ in range(reps):
            must(sql)
            runs.append(c.last_profile())
        kern = {}
        for k in WINDOW:
            per_run = [sum(x["ms"] for x in p["kernels"] if x["name"] == k) for p in runs]
            launches = sum(1 for x in runs[-1]["kernels"] if x["name"] == k)
            if not launches:
                continue
            nbytes = sum(x["bytes"] for x in runs[-1]["kernels"] if x["name"] == k)
            ms = statistics.median(per_run)
            kern[k] = {"launches": launches, "ms": ms, "ms_per_launch": ms / launches, "bytes_per_launch": nbytes / launches,
                       "gb_per_s": nbytes / (ms * 1e6) if ms > 0 else 0.0}
        rest = statistics.median(sum(x["ms"] for x in p["kernels"] if x["name"] not in WINDOW) for p in runs)
        totals = [p["total_ms"] for p in runs]
        print("window", json.dumps({"rows": n, "partitions": np_, "call": call, "count": answer[0], "max": answer[1],
                                    "kernels": kern, "other_kernels_ms_median": rest,
                                    "statement_ms_median": statistics.median(totals), "statement_ms_min": min(totals),
                                    "statement_ms_max": max(totals)}), flush=True)
c.close()
