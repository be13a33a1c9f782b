#!/usr/bin/env python3
"""C2 steps (`SELECT COUNT(*) FROM t WHERE x > 24`, or the SQL given) over a
1e6-row table, timed one by one from Python as tools/query_overhead.py does.
GPU only.  Usage: c2_loop.py PROFILE(true|false) STEPS [SQL]

C2_FLOORS0=1 sets the code, plane and histogram floors to 0, so the small table
runs the kernels of the 1e9-row step (filter_agg_hist); C2_TAIL=false sets
mbx_result_tail.  Run it under `rocprofv3 --kernel-trace` and give the output
directory to tools/trace_gaps.py for the device timeline of a step
(profiles/result_tail/)."""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402

m = ge._load()
prof, steps = sys.argv[1], int(sys.argv[2])
sql = sys.argv[3] if len(sys.argv) > 3 else "SELECT COUNT(*) FROM t WHERE x > 24"
cfg = m.Config.create()
cfg.set("mbx_profile", prof)
if os.environ.get("C2_FLOORS0"):
    for k in ("mbx_scan_codes_min_rows", "mbx_scan_codes_planes_min_rows", "mbx_scan_hist_min_rows"):
        cfg.set(k, "0")
if os.environ.get("C2_TAIL"):
    cfg.set("mbx_result_tail", os.environ["C2_TAIL"])
c = m.connect_with_config(cfg).value
c.query("CREATE TABLE t AS SELECT mbx_synth(42, i, 50) + 1 AS x FROM range(1000000) tbl(i)")
ts = []
for i in range(steps):
    t0 = time.perf_counter()
    rr = c.query_raw(sql)
    v = rr.value(0, 0)
    rr.close()
    ts.append(time.perf_counter() - t0)
print(json.dumps({"profile": prof, "sql": sql, "steps": steps, "value": str(v),
                  "median_us": statistics.median(ts[50:]) * 1e6, "min_us": min(ts) * 1e6}))
c.close()
