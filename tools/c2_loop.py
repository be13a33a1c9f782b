#!/usr/bin/env python3
"""C2 steps (`SELECT COUNT(*) FROM t WHERE x > 24`, or the SQL given) over a
1e6-row table, timed one by one from Python as tools/query_overhead.py does.
GPU only.  Usage: c2_loop.py PROFILE(true|false) STEPS [SQL]

C2_FLOORS0=1 sets the code, plane and histogram floors and the floor of the
host answer to 0, so the small table takes the path of the 1e9-row step (the
histogram's host answer; with C2_HOST=false, which sets mbx_scan_hist_host, the
filter_agg_hist kernel); C2_TAIL=false sets mbx_result_tail, C2_SPIN=US sets
mbx_tail_spin_us (0: block on the stream).  The line it prints also carries
duckdb_mbx_tail_wait_stats and duckdb_mbx_scan_hist_host_stats over the loop and
the process's resident set in kB before and after it (the soak runs of
profiles/tail_wait/ and profiles/hist_host/).  Run it under `rocprofv3 --kernel-trace` and give the output
directory to tools/trace_gaps.py for the device timeline of a step
(profiles/result_tail/)."""
import array
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
    for k in ("mbx_scan_codes_min_rows", "mbx_scan_codes_planes_min_rows", "mbx_scan_hist_min_rows",
              "mbx_scan_hist_host_min_rows"):
        cfg.set(k, "0")
if os.environ.get("C2_HOST"):
    cfg.set("mbx_scan_hist_host", os.environ["C2_HOST"])
if os.environ.get("C2_TAIL"):
    cfg.set("mbx_result_tail", os.environ["C2_TAIL"])
if os.environ.get("C2_SPIN"):
    cfg.set("mbx_tail_spin_us", os.environ["C2_SPIN"])
c = m.connect_with_config(cfg).value
c.query("CREATE TABLE t AS SELECT mbx_synth(42, i, 50) + 1 AS x FROM range(1000000) tbl(i)")


def rss_kb():
    with open("/proc/self/status") as f:
        return next(int(ln.split()[1]) for ln in f if ln.startswith("VmRSS:"))


for i in range(50):  # warm: the pool, the event pairs, the statement's allocations
    c.query_raw(sql).close()
if prof == "true":
    c.profile_drain()
ts = array.array("d", [0.0]) * steps  # (made before the first resident-set reading, so the loop allocates nothing)
w0, h0, rss0 = c.tail_wait_stats(), c.scan_hist_host_stats(), rss_kb()
for i in range(steps):
    t0 = time.perf_counter()
    rr = c.query_raw(sql)
    v = rr.value(0, 0)
    rr.close()
    ts[i] = time.perf_counter() - t0
    if prof == "true" and (i + 1) % 50000 == 0:
        c.profile_drain()  # (the history keeps 100000 entries)
w1, h1, rss1 = c.tail_wait_stats(), c.scan_hist_host_stats(), rss_kb()
ts = sorted(ts)
print(json.dumps({"profile": prof, "sql": sql, "steps": steps, "value": str(v),
                  "median_us": statistics.median(ts) * 1e6, "min_us": ts[0] * 1e6,
                  "p90_us": ts[int(0.90 * (len(ts) - 1))] * 1e6, "p99_us": ts[int(0.99 * (len(ts) - 1))] * 1e6, "mean_us": sum(ts) / len(ts) * 1e6,
                  "tail_wait": {k: w1[k] - w0[k] for k in ("polled", "blocked", "wait_ns")},
                  "hist_host": {k: h1[k] - h0[k] for k in ("answered", "fetches", "declined")},
                  "rss_kb": [rss0, rss1]}))
c.close()
