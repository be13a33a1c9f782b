#!/usr/bin/env python3
"""Kernel time of the fused filter-aggregate over the benchmark's column
(x = mbx_synth(42, i, 50) + 1, BIGINT, codes of 6 bits) for predicates that
read different numbers of bit planes (csrc/scan_planes.h), and of building the
image.  One process measures one library: run it once per build (the library is
chosen with DUCKDB_MB_AMD_LIB) and alternate the builds.  GPU only.
Usage: [LABEL=name] [REPS=n] [SCAN_HIST=false] scan_planes_bench.py [rows]
(SCAN_HIST=false sets mbx_scan_hist: without it a library that keeps code
histograms answers these statements from them, and the figures are that path's)

Prints one JSON line for the setup: LABEL (what the run calls its build, e.g.
"parent" or "this build"; default the library's file name), REPS, and for each
of two CTAS of the table the wall time of the CTAS with a COUNT(*) that waits
for it (the first of a process also loads the code objects) and the CTAS's own
`scan_encode` profile entries.  Then one line per statement: the answer, the
`filter_agg` profile entry's bytes, and its kernel time over REPS (default 30)
runs after 3 warm-up runs: median, minimum and maximum."""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402

m = ge._load()
n = int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000_000
reps = max(3, int(os.environ.get("REPS", "30")))
cfg = m.Config.create()
cfg.set("mbx_profile", "true")
if os.environ.get("SCAN_HIST"):  # SCAN_HIST=false: the plane scan itself (a library without the option refuses the key)
    cfg.set("mbx_scan_hist", os.environ["SCAN_HIST"])
c = m.connect_with_config(cfg).value

label = os.environ.get("LABEL") or os.path.basename(m.LIB_PATH)
ctas_s, enc = [], []
for _ in range(2):  # the first CREATE TABLE of a process also loads the kernels' code objects
    c.query("DROP TABLE IF EXISTS t")
    t0 = time.perf_counter()
    r = c.query(f"CREATE TABLE t AS SELECT mbx_synth(42, i, 50) + 1 AS x FROM range({n}) tbl(i)")
    assert hasattr(r, "value"), r.error.message
    enc.append([k for k in c.last_profile()["kernels"] if k["name"] == "scan_encode"])  # the CTAS's own profile
    assert c.query("SELECT COUNT(*) FROM t").value.rows[0] == [str(n)]  # waits for the stream
    ctas_s.append(time.perf_counter() - t0)
print("setup", json.dumps({"rows": n, "label": label, "reps": reps, "ctas_s": ctas_s, "scan_encode": enc}), flush=True)

statements = {
    "c2_gt24": "SELECT COUNT(*) FROM t WHERE x > 24",
    "gt23": "SELECT COUNT(*) FROM t WHERE x > 23",
    "gt16": "SELECT COUNT(*) FROM t WHERE x > 16",
    "between_9_40": "SELECT COUNT(*) FROM t WHERE x BETWEEN 9 AND 40",
    "c5_sum_gt24": "SELECT COUNT(*), SUM(x) FROM t WHERE x > 24",
    "sum_gt23": "SELECT SUM(x) FROM t WHERE x > 23",
    "minmax_gt24": "SELECT COUNT(*), SUM(x), MIN(x), MAX(x) FROM t WHERE x > 24",
}
for name, sql in statements.items():
    ms, rows, nbytes = [], None, None
    for i in range(reps + 3):
        rr = c.query(sql)
        assert hasattr(rr, "value"), rr.error.message
        rows = rr.value.rows[0]
        fa = [k for k in c.last_profile()["kernels"] if k["name"] == "filter_agg"]
        assert len(fa) == 1, fa
        nbytes = fa[0]["bytes"]
        if i >= 3:
            ms.append(fa[0]["ms"])
    print(name, json.dumps({"sql": sql, "answer": rows, "bytes": nbytes, "kernel_ms_median": statistics.median(ms),
                            "kernel_ms_min": min(ms), "kernel_ms_max": max(ms),
                            "tb_per_s": nbytes / statistics.median(ms) / 1e9}), flush=True)
c.close()
