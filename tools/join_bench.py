#!/usr/bin/env python3
"""Kernel times of the inner equi-join (csrc/join.cpp, join_kernels.hip) from
the statement profile.  GPU only.
Usage: join_bench.py [probe_rows] [build_keys,build_keys,...]

  SELECT COUNT(*), SUM(f.v + d.w) FROM f JOIN d ON f.k = d.k

f has `probe_rows` rows (default 1e8) with a BIGINT key and a BIGINT value, d
one row per distinct key (default 1e3, 1e5 and 1e7 keys) with a BIGINT value.
Each build size runs twice: every probe row matching (f.k uniform over d's
keys) and 10 % matching (f.k uniform over ten times as many values).  Prints
one JSON line per case: the median over REPS (default 5) runs of each join
kernel's time, of the build side's sort and of the gathers, the bytes the
executor counts for each pass, the rest of the statement (the projection and
the aggregate over the joined rows), and, first, this device's ring-read
ceiling from duckdb_mbx_hbm_calibrate_ex."""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402

m = ge._load()
n = int(float(sys.argv[1])) if len(sys.argv) > 1 else 100_000_000
builds = [int(float(x)) for x in sys.argv[2].split(",")] if len(sys.argv) > 2 else [1_000, 100_000, 10_000_000]
reps = max(3, int(os.environ.get("REPS", "5")))
JOIN = ("join_keys", "radix_sort", "join_build", "join_probe_count", "join_expand", "join_gather")
SQL = "SELECT COUNT(*), SUM(f.v + d.w) FROM f JOIN d ON f.k = d.k"

cfg = m.Config.create()
cfg.set("mbx_profile", "true")
c = m.connect_with_config(cfg).value
cal = c.hbm_calibrate()
print("calibrate", json.dumps({"ring_read_gbs": cal["ring_read_gbs"], "copy_gbs": cal["copy_gbs"]}), flush=True)


def must(sql):
    r = c.query(sql)
    assert hasattr(r, "value"), r.error.message
    return r.value


for nd in builds:
    must("DROP TABLE IF EXISTS d")
    must(f"CREATE TABLE d AS SELECT i AS k, mbx_synth(11, i, 1000) AS w FROM range({nd}) tbl(i)")
    for label, span in (("all_match", nd), ("match_10pct", 10 * nd)):
        must("DROP TABLE IF EXISTS f")
        must(f"CREATE TABLE f AS SELECT mbx_synth(5, i, {span}) AS k, mbx_synth(6, i, 1000) AS v FROM range({n}) tbl(i)")
        answer = must(SQL).rows[0]  # (also the warm-up)
        runs = []
        for _ in range(reps):
            must(SQL)
            runs.append(c.last_profile())
        ms, nbytes = {}, {}
        for name in JOIN:
            per_run = [sum(k["ms"] for k in p["kernels"] if k["name"] == name) for p in runs]
            ms[name] = statistics.median(per_run)
            nbytes[name] = sum(k["bytes"] for k in runs[-1]["kernels"] if k["name"] == name)
        rest = statistics.median(sum(k["ms"] for k in p["kernels"] if k["name"] not in JOIN) for p in runs)
        total = statistics.median(p["total_ms"] for p in runs)
        gbs = {k: (nbytes[k] / (ms[k] * 1e6) if ms[k] > 0 else 0.0) for k in JOIN}
        print("join", json.dumps({"probe_rows": n, "build_keys": nd, "case": label, "rows_out": int(answer[0]),
                                  "sum": answer[1], "kernel_ms_median": ms, "pass_bytes": nbytes, "pass_gb_per_s": gbs,
                                  "other_kernels_ms_median": rest, "statement_ms_median": total}), flush=True)
c.close()
