#!/usr/bin/env python3
"""Kernel time of the partitioned GROUP BY under a WHERE (the predicates run
inside its hist and scatter passes, csrc/group_pred_plan.h) against the path
that answered these statements before -- FilterProject, then the hash path;
MBX_PART_GROUP=0 selects it -- alternating in one process.  GPU only.
Usage: group_where_bench.py [rows] [groups]

  c3h     one dense INT64 key, `groups` keys
  c3s     the same key sparse (x 2654435761): hashed partitions
  dense2  GROUP BY k1, k2: two INT32 keys, `groups` codes, dense

Each with WHERE x > 24 (x a BIGINT column of its own in 1..50: selectivity
0.52) and, in the same run, without the WHERE.  Prints one JSON line per shape:
the statement's profile-scope kernel time, medians of REPS (default 4) runs of
either path, and whether the sorted rows of the two paths agree (checked once,
over the pulled cells)."""
import json
import os
import statistics
import sys

os.environ["MBX_EXPERIMENTS"] = "1"  # the library reads MBX_PART_GROUP only with this opt-in
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402

m = ge._load()
n = int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000_000
groups = int(sys.argv[2]) if len(sys.argv) > 2 else 100_000
g1 = max(1, int(round(groups ** 0.5)))
g2 = max(1, groups // g1)
reps = max(4, int(os.environ.get("REPS", "4")))
cfg = m.Config.create()
cfg.set("mbx_profile", "true")
c = m.connect_with_config(cfg).value
V = "mbx_synth(9, i, 1099511627776) - 549755813888 AS v, mbx_synth(42, i, 50) + 1 AS x"
shapes = {
    "c3h": (f"CREATE TABLE t AS SELECT mbx_synth(7, i, {groups}) AS k, {V} FROM range({n}) tbl(i)",
            "SELECT k, SUM(v), COUNT(*) FROM t {w} GROUP BY k"),
    "c3s": (f"CREATE TABLE t AS SELECT mbx_synth(7, i, {groups}) * 2654435761 AS k, {V} FROM range({n}) tbl(i)",
            "SELECT k, SUM(v), COUNT(*) FROM t {w} GROUP BY k"),
    "dense2": (f"CREATE TABLE t AS SELECT CAST(mbx_synth(7, i, {g1}) AS INTEGER) AS k1, "
               f"CAST(mbx_synth(13, i, {g2}) AS INTEGER) AS k2, {V} FROM range({n}) tbl(i)",
               "SELECT k1, k2, SUM(v), COUNT(*) FROM t {w} GROUP BY k1, k2"),
}
if os.environ.get("SHAPES"):
    shapes = {k: v for k, v in shapes.items() if k in os.environ["SHAPES"].split(",")}


def run(sql, old_path, cells=False):
    if old_path:
        os.environ["MBX_PART_GROUP"] = "0"
    try:
        rr = c.query_raw(sql)
    finally:
        os.environ.pop("MBX_PART_GROUP", None)
    rows = sorted(tuple(r) for r in rr.cells()[0]) if cells else None
    rr.close()
    return {k["name"]: k["ms"] for k in c.last_profile()["kernels"]}, rows


def summary(runs):
    med = {k: statistics.median(d[k] for d in runs if k in d) for k in runs[-1]}
    sums = [sum(d.values()) for d in runs]
    return {"kernel_ms_median": med, "kernel_ms_sum_median": statistics.median(sums), "kernel_ms_sum_runs": sums}


for name, (setup, tmpl) in shapes.items():
    c.query("DROP TABLE IF EXISTS t")
    r = c.query(setup)
    assert hasattr(r, "value"), r.error.message
    where, plain = tmpl.format(w="WHERE x > 24"), tmpl.format(w="")
    _, new_rows = run(where, False, cells=True)  # (also the warm-up of both paths)
    _, old_rows = run(where, True, cells=True)
    run(plain, False)
    kern = {"where_new": [], "where_old": [], "no_where": []}
    for _ in range(reps):
        kern["where_new"].append(run(where, False)[0])
        kern["where_old"].append(run(where, True)[0])
        kern["no_where"].append(run(plain, False)[0])
    out = {"rows": n, "groups_out": len(new_rows), "rows_equal": new_rows == old_rows}
    for label, runs in kern.items():
        out[label] = summary(runs)
    out["old_over_new"] = out["where_old"]["kernel_ms_sum_median"] / out["where_new"]["kernel_ms_sum_median"]
    out["where_over_no_where"] = out["where_new"]["kernel_ms_sum_median"] / out["no_where"]["kernel_ms_sum_median"]
    print(name, json.dumps(out), flush=True)
c.close()
