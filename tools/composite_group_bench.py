#!/usr/bin/env python3
"""Kernel time of the partitioned GROUP BY over composite and NULL-able keys
(the group code, csrc/group_code.h) against the hash path that answered these
shapes before (MBX_PART_GROUP=0 selects it), alternating in one process.
GPU only.  Usage: composite_group_bench.py [rows] [groups]

  dense2   GROUP BY k1, k2: two INT32 keys, `groups` codes, dense
  hashed2  the same with k1 sparse (x 1 000 003, INT64): hashed partitions
  c3s_null the c3s key (g x 2654435761) made NULL-able, 1/7 NULL: hashed

Prints one JSON line per shape: per-kernel medians of both paths and whether
the sorted rows agree (checked once, over the pulled cells)."""
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
reps = int(os.environ.get("REPS", "4"))
cfg = m.Config.create()
cfg.set("mbx_profile", "true")
c = m.connect_with_config(cfg).value
V = "mbx_synth(9, i, 1099511627776) - 549755813888 AS v"
shapes = {
    "dense2": (f"CREATE TABLE t AS SELECT CAST(mbx_synth(7, i, {g1}) AS INTEGER) AS k1, "
               f"CAST(mbx_synth(13, i, {g2}) AS INTEGER) AS k2, {V} FROM range({n}) tbl(i)",
               "SELECT k1, k2, SUM(v), COUNT(*) FROM t GROUP BY k1, k2"),
    "hashed2": (f"CREATE TABLE t AS SELECT mbx_synth(7, i, {g1}) * 1000003 AS k1, "
                f"CAST(mbx_synth(13, i, {g2}) AS INTEGER) AS k2, {V} FROM range({n}) tbl(i)",
                "SELECT k1, k2, SUM(v), COUNT(*) FROM t GROUP BY k1, k2"),
    "c3s_null": (f"CREATE TABLE t AS SELECT CASE WHEN mbx_synth(19, i, 7) = 0 THEN NULL "
                 f"ELSE mbx_synth(7, i, {groups}) * 2654435761 END AS k, {V} FROM range({n}) tbl(i)",
                 "SELECT k, SUM(v), COUNT(*) FROM t GROUP BY k"),
}
if os.environ.get("SHAPES"):
    shapes = {k: v for k, v in shapes.items() if k in os.environ["SHAPES"].split(",")}


def run(sql, hash_path, cells=False):
    if hash_path:
        os.environ["MBX_PART_GROUP"] = "0"
    try:
        rr = c.query_raw(sql)
    finally:
        os.environ.pop("MBX_PART_GROUP", None)
    rows = sorted(tuple(r) for r in rr.cells()[0]) if cells else None
    rr.close()
    return {k["name"]: k["ms"] for k in c.last_profile()["kernels"]}, rows


for name, (setup, sql) in shapes.items():
    c.query("DROP TABLE IF EXISTS t")
    r = c.query(setup)
    assert hasattr(r, "value"), r.error.message
    _, new_rows = run(sql, False, cells=True)  # (also the warm-up of both paths)
    _, old_rows = run(sql, True, cells=True)
    kern = {False: [], True: []}
    for _ in range(reps):
        for hp in (False, True):
            kern[hp].append(run(sql, hp)[0])
    out = {"rows": n, "groups_out": len(new_rows), "rows_equal": new_rows == old_rows}
    for hp, label in ((False, "group_code"), (True, "hash_path")):
        med = {k: statistics.median(d[k] for d in kern[hp] if k in d) for k in kern[hp][-1]}
        out[label] = {"kernel_ms_median": med, "kernel_ms_sum": sum(med.values()),
                      "kernel_ms_sum_runs": [sum(d.values()) for d in kern[hp]]}
    print(name, json.dumps(out), flush=True)
c.close()
