#!/usr/bin/env python3
"""x [NOT] IN (subquery) on the device (the mark join: executor.cpp MarkLowering,
join_kernels.hip join_probe_mark) against the join that used to stand in for
it.  GPU only.
Usage: semi_join_bench.py [probe_rows] [set_keys,set_keys,...]

  SELECT COUNT(*) FROM f WHERE k IN (SELECT k FROM d)          -- "in"
  SELECT COUNT(*) FROM f WHERE k NOT IN (SELECT k FROM d)      -- "not_in"
  SELECT COUNT(*) FROM f JOIN (SELECT DISTINCT k FROM d) u ON f.k = u.k   -- the baseline

f has `probe_rows` rows (default 1e8) with one BIGINT key, d one row per
distinct key (default 1e3, 1e5 and 1e7 keys).  Each set size runs twice: every
probe row a member (f.k uniform over d's keys) and 10 % of them members (f.k
uniform over ten times as many values).

Three connections of this one process hold the same tables: the membership
statements run on the first, the baseline on the second as the engine runs it by
default (the fused probe-and-aggregate) and on the third with mbx_join_agg=false
(the materialising path, whose join_probe_count reads what join_probe_mark
reads).  The statements alternate, REPS (default 5) times after a warm-up each.
One JSON line per cell and statement: the median of every kernel's time per
launch, the bytes the executor counts for it, and the statement's time with its
least and greatest run.  Then an "expect" line per cell: join_probe_mark's and
join_probe_count's medians over the same table and probe column, the spread
(greatest minus least) of join_probe_count's own runs, and whether the mark
kernel's median exceeds the count kernel's by more than that spread.

First line: this device's ring-read ceiling from duckdb_mbx_hbm_calibrate_ex."""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402

m = ge._load()
n = int(float(sys.argv[1])) if len(sys.argv) > 1 else 100_000_000
sets = [int(float(x)) for x in sys.argv[2].split(",") if x] if len(sys.argv) > 2 else [1_000, 100_000, 10_000_000]
reps = max(3, int(os.environ.get("REPS", "5")))
BASE = "SELECT COUNT(*) FROM f JOIN (SELECT DISTINCT k FROM d) u ON f.k = u.k"
RUNS = (
    ("in", 0, "SELECT COUNT(*) FROM f WHERE k IN (SELECT k FROM d)"),
    ("not_in", 0, "SELECT COUNT(*) FROM f WHERE k NOT IN (SELECT k FROM d)"),
    ("join_fused", 1, BASE),
    ("join_materialised", 2, BASE),
)


def connect(**opts):
    cfg = m.Config.create()
    for k, v in dict(mbx_profile="true", **opts).items():
        assert hasattr(cfg.set(k, str(v)), "value"), (k, v)
    return m.connect_with_config(cfg).value


CONNS = (connect(), connect(mbx_join_agg="true", mbx_join_agg_max_run=1 << 30), connect(mbx_join_agg="false"))
cal = CONNS[0].hbm_calibrate()
print("calibrate", json.dumps({"ring_read_gbs": cal["ring_read_gbs"], "copy_gbs": cal["copy_gbs"]}), flush=True)


def must(c, sql):
    r = c.query(sql)
    assert hasattr(r, "value"), r.error.message
    return r.value


def everywhere(sql):
    for c in CONNS:
        must(c, sql)


def per_launch(profiles, name):
    """median over the runs of the kernel's time per launch, and the bytes of one launch"""
    per_run = []
    for p in profiles:
        ks = [x for x in p["kernels"] if x["name"] == name]
        if ks:
            per_run.append(sum(x["ms"] for x in ks) / len(ks))
    if not per_run:
        return None
    ks = [x for x in profiles[-1]["kernels"] if x["name"] == name]
    return {"ms": statistics.median(per_run), "ms_min": min(per_run), "ms_max": max(per_run), "launches": len(ks),
            "bytes": ks[0]["bytes"]}


def cell(head):
    answers = {tag: int(must(CONNS[ci], sql).rows[0][0]) for tag, ci, sql in RUNS}  # (also the warm-up)
    assert answers["in"] == answers["join_fused"] == answers["join_materialised"], answers
    assert answers["in"] + answers["not_in"] == n, answers  # neither side has a NULL
    runs = {tag: [] for tag, _, _ in RUNS}
    for _ in range(reps):
        for tag, ci, sql in RUNS:
            must(CONNS[ci], sql)
            runs[tag].append(CONNS[ci].last_profile())
    kern = {}
    for tag, _, _ in RUNS:
        ps = runs[tag]
        names = []
        for x in ps[-1]["kernels"]:
            if x["name"] not in names:
                names.append(x["name"])
        kern[tag] = {k: per_launch(ps, k) for k in names}
        for v in kern[tag].values():
            v["gb_per_s"] = v["bytes"] / (v["ms"] * 1e6) if v["ms"] > 0 else 0.0
        totals = [p["total_ms"] for p in ps]
        print("semi_join", json.dumps(dict(head, statement=tag, rows_out=answers[tag], kernels=kern[tag],
                                           statement_ms_median=statistics.median(totals), statement_ms_min=min(totals),
                                           statement_ms_max=max(totals))), flush=True)
    mark, count = kern["in"]["join_probe_mark"], kern["join_materialised"]["join_probe_count"]
    spread = count["ms_max"] - count["ms_min"]
    print("expect", json.dumps(dict(head, join_probe_mark_ms=mark["ms"], join_probe_mark_range_ms=[mark["ms_min"], mark["ms_max"]],
                                    join_probe_count_ms=count["ms"], join_probe_count_range_ms=[count["ms_min"], count["ms_max"]],
                                    join_probe_count_spread_ms=spread, mark_over_count=mark["ms"] / count["ms"],
                                    holds=mark["ms"] <= count["ms"] + spread)), flush=True)


for nd in sets:
    everywhere("DROP TABLE IF EXISTS d")
    everywhere(f"CREATE TABLE d AS SELECT i AS k FROM range({nd}) tbl(i)")
    for label, span in (("all_members", nd), ("members_10pct", 10 * nd)):
        everywhere("DROP TABLE IF EXISTS f")
        everywhere(f"CREATE TABLE f AS SELECT mbx_synth(5, i, {span}) AS k FROM range({n}) tbl(i)")
        cell({"probe_rows": n, "set_keys": nd, "case": label})
for c in CONNS:
    c.close()
