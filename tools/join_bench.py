#!/usr/bin/env python3
"""Kernel times of the inner equi-join (csrc/join.cpp, join_kernels.hip) from
the statement profile, the fused probe-and-aggregate against the materialising
path.  GPU only.
Usage: join_bench.py [probe_rows] [build_keys,build_keys,...] [skew_runs,...]

  SELECT COUNT(*), SUM(f.v + d.w) FROM f JOIN d ON f.k = d.k

f has `probe_rows` rows (default 1e8) with a BIGINT key and a BIGINT value, d
one row per distinct key (default 1e3, 1e5 and 1e7 keys) with a BIGINT value.
Each build size runs twice: every probe row matching (f.k uniform over d's
keys) and 10 % matching (f.k uniform over ten times as many values).

Every cell runs on two connections of this one process, mbx_join_agg=true
(with mbx_join_agg_max_run out of the way, so that the fused kernel runs
whatever the runs are) and mbx_join_agg=false, alternating statement by
statement, REPS (default 5) times after a warm-up each.  Prints one JSON line
per cell and mode: the median of each join kernel's time, of the build side's
sort and of the gathers, the bytes the executor counts for each pass, the rest
of the statement, and the statement's own time with its least and greatest run;
then an "ab" line: the two medians, their ratio and whether the two modes'
ranges over the runs are apart.  The `false` lines are also the check that the
materialising path has not moved (profiles/join/).

The skewed sweep (default r = 2, 4, ... 1024; "-" skips it): 1e5 build keys of
which one in 256 has a run of r rows and the rest one row, every probe row
matching.  A tile of the fused kernel costs as many interpreter passes as the
longest run among its 256 probe rows, so this is its bad case; the sweep is
what the default of mbx_join_agg_max_run is read from.

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
builds = [int(float(x)) for x in sys.argv[2].split(",") if x] if len(sys.argv) > 2 else [1_000, 100_000, 10_000_000]
skews = [2 ** i for i in range(1, 11)]
if len(sys.argv) > 3:
    skews = [] if sys.argv[3] == "-" else [int(x) for x in sys.argv[3].split(",")]
reps = max(3, int(os.environ.get("REPS", "5")))
JOIN = ("join_keys", "radix_sort", "join_build", "join_probe_count", "join_expand", "join_gather", "join_probe_agg",
        "join_agg_fold")
SQL = "SELECT COUNT(*), SUM(f.v + d.w) FROM f JOIN d ON f.k = d.k"
SKEW_KEYS = 100_000


def connect(**opts):
    cfg = m.Config.create()
    for k, v in dict(mbx_profile="true", **opts).items():
        assert hasattr(cfg.set(k, str(v)), "value"), (k, v)
    return m.connect_with_config(cfg).value


MODES = (("fused", connect(mbx_join_agg="true", mbx_join_agg_max_run=1 << 30)), ("materialised", connect(mbx_join_agg="false")))
cal = MODES[0][1].hbm_calibrate()
print("calibrate", json.dumps({"ring_read_gbs": cal["ring_read_gbs"], "copy_gbs": cal["copy_gbs"]}), flush=True)


def must(c, sql):
    r = c.query(sql)
    assert hasattr(r, "value"), r.error.message
    return r.value


def both(sql):
    for _, c in MODES:
        must(c, sql)


def cell(tag, head):
    """the statement on both connections, alternating; one line per mode, then the comparison"""
    answers = {name: must(c, SQL).rows[0] for name, c in MODES}  # (also the warm-up)
    assert answers["fused"] == answers["materialised"], answers
    runs = {name: [] for name, _ in MODES}
    for _ in range(reps):
        for name, c in MODES:
            must(c, SQL)
            runs[name].append(c.last_profile())
    stmt = {}
    for name, _ in MODES:
        ps = runs[name]
        ms, nbytes = {}, {}
        for k in JOIN:
            per_run = [sum(x["ms"] for x in p["kernels"] if x["name"] == k) for p in ps]
            if not any(per_run):
                continue
            ms[k] = statistics.median(per_run)
            nbytes[k] = sum(x["bytes"] for x in ps[-1]["kernels"] if x["name"] == k)
        rest = statistics.median(sum(x["ms"] for x in p["kernels"] if x["name"] not in JOIN) for p in ps)
        totals = [p["total_ms"] for p in ps]
        stmt[name] = totals
        gbs = {k: (nbytes[k] / (ms[k] * 1e6) if ms[k] > 0 else 0.0) for k in ms}
        print(tag, json.dumps(dict(head, mode=name, rows_out=int(answers[name][0]), sum=answers[name][1], kernel_ms_median=ms,
                                   pass_bytes=nbytes, pass_gb_per_s=gbs, other_kernels_ms_median=rest,
                                   statement_ms_median=statistics.median(totals), statement_ms_min=min(totals),
                                   statement_ms_max=max(totals))), flush=True)
    f, o = stmt["fused"], stmt["materialised"]
    print(tag + "_ab", json.dumps(dict(head, fused_ms=statistics.median(f), materialised_ms=statistics.median(o),
                                       fused_over_materialised=statistics.median(f) / statistics.median(o),
                                       fused_range_ms=[min(f), max(f)], materialised_range_ms=[min(o), max(o)],
                                       verdict="faster" if max(f) < min(o) else "slower" if min(f) > max(o) else "within spread")),
          flush=True)


for nd in builds:
    both("DROP TABLE IF EXISTS d")
    both(f"CREATE TABLE d AS SELECT i AS k, mbx_synth(11, i, 1000) AS w FROM range({nd}) tbl(i)")
    for label, span in (("all_match", nd), ("match_10pct", 10 * nd)):
        both("DROP TABLE IF EXISTS f")
        both(f"CREATE TABLE f AS SELECT mbx_synth(5, i, {span}) AS k, mbx_synth(6, i, 1000) AS v FROM range({n}) tbl(i)")
        cell("join", {"probe_rows": n, "build_keys": nd, "case": label})

if skews:
    nd = SKEW_KEYS
    both("DROP TABLE IF EXISTS f")
    both(f"CREATE TABLE f AS SELECT mbx_synth(5, i, {nd}) AS k, mbx_synth(6, i, 1000) AS v FROM range({n}) tbl(i)")
    long_keys = (nd + 255) // 256
    for r in skews:
        # rows 0 .. nd - 1: one per key; then r - 1 more rows for every 256th key
        total = nd + long_keys * (r - 1)
        both("DROP TABLE IF EXISTS d")
        both(f"CREATE TABLE d AS SELECT CASE WHEN i < {nd} THEN i ELSE ((i - {nd}) // {r - 1}) * 256 END AS k, "
             f"mbx_synth(11, i, 1000) AS w FROM range({total}) tbl(i)")
        cell("skew", {"probe_rows": n, "build_keys": nd, "long_run": r, "build_rows": total})
for _, c in MODES:
    c.close()
