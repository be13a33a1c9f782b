#!/usr/bin/env python3
"""MIN / MAX over VARCHAR (csrc/str_minmax.h, csrc/str_kernels.hip) over a
device table of 5-30-byte strings: the kernel time per launch of the
str_minmax_* profile scopes, their sum per statement (medians of 5), the bytes
the scopes count and this box's ring-read figure of duckdb_mbx_hbm_calibrate_ex
from the same process.  Statements: MIN(s), MAX(s) without GROUP BY, grouped by
a 32-value key, grouped by a 1e5-value key, and MIN / MAX of a 3-value "status"
column, where a third of all rows survive round 0.

The only earlier way to the ungrouped answer was
SELECT s FROM t WHERE s IS NOT NULL ORDER BY s LIMIT 1; its kernel-time sum is
recorded beside it.  One process measures one library (chosen with
DUCKDB_MB_AMD_LIB): run it once per build, MODE=sort for a build without the
aggregate, and alternate the processes.  GPU only.
Usage: [LABEL=name] [MODE=minmax|sort] str_minmax_bench.py [rows] [steps] [warmup];
prints one JSON line for the setup and one per statement."""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402

WORDS = ["alpha", "abacus-07", "bravo-charlie", "delta-echo-foxtrot", "golf-hotel-india-juliet",
         "kilo-lima-mike-november-oscar!"]
STATUS = ["open", "closed", "pending"]

m = ge._load()
n = int(sys.argv[1]) if len(sys.argv) > 1 else 100_000_000
steps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
warmup = int(sys.argv[3]) if len(sys.argv) > 3 else 2
mode = os.environ.get("MODE", "minmax")
label = os.environ.get("LABEL", os.path.basename(m.LIB_PATH))
cfg = m.Config.create()
cfg.set("mbx_profile", "true")
c = m.connect_with_config(cfg).value


def rows(sql):
    r = c.query(sql)
    if not hasattr(r, "value"):
        raise SystemExit(f"{sql}: {r.error.message}")
    return r.value.rows


case = " ".join(f"WHEN {k} THEN '{w}'" for k, w in enumerate(WORDS[:-1]))
rows(f"CREATE TABLE t0 AS SELECT mbx_synth(3, i, {len(WORDS)}) AS w, mbx_synth(5, i, 32) AS k32, "
     f"mbx_synth(7, i, 100000) AS k1e5, mbx_synth(9, i, 3) AS st FROM range({n}) tbl(i)")
rows(f"CREATE TABLE t1 AS SELECT k32, k1e5, st, CASE w {case} ELSE '{WORDS[-1]}' END AS s FROM t0")
scase = " ".join(f"WHEN {k} THEN '{w}'" for k, w in enumerate(STATUS[:-1]))
rows(f"CREATE TABLE t AS SELECT k32, k1e5, s, CASE st {scase} ELSE '{STATUS[-1]}' END AS status FROM t1")
rows("DROP TABLE t0")
rows("DROP TABLE t1")
counts = [int(rows(f"SELECT COUNT(*) FROM t WHERE s = '{w}'")[0][0]) for w in WORDS]
assert sum(counts) == n, counts
chars = sum(k * len(w) for k, w in zip(counts, WORDS))
cal = c.hbm_calibrate()
print(json.dumps({"label": label, "mode": mode, "rows": n, "chars_bytes": chars, "steps": steps,
                  "ring_read_gbs": round(cal["ring_read_gbs"], 1), "read_gbs": round(cal["read_gbs"], 1)}), flush=True)

def by_bytes(xs):
    """(least, greatest) in the byte order of the device"""
    return min(xs, key=lambda s: s.encode()), max(xs, key=lambda s: s.encode())


if mode == "sort":
    STATEMENTS = [("sort_limit_1", "SELECT s FROM t WHERE s IS NOT NULL ORDER BY s LIMIT 1", [[by_bytes(WORDS)[0]]])]
else:
    STATEMENTS = [("global", "SELECT MIN(s), MAX(s) FROM t", [list(by_bytes(WORDS))]),
                  ("group_32", "SELECT k32, MIN(s), MAX(s) FROM t GROUP BY k32", 32),
                  ("group_1e5", "SELECT k1e5, MIN(s), MAX(s) FROM t GROUP BY k1e5", 100000),
                  ("status", "SELECT MIN(status), MAX(status) FROM t", [list(by_bytes(STATUS))])]

for name, sql, want in STATEMENTS:
    total, per = [], {}
    for rep in range(warmup + steps):
        got = rows(sql)
        if isinstance(want, int):
            # (1e8 rows put every word in every group)
            assert len(got) == want and all(g[1:] == list(by_bytes(WORDS)) for g in got), (name, len(got), got[:2])
        else:
            assert got == want, (name, got, want)
        ks = c.last_profile()["kernels"]
        if rep < warmup:
            continue
        mine = [k for k in ks if mode == "sort" or k["name"].startswith("str_minmax")]
        total.append(sum(k["ms"] for k in mine))
        seen = {}
        for k in mine:
            seen.setdefault(k["name"], []).append(k)
        for nm, launches in seen.items():
            e = per.setdefault(nm, {"launches": len(launches), "ms": [], "bytes": sum(k.get("bytes", 0) for k in launches)})
            e["ms"].append(sum(k["ms"] for k in launches))
    med = statistics.median(total)
    out = {"label": label, "statement": name, "sql": sql, "kernel_ms_sum_median": round(med, 4),
           "kernel_ms_sum_min": round(min(total), 4), "kernel_ms_sum_max": round(max(total), 4), "steps": steps, "passes": {}}
    for nm, e in per.items():
        pm = statistics.median(e["ms"])
        out["passes"][nm] = {"launches": e["launches"], "ms_median": round(pm, 4),
                             "ms_per_launch": round(pm / e["launches"], 4), "bytes": e["bytes"],
                             "gbs": round(e["bytes"] / pm / 1e6, 1) if pm > 0 else None,
                             "of_ring_read": round(e["bytes"] / pm / 1e6 / cal["ring_read_gbs"], 3) if pm > 0 else None}
    print(json.dumps(out, ensure_ascii=False), flush=True)
c.close()
