#!/usr/bin/env python3
"""str_match (csrc/str_kernels.hip) over a device table of 5-30-byte strings:
COUNT(*) under `s = c`, `s LIKE 'ab%'` and `s LIKE '%b%'`, the kernel time of
the str_match profile scope, and the algorithmic bytes (8 B/row of offsets +
the chars + 1 B/row out) over that time next to this box's ring-read figure of
duckdb_mbx_hbm_calibrate_ex from the same process.  The LDS-staged form and the
per-row global form (MBX_STR_GLOBAL=1) alternate launch by launch.  GPU only.
Usage: str_match_bench.py [rows] [steps] [warmup]; prints one JSON line per
statement and form."""
import json
import os
import statistics
import sys

os.environ["MBX_EXPERIMENTS"] = "1"  # the switch is read only with the opt-in (csrc/knobs.h)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402

WORDS = ["alpha", "abacus-07", "bravo-charlie", "delta-echo-foxtrot", "golf-hotel-india-juliet",
         "kilo-lima-mike-november-oscar!"]

m = ge._load()
n = int(sys.argv[1]) if len(sys.argv) > 1 else 100_000_000
steps = int(sys.argv[2]) if len(sys.argv) > 2 else 7
warmup = int(sys.argv[3]) if len(sys.argv) > 3 else 2
cfg = m.Config.create()
cfg.set("mbx_profile", "true")
c = m.connect_with_config(cfg).value


def rows(sql):
    r = c.query(sql)
    if not hasattr(r, "value"):
        raise SystemExit(f"{sql}: {r.error.message}")
    return r.value.rows


case = " ".join(f"WHEN {k} THEN '{w}'" for k, w in enumerate(WORDS[:-1]))
rows(f"CREATE TABLE t AS SELECT CASE mbx_synth(3, i, {len(WORDS)}) {case} ELSE '{WORDS[-1]}' END AS s "
     f"FROM range({n}) tbl(i)")
counts = [int(rows(f"SELECT COUNT(*) FROM t WHERE s = '{w}'")[0][0]) for w in WORDS]
assert sum(counts) == n, counts
chars = sum(k * len(w) for k, w in zip(counts, WORDS))
algo_bytes = 8 * (n + 1) + chars + n
cal = c.hbm_calibrate()
print(json.dumps({"rows": n, "chars_bytes": chars, "algorithmic_bytes": algo_bytes,
                  "ring_read_gbs": round(cal["ring_read_gbs"], 1), "read_gbs": round(cal["read_gbs"], 1)}), flush=True)

STATEMENTS = [("eq", f"SELECT COUNT(*) FROM t WHERE s = '{WORDS[2]}'", counts[2]),
              ("like_prefix", "SELECT COUNT(*) FROM t WHERE s LIKE 'ab%'", counts[1]),
              ("like_contains", "SELECT COUNT(*) FROM t WHERE s LIKE '%b%'", counts[1] + counts[2] + counts[5])]
for name, sql, want in STATEMENTS:
    ms = {"lds": [], "global": []}
    for rep in range(warmup + steps):
        for form in ("lds", "global"):
            os.environ["MBX_STR_GLOBAL"] = "1" if form == "global" else "0"
            got = int(rows(sql)[0][0])
            assert got == want, (name, form, got, want)
            ks = [k["ms"] for k in c.last_profile()["kernels"] if k["name"] == "str_match"]
            assert len(ks) == 1, ks
            if rep >= warmup:
                ms[form].append(ks[0])
    for form in ("lds", "global"):
        med = statistics.median(ms[form])
        print(json.dumps({"statement": name, "form": form, "kernel_ms_median": round(med, 4),
                          "kernel_ms_min": round(min(ms[form]), 4), "kernel_ms_max": round(max(ms[form]), 4),
                          "algorithmic_gbs": round(algo_bytes / med / 1e6, 1),
                          "of_ring_read": round(algo_bytes / med / 1e6 / cal["ring_read_gbs"], 3),
                          "steps": steps}), flush=True)
os.environ.pop("MBX_STR_GLOBAL", None)
c.close()
