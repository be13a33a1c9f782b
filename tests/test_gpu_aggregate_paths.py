"""The order in which Aggregate() (csrc/aggregate.cpp) tries its paths, pinned:
one statement per path, the exact list of kernel names the query profile
reports, and the rows against numpy over the same data.

The tables are the smallest at which each path is still chosen: 4 099 rows
where the path has no floor (4 096 for the code image, so the table is exactly
`mbx_scan_codes_min_rows` apart from the option), 65 537 for the hashed and
the group-code partitioned paths (both start at 2^16 rows).  The group code
needs more than 4 096 codes: 300 x 100 here.  The run-time compiled kernels
are compiled synchronously (MBX_JIT=sync) where they are the subject and
switched off (MBX_JIT=0) where the paths behind them are, so no list depends
on how fast the compiler was.

The kernel lists were recorded on the build before Aggregate() became a
dispatcher; the dispatcher must reproduce them.

Two forms of the direct GROUP BY's launch plan (csrc/group_direct_plan.h) have
tables of their own, recorded on the build before the plan had a header:
f2_segmented (values near 2^56 leave 4096 rows between flushes, fewer than a
workgroup's share of 1 000 003 rows, so the segmented kernel runs) and
f2_refused (1001 key slots with every column NULL-able and MIN / MAX do not
fit beside the ring at three workgroups per CU: the launch is refused, which
still leaves its group_direct entry in the profile, F3 is skipped and, with the
run-time compiler off, group_assign and one group_reduce per aggregate answer)."""
import numpy as np
import pytest

from conftest import q

pytestmark = pytest.mark.gpu

N = 4_099
NP = 65_537  # the partitioned paths' floor is 2^16 rows


def _conn(mbx, codes_min_rows=None):
    cfg = mbx.Config.create()
    assert isinstance(cfg.set("mbx_profile", "true"), mbx.Ok)
    if codes_min_rows is not None:
        assert isinstance(cfg.set("mbx_scan_codes_min_rows", str(codes_min_rows)), mbx.Ok)
    r = mbx.connect_with_config(cfg)
    assert isinstance(r, mbx.Ok), r.error.message
    return r.value


def _profile(c):
    return c.last_profile()["kernels"]


def _kernels(c):
    return [kk["name"] for kk in _profile(c)]


# ---- the table and its numpy restatement ---------------------------------
T_SQL = ("CREATE TABLE t AS SELECT (i * 7919) % 50 + 1 AS x, (i * 104729) % 2000001 - 1000000 AS y, "
         "CAST((i * 31) % 300 AS INTEGER) AS k, "
         "CASE WHEN i % 7 = 0 THEN NULL ELSE CAST((i * 31) % 300 AS INTEGER) END AS kn, "
         "(i * 13) % 3000 AS kw, ((i * 11) % 1000) * 1000003 AS ks, "
         "CAST((i * 7) % 100 - 50 AS INTEGER) AS b, (i * 17) % 1000 AS w, "
         "CASE WHEN i % 3 = 0 THEN 'alpha' WHEN i % 3 = 1 THEN 'beta' ELSE NULL END AS s "
         "FROM range({n}) tbl(i)")
NULL = np.iinfo(np.int64).max  # stands for a NULL key: above every key here, so it sorts last


def _cols(n):
    i = np.arange(n, dtype=np.int64)
    k = (i * 31) % 300
    return {"x": (i * 7919) % 50 + 1, "y": (i * 104729) % 2000001 - 1000000, "k": k,
            "kn": np.where(i % 7 == 0, NULL, k), "kw": (i * 13) % 3000, "ks": ((i * 11) % 1000) * 1000003,
            "b": (i * 7) % 100 - 50, "w": (i * 17) % 1000, "s": np.where(i % 3 == 0, 0, np.where(i % 3 == 1, 1, NULL))}


def _scalar(v, mask, aggs):
    """one row of COUNT(*) / SUM / MIN / MAX over v[mask] (int64 sums: |v| <= 1e6, n < 2^17)"""
    sel = v[mask]
    f = {"count": lambda: len(sel), "sum": lambda: int(sel.sum()), "min": lambda: int(sel.min()),
         "max": lambda: int(sel.max())}
    return [[str(f[a]()) for a in aggs]]


def _grouped(keys, v, mask, aggs, names=None):
    """rows of a GROUP BY over the stacked keys in key order, NULL keys last and empty"""
    K = np.stack([kk[mask] for kk in keys], axis=1)
    v = v[mask]
    uk, inv = np.unique(K, axis=0, return_inverse=True)
    inv = inv.reshape(-1)
    cols = []
    for a in aggs:
        if a == "count":
            cols.append(np.bincount(inv, minlength=len(uk)))
        elif a == "sum":
            o = np.zeros(len(uk), dtype=np.int64)
            np.add.at(o, inv, v)
            cols.append(o)
        elif a == "min":
            o = np.full(len(uk), NULL)
            np.minimum.at(o, inv, v)
            cols.append(o)
        else:
            o = np.full(len(uk), -NULL)
            np.maximum.at(o, inv, v)
            cols.append(o)
    rows = []
    for g in range(len(uk)):
        kr = ["" if x == NULL else (names[x] if names else str(x)) for x in uk[g].tolist()]
        rows.append(kr + [str(int(c[g])) for c in cols])
    return rows


# ---- f2_segmented: 40 BIGINT keys, |v| up to 1000 * VS, just under 2^56 ----
NSEG = 1_000_003
VS = 72057594037927  # 2^56 // 1000
TSEG_SQL = ("CREATE TABLE t AS SELECT (i * 31) % 40 AS k, ((i * 104729) % 2001 - 1000) * " + str(VS) + " AS v "
            "FROM range({n}) tbl(i)")


def _seg_rows(n):
    """k, COUNT(*), SUM(v) in exact Python integers (the sums pass 2^63)"""
    i = np.arange(n, dtype=np.int64)
    k, c = (i * 31) % 40, (i * 104729) % 2001 - 1000
    cnt, csum = np.bincount(k, minlength=40), np.zeros(40, dtype=np.int64)
    np.add.at(csum, k, c)
    return [[str(g), str(int(cnt[g])), str(int(csum[g]) * VS)] for g in range(40)]


# ---- f2_refused: NULL-able INTEGER key of range 1000, two NULL-able BIGINT columns
TREF_SQL = ("CREATE TABLE t AS SELECT "
            "CASE WHEN i % 7 = 0 THEN NULL ELSE CAST((i * 31) % 1000 AS INTEGER) END AS kn, "
            "CASE WHEN i % 5 = 0 THEN NULL ELSE (i * 104729) % 2000001 - 1000000 END AS yn, "
            "CASE WHEN i % 11 = 0 THEN NULL ELSE (i * 17) % 1000 END AS wn FROM range({n}) tbl(i)")


def _ref_rows(n):
    """kn, SUM / MIN / MAX of yn and of wn over their non-NULL rows (NULL when a group has none), NULL key last"""
    i = np.arange(n, dtype=np.int64)
    kn = np.where(i % 7 == 0, 1000, (i * 31) % 1000)
    cols = [(i % 5 != 0, (i * 104729) % 2000001 - 1000000), (i % 11 != 0, (i * 17) % 1000)]
    rows = []
    for g in np.unique(kn).tolist():
        row = ["" if g == 1000 else str(g)]
        for ok, v in cols:
            sel = v[(kn == g) & ok]
            row += [str(int(sel.sum())), str(int(sel.min())), str(int(sel.max()))] if len(sel) else ["", "", ""]
        rows.append(row)
    return rows


ALL = slice(None)
CSMM = ["count", "sum", "min", "max"]
CS = ["count", "sum"]
FPROJ = ["vm_filter", "vm_project"]  # FilterProject ahead of the generic reductions (interpreted: MBX_JIT=0)

# id -> (rows, mbx_scan_codes_min_rows, MBX_JIT, sql, the profile's kernel names,
#        rows in key order?, numpy rows)
CASES = {
    "f1_values": (N, None, None, "SELECT COUNT(*), SUM(x), MIN(x), MAX(x) FROM t WHERE x > 24",
                  ["filter_agg"], True, lambda d: _scalar(d["x"], d["x"] > 24, CSMM)),
    "f1_codes": (4096, 1, None, "SELECT COUNT(*), SUM(x), MIN(x), MAX(x) FROM t WHERE x > 24",
                 ["filter_agg"], True, lambda d: _scalar(d["x"], d["x"] > 24, CSMM)),
    "f1_count_star": (N, None, None, "SELECT COUNT(*) FROM t",
                      [], True, lambda d: [[str(len(d["x"]))]]),
    "f1_zone_map_excluded": (4096, 1, None, "SELECT COUNT(*) FROM t WHERE x > 50",
                             ["filter_agg"], True, lambda d: [["0"]]),
    "filter_multi": (N, None, None, "SELECT COUNT(*), SUM(y) FROM t WHERE x > 24 AND w < 500",
                     ["filter_multi"], True, lambda d: _scalar(d["y"], (d["x"] > 24) & (d["w"] < 500), CS)),
    "f2_plain": (N, None, None, "SELECT k, COUNT(*), SUM(y), MIN(y), MAX(y) FROM t GROUP BY k",
                 ["group_direct"], True, lambda d: _grouped([d["k"]], d["y"], ALL, CSMM)),
    "f2_nullable_key": (N, None, None, "SELECT kn, COUNT(*), SUM(y), MIN(y), MAX(y) FROM t GROUP BY kn",
                        ["group_direct"], True, lambda d: _grouped([d["kn"]], d["y"], ALL, CSMM)),
    "f2_where_third_column": (N, None, None, "SELECT k, COUNT(*), SUM(y) FROM t WHERE w < 500 GROUP BY k",
                              ["group_direct"], True, lambda d: _grouped([d["k"]], d["y"], d["w"] < 500, CS)),
    "f2_segmented": (NSEG, None, None, "SELECT k, COUNT(*), SUM(v) FROM t GROUP BY k",
                     ["group_direct"], True, lambda d: d),
    "f2_refused": (N, None, "0", "SELECT kn, SUM(yn), MIN(yn), MAX(yn), SUM(wn), MIN(wn), MAX(wn) FROM t GROUP BY kn",
                   ["group_direct", "group_assign"] + 6 * ["group_reduce"], True, lambda d: d),
    "f3_range_above_1024": (N, None, None, "SELECT kw, COUNT(*), SUM(y), MIN(y), MAX(y) FROM t GROUP BY kw",
                            ["group_part"], True, lambda d: _grouped([d["kw"]], d["y"], ALL, CSMM)),
    "f3_hashed": (NP, None, None, "SELECT ks, COUNT(*), SUM(y), MIN(y), MAX(y) FROM t GROUP BY ks",
                  ["group_part_hashed"], False, lambda d: _grouped([d["ks"]], d["y"], ALL, CSMM)),
    "group_code_composite": (NP, None, None, "SELECT k, b, COUNT(*), SUM(y) FROM t GROUP BY k, b",
                             ["group_part"], True, lambda d: _grouped([d["k"], d["b"]], d["y"], ALL, CS)),
    "jit_aggregate": (N, None, "sync", "SELECT COUNT(*), SUM(x + 1) FROM t WHERE x > 24",
                      ["jit_aggregate"], True, lambda d: _scalar(d["x"] + 1, d["x"] > 24, CS)),
    "jit_group": (N, None, "sync", "SELECT k, COUNT(*), SUM(y + 1) FROM t GROUP BY k",
                  ["jit_group"], True, lambda d: _grouped([d["k"]], d["y"] + 1, ALL, CS)),
    "reduce_column": (N, None, "0", "SELECT COUNT(*), SUM(x + 1) FROM t WHERE x > 24",
                      FPROJ + ["reduce_column"], True, lambda d: _scalar(d["x"] + 1, d["x"] > 24, CS)),
    "direct_reduce_all": (N, None, "0", "SELECT k, COUNT(*), SUM(y + 1) FROM t WHERE w < 500 GROUP BY k",
                          FPROJ + ["group_direct"], True,
                          lambda d: _grouped([d["k"]], d["y"] + 1, d["w"] < 500, CS)),
    "group_assign_reduce": (N, None, "0", "SELECT kn, COUNT(*), SUM(y + 1) FROM t WHERE w < 500 GROUP BY kn",
                            FPROJ + ["group_assign", "group_reduce"], True,
                            lambda d: _grouped([d["kn"]], d["y"] + 1, d["w"] < 500, CS)),
    "hash_varchar_key": (N, None, "0", "SELECT s, COUNT(*), SUM(y) FROM t GROUP BY s",
                         ["hash_group_assign", "group_direct"], False,
                         lambda d: _grouped([d["s"]], d["y"], ALL, CS, names=["alpha", "beta"])),
    "distinct": (N, None, "0", "SELECT COUNT(DISTINCT x), SUM(x) FROM t",
                 ["filter_agg", "group_direct", "reduce_column"], True,
                 lambda d: [[str(len(np.unique(d["x"]))), str(int(d["x"].sum()))]]),
}
# the cases with a table of their own: its SQL and what the case's last entry is given
TABLES = {"f2_segmented": (TSEG_SQL, _seg_rows), "f2_refused": (TREF_SQL, _ref_rows)}


@pytest.mark.parametrize("case", list(CASES))
def test_path(mbx, monkeypatch, case):
    n, min_rows, jit, sql, kernels, ordered, want = CASES[case]
    if jit is not None:
        monkeypatch.setenv("MBX_JIT", jit)
    c = _conn(mbx, min_rows)
    table, cols = TABLES.get(case, (T_SQL, _cols))
    q(c, table.format(n=n))
    got = q(c, sql).rows
    prof = _profile(c)
    assert [kk["name"] for kk in prof] == kernels, (case, prof)
    if case == "f1_codes":  # the 1-byte image was read, not the 8-byte values
        assert prof[0]["bytes"] == n, prof
    if case == "f1_zone_map_excluded":  # the entry of a scan that never ran
        assert prof[0]["bytes"] == 0, prof
    rows = want(cols(n))
    assert (got if ordered else sorted(got)) == (rows if ordered else sorted(rows)), case
    c.close()
