"""MIN / MAX over VARCHAR on the device (str_minmax.h; str_kernels.hip:
str_minmax_key, _live, _round, _rows), without GROUP BY, on the slot path
(group_assign), on the hash path, and through everything around an aggregate.

The model: min / max over s.encode() of a group's non-NULL values (bytes compare
unsigned, a prefix first: DuckDB's binary order), None when there are none.
Cells are compared as text, groups as sorted rows.  Every statement is run on a
profiled connection and must have launched str_minmax_key and no radix_sort:
the answer comes from the rounds, not from a sort.

The row appender takes NUL-terminated strings, so no table here holds a NUL
byte; the trailing-NUL order ("a" < "a\\0" < "a\\0\\0": equal chunk keys, the
length decides) is checked by the host program of test_str_minmax_plan.py, which
runs the same functions."""
import pytest

from conftest import q
from gpu_tables import fill, kernels

pytestmark = pytest.mark.gpu


def connect(mbx, **opts):
    cfg = mbx.Config.create()
    for k, v in dict(mbx_profile="true", **opts).items():
        assert isinstance(cfg.set(k, str(v)), mbx.Ok), (k, v)
    r = mbx.connect_with_config(cfg)
    assert isinstance(r, mbx.Ok), r.error.message
    return r.value


def ran(c, sql="", own_sort=False):
    """own_sort: the statement has an operator that sorts for itself (a join sorts its build keys, an
    ORDER BY its rows, both under the name radix_sort), so only the rounds are asked for"""
    ks = kernels(c)
    assert "str_minmax_key" in ks, (sql, ks)
    assert own_sort or "radix_sort" not in ks, (sql, ks)
    return ks


def cells(c, sql):
    """the statement's rows, None for a NULL cell"""
    res = c.query_raw(sql)
    try:
        text, nulls = res.cells()
        return [[None if n else t for t, n in zip(tr, nr)] for tr, nr in zip(text, nulls)]
    finally:
        res.close()


def lo(vals):
    xs = [v for v in vals if v is not None]
    return min(xs, key=lambda s: s.encode()) if xs else None


def hi(vals):
    xs = [v for v in vals if v is not None]
    return max(xs, key=lambda s: s.encode()) if xs else None


def srt(rows):
    return sorted(rows, key=lambda r: [(x is None, x or "") for x in r])


# the edge set of the host program (tests/plan_harness/str_minmax.cpp), without its NUL bytes: every
# length around the chunk borders, ties on the first 8 and 16 bytes, bytes >= 0x80 against ASCII
TOP = "\U0010FFFF" * 2  # F4 8F BF BF twice: eight bytes, above every other string here
EDGE = ["m" * n for n in (0, 1, 7, 8, 9, 15, 16, 17, 24, 25)] + \
       ["prefix08", "prefix08a", "prefix08b", "prefix08prefix16", "prefix08prefix16x", "prefix08prefix16y",
        "a", "z", "é", "日本", "日本語", "\x7f", TOP]
assert lo(EDGE) == "" and hi(EDGE) == TOP and len(set(EDGE)) == len(EDGE)


# ---- 1. global: the wave, the block and the grid-stride tail -------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 255, 256, 257, 1025])
def test_global_sizes(mbx, n):
    c = connect(mbx)
    vals = [EDGE[(r * 7 + 3) % len(EDGE)] for r in range(n)]
    fill(c, "t", "s VARCHAR", [(s,) for s in vals])
    sql = "SELECT MIN(s), MAX(s) FROM t"
    assert cells(c, sql) == [[lo(vals), hi(vals)]], (n, sql)
    ran(c, sql)  # (without rows nothing is launched; the profile still names the pass, with no bytes)
    assert cells(c, "SELECT MAX(s) FROM t") == [[hi(vals)]]
    assert cells(c, "SELECT MIN(DISTINCT s) FROM t") == [[lo(vals)]]
    c.close()


@pytest.mark.parametrize("which", ["smallest", "largest"])
def test_global_70001_extreme_in_the_last_row(mbx, which):
    """70 001 rows: 274 wave steps, the last of one row, which holds the only copy of the extreme"""
    c = connect(mbx)
    mid = [s for s in EDGE if s not in ("", TOP)]
    vals = [mid[(r * 5 + 1) % len(mid)] for r in range(70000)] + ["" if which == "smallest" else TOP]
    fill(c, "t", "s VARCHAR", [(s,) for s in vals])
    sql = "SELECT MIN(s), MAX(s) FROM t"
    assert cells(c, sql) == [[lo(vals), hi(vals)]]
    ran(c, sql)
    assert (lo(vals) if which == "smallest" else hi(vals)) == vals[-1]
    c.close()


# ---- 2. global: NULLs ------------------------------------------------------------------------------------
def test_global_nulls(mbx):
    c = connect(mbx)
    fill(c, "an", "s VARCHAR, v BIGINT", [(None, r) for r in range(300)])
    assert cells(c, "SELECT MIN(s), MAX(s) FROM an") == [[None, None]]
    ran(c)
    fill(c, "one", "s VARCHAR, v BIGINT", [("needle" if r == 613 else None, r) for r in range(1001)])
    assert cells(c, "SELECT MIN(s), MAX(s), COUNT(s), COUNT(*) FROM one") == [["needle", "needle", "1", "1001"]]
    ran(c)
    fill(c, "blank", "s VARCHAR, v BIGINT", [("" if r % 3 == 1 else None, r) for r in range(100)])
    assert cells(c, "SELECT MIN(s), MAX(s) FROM blank") == [["", ""]]
    ran(c)
    # every row filtered away: no row reaches the passes
    assert cells(c, "SELECT MIN(s), MAX(s), COUNT(*) FROM one WHERE v < 0") == [[None, None, "0"]]
    ran(c)
    c.close()


# ---- 3. ties past round 0 --------------------------------------------------------------------------------
def test_ties_past_round_0(mbx):
    """5000 rows that share 16 bytes and differ from byte 17 on: every row is a candidate, and the
    second and third chunk decide"""
    c = connect(mbx)
    tails = ["z", "é", "日本", "a", "zz", "y", "日", "é", "~"]
    vals = ["prefix08prefix16" + tails[r % len(tails)] + str(r % 7) for r in range(5000)]
    fill(c, "t", "s VARCHAR, k BIGINT", [(s, r % 3) for r, s in enumerate(vals)])
    sql = "SELECT MIN(s), MAX(s) FROM t"
    assert cells(c, sql) == [[lo(vals), hi(vals)]]
    ks = ran(c, sql)
    assert ks.count("str_minmax_round") > 1, ks
    assert hi(vals).startswith("prefix08prefix16日本") and lo(vals).startswith("prefix08prefix16a")
    # the same per group, and 'z' against the UTF-8 tails alone
    want = srt([[str(k), lo(vals[k::3]), hi(vals[k::3])] for k in range(3)])
    assert srt(cells(c, "SELECT k, MIN(s), MAX(s) FROM t GROUP BY k")) == want
    ran(c)
    fill(c, "u", "s VARCHAR", [(s,) for s in ["z", "é", "日本", "z"] * 50])
    assert cells(c, "SELECT MIN(s), MAX(s) FROM u") == [["z", "日本"]]
    ran(c)
    c.close()


# ---- 4. grouped ------------------------------------------------------------------------------------------
GN = 300003
STR = ["", "a", "prefix08", "prefix08a", "prefix08prefix16x", "prefix08prefix16y", "é", "日本"]
KS = [None, "", "g", "group_08", "group_08b", "group_08group_16!"]


def g_row(i):
    """(s, v, kn, ks) of row i: s is NULL in one row of 7; kn is NULL in one row of 13 and is 77777
    exactly in the rows whose s is NULL otherwise (a group without a non-NULL value)"""
    s = None if i % 7 == 3 else STR[(i % 1025) % 4 + ((i % 3) % 2) * 4]
    kn = None if i % 13 == 0 else 77777 if i % 7 == 3 else i % 100
    return s, (i * 37) % 1001 - 500, kn, KS[i % 6]


@pytest.fixture(scope="module")
def grouped(mbx):
    c = connect(mbx)
    # one CASE per statement: the expression VM's programs are short
    q(c, f"CREATE TABLE b0 AS SELECT range AS i FROM range({GN})")
    q(c, "CREATE TABLE b1 AS SELECT i, CASE WHEN i % 7 = 3 THEN -1 ELSE (i % 1025) % 4 + ((i % 3) % 2) * 4 END AS j FROM b0")
    q(c, "CREATE TABLE b2 AS SELECT i, j, (i * 37) % 1001 - 500 AS v, "
         "CASE WHEN i % 13 <> 0 AND i % 7 = 3 THEN 77777 WHEN i % 13 <> 0 THEN i % 100 END AS kn FROM b1")
    s_case = "CASE " + " ".join(f"WHEN j = {j} THEN '{s}'" for j, s in enumerate(STR)) + " END"
    q(c, f"CREATE TABLE b3 AS SELECT i, v, kn, {s_case} AS s FROM b2")
    ks_case = "CASE " + " ".join(f"WHEN i % 6 = {j} THEN '{s}'" for j, s in enumerate(KS) if s is not None) + " END"
    q(c, f"CREATE TABLE g AS SELECT i, v, kn, s, {ks_case} AS ks FROM b3")
    rows = [g_row(i) for i in range(GN)]
    # the table is what the model says it is
    assert cells(c, "SELECT COUNT(*), COUNT(s), COUNT(kn), COUNT(ks), SUM(v) FROM g") == [[
        str(GN), str(sum(r[0] is not None for r in rows)), str(sum(r[2] is not None for r in rows)),
        str(sum(r[3] is not None for r in rows)), str(sum(r[1] for r in rows))]]
    yield c, rows
    c.close()


AGGS = "MIN(s), MAX(s), COUNT(*), SUM(v), COUNT(s)"


def model(rows, keys):
    """sorted [key cells..., MIN(s), MAX(s), COUNT(*), SUM(v), COUNT(s)] of the groups of keys[i]"""
    groups = {}
    for key, r in zip(keys, rows):
        groups.setdefault(key, []).append(r)
    out = []
    for key, rs in groups.items():
        ss = [r[0] for r in rs]
        out.append([None if k is None else str(k) for k in key] +
                   [lo(ss), hi(ss), str(len(rs)), str(sum(r[1] for r in rs)), str(sum(s is not None for s in ss))])
    return srt(out)


@pytest.mark.parametrize("nk", [2, 32, 1024, 1025, 5000])
def test_grouped_bigint_key(grouped, nk):
    """the slot path (group_assign) on either side of the 1024 keys the LDS reduction would take: the
    VARCHAR aggregates turn that off for the whole select, and the integer columns must not change"""
    c, rows = grouped
    sql = f"SELECT i % {nk} AS k, {AGGS} FROM g GROUP BY k"
    assert srt(cells(c, sql)) == model(rows, [(i % nk,) for i in range(GN)])
    ks = ran(c, sql)
    assert "group_assign" in ks and "group_direct" not in ks, ks


def test_grouped_nullable_key_and_a_group_of_nulls(grouped):
    c, rows = grouped
    sql = f"SELECT kn, {AGGS} FROM g GROUP BY kn"
    got = srt(cells(c, sql))
    assert got == model(rows, [(r[2],) for r in rows])
    ran(c, sql)
    assert ["77777", None, None] in [r[:3] for r in got] and any(r[0] is None for r in got)


def test_grouped_varchar_and_two_column_keys(grouped):
    c, rows = grouped
    sql = f"SELECT ks, {AGGS} FROM g GROUP BY ks"
    assert srt(cells(c, sql)) == model(rows, [(r[3],) for r in rows])
    assert "hash_group_assign" in ran(c, sql)
    sql = f"SELECT i % 32 AS k, ks, {AGGS} FROM g GROUP BY k, ks"
    assert srt(cells(c, sql)) == model(rows, [(i % 32, r[3]) for i, r in enumerate(rows)])
    assert "hash_group_assign" in ran(c, sql)
    # only the VARCHAR aggregates, and MAX before MIN
    sql = "SELECT ks, MAX(s), MIN(s) FROM g GROUP BY ks"
    want = srt([[r[0], r[2], r[1]] for r in model(rows, [(r[3],) for r in rows])])
    assert srt(cells(c, sql)) == want
    ran(c, sql)


# ---- 5. around it ----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def around(mbx):
    c = connect(mbx)
    rows = [(None if r % 9 == 4 else EDGE[(r * 11 + r // 7) % len(EDGE)], r % 10, (r * 13) % 17) for r in range(2000)]
    fill(c, "t", "s VARCHAR, k BIGINT, v BIGINT", rows)
    dim = [(k, None if k == 3 else STR[(k * 5) % len(STR)]) for k in range(12)]  # keys 10, 11 find no fact row
    fill(c, "d", "k BIGINT, s VARCHAR", dim)
    yield c, rows, dim
    c.close()


def by_k(rows, keep=lambda r: True):
    out = {}
    for r in rows:
        if keep(r):
            out.setdefault(r[1], []).append(r[0])
    return out


def test_where_like(around):
    c, rows, _ = around
    kept = [r for r in rows if r[0] is not None and r[0].startswith("a")]
    assert cells(c, "SELECT MIN(s), COUNT(*) FROM t WHERE s LIKE 'a%'") == [[lo([r[0] for r in kept]), str(len(kept))]]
    ran(c)
    kept = [r for r in rows if r[0] is not None and r[0].startswith("prefix")]
    want = srt([[str(k), lo(v), hi(v)] for k, v in by_k(kept).items()])
    assert srt(cells(c, "SELECT k, MIN(s), MAX(s) FROM t WHERE s LIKE 'prefix%' GROUP BY k")) == want
    ran(c)


def test_having(around):
    c, rows, _ = around
    kept = [r for r in rows if r[2] == 5]  # few rows per group, so that the groups' minima differ
    want = srt([[str(k), lo(v)] for k, v in by_k(kept).items() if lo(v) is not None and lo(v).encode() > b"b"])
    assert 0 < len(want) < len(by_k(kept))
    assert srt(cells(c, "SELECT k, MIN(s) FROM t WHERE v = 5 GROUP BY k HAVING MIN(s) > 'b'")) == want
    ran(c)


def test_order_by_max_desc_limit(around):
    c, rows, _ = around
    kept = [r for r in rows if r[2] == 5]
    groups = [[str(k), hi(v)] for k, v in by_k(kept).items()]
    tops = sorted({g[1].encode() for g in groups if g[1] is not None}, reverse=True)
    got = cells(c, "SELECT k, MAX(s) FROM t WHERE v = 5 GROUP BY k ORDER BY MAX(s) DESC LIMIT 3")
    ran(c, own_sort=True)
    assert len(got) == 3 and len(groups) > 3
    # in order; groups that tie on MAX(s) may come in either order
    assert [g[1].encode() for g in got] == sorted((g[1].encode() for g in got), reverse=True)
    assert got[0][1].encode() == tops[0] and all(g in groups for g in got)
    nth = sorted((g[1].encode() for g in groups if g[1] is not None), reverse=True)[2]
    assert got[2][1].encode() == nth


def test_count_distinct_beside_min(around):
    c, rows, _ = around
    sql = "SELECT COUNT(DISTINCT v), MIN(s) FROM t"
    assert cells(c, sql) == [[str(len({r[2] for r in rows})), lo([r[0] for r in rows])]]
    ran(c, sql)
    want = srt([[str(k), str(len({r[2] for r in rows if r[1] == k})), hi(v)] for k, v in by_k(rows).items()])
    assert srt(cells(c, "SELECT k, COUNT(DISTINCT v), MAX(s) FROM t GROUP BY k")) == want
    ran(c)


def test_over_a_join(around):
    c, rows, dim = around
    name = dict(dim)
    joined = [(name[r[1]], r[2]) for r in rows]  # every fact row finds its key
    sql = "SELECT MIN(d.s), MAX(d.s), COUNT(*) FROM t f JOIN d ON f.k = d.k"
    assert cells(c, sql) == [[lo([j[0] for j in joined]), hi([j[0] for j in joined]), str(len(joined))]]
    ran(c, sql, own_sort=True)
    groups = {}
    for s, v in joined:
        groups.setdefault(v, []).append(s)
    want = srt([[str(v), lo(ss), hi(ss)] for v, ss in groups.items()])
    sql = "SELECT f.v, MIN(d.s), MAX(d.s) FROM t f JOIN d ON f.k = d.k GROUP BY f.v"
    assert srt(cells(c, sql)) == want
    ran(c, sql, own_sort=True)


def test_ctas_and_union_all(around):
    c, rows, _ = around
    want = srt([[str(k), lo(v)] for k, v in by_k(rows).items()])
    q(c, "CREATE TABLE mins AS SELECT k, MIN(s) AS m FROM t GROUP BY k")
    ran(c)
    assert srt(cells(c, "SELECT k, m FROM mins")) == want
    assert cells(c, "SELECT MAX(m) FROM mins") == [[hi([w[1] for w in want])]]
    q(c, "DROP TABLE mins")
    both = want + [[str(k), hi(v)] for k, v in by_k(rows).items()]
    sql = "SELECT k, MIN(s) FROM t GROUP BY k UNION ALL SELECT k, MAX(s) FROM t GROUP BY k"
    assert srt(cells(c, sql)) == srt(both)
    ran(c, sql)
    sql = "SELECT MIN(s) FROM t UNION ALL SELECT MAX(s) FROM t WHERE k = 4"
    assert srt(cells(c, sql)) == srt([[lo([r[0] for r in rows])], [hi([r[0] for r in rows if r[1] == 4])]])
    ran(c, sql)


def test_refused_forms_stay_refused(around):
    c, _, _ = around
    for sql in ("SELECT SUM(s) FROM t", "SELECT AVG(s) FROM t", "SELECT min(s) OVER (PARTITION BY k) FROM t"):
        r = c.query(sql)
        assert not hasattr(r, "value"), sql


# ---- 6. sharded ------------------------------------------------------------------------------------------
SHARD_ROWS = 3400


@pytest.mark.parametrize("null_shard", [False, True])
def test_sharded(mbx, null_shard):
    """three shards of one device; with null_shard the middle one holds NULLs only"""
    n = 10007

    def s_of(r):
        if r % 5 == 2 or (null_shard and SHARD_ROWS <= r < 2 * SHARD_ROWS):
            return None
        return EDGE[(r * 7 + r // 11) % (len(EDGE) - (r < 2 * SHARD_ROWS))]  # TOP only in the last shard

    rows = [(s_of(r), r % 37, r) for r in range(n)]
    sh = connect(mbx, gpu_devices="0,0,0", mbx_shard_rows=SHARD_ROWS, mbx_appender_flush_rows=SHARD_ROWS)
    assert sh.shard_stats()["shards"] == 3
    one = connect(mbx)
    for c in (sh, one):
        fill(c, "t", "s VARCHAR, k BIGINT, v BIGINT", rows)
    ss = [r[0] for r in rows]
    sql = "SELECT MIN(s), MAX(s), COUNT(s), COUNT(*) FROM t"
    want = [[lo(ss), hi(ss), str(sum(s is not None for s in ss)), str(n)]]
    assert cells(one, sql) == want and cells(sh, sql) == want
    ran(one, sql)
    ran(sh, sql)
    sql = "SELECT k, MIN(s), MAX(s), SUM(v) FROM t GROUP BY k"
    want = srt([[str(k), lo(v), hi(v), str(sum(r[2] for r in rows if r[1] == k))] for k, v in by_k(rows).items()])
    assert srt(cells(one, sql)) == want and srt(cells(sh, sql)) == want
    ran(sh, sql)
    sh.close()
    one.close()
