"""The result tail (csrc/result_tail.h): the kernel that emits the one row of an
aggregate without GROUP BY also stores it in the host's mapped buffer where that
row is the statement's own result, so ToHost waits once and copies nothing.

Every case runs on two connections over the same rows, mbx_result_tail true and
false.  The cells of the two are compared exactly, and with Python integers
over the generated rows (AVG within 2^-51 of the exact quotient: the 128-bit
sum and the division each round once).  Which way the result reached the host
comes from the counters of duckdb_mbx_result_tail_stats.  The code, plane and
histogram floors are 0, as test_gpu_scan_hist.py sets them, so the small tables
take the paths the large ones do."""
import numpy as np
import pytest

from conftest import q

pytestmark = pytest.mark.gpu

SIZES = [1, 33, 8193, (1 << 20) + 1]
AGGS = ["COUNT(*)", "COUNT({c})", "SUM({c})", "MIN({c})", "MAX({c})", "AVG({c})"]
WIDE = 1 << 33  # z spans more than 2^32: no code image, the raw values are scanned


def connect(mbx, tail, **opts):
    cfg = mbx.Config.create()
    base = dict(mbx_profile="true", mbx_scan_codes_min_rows=0, mbx_scan_codes_planes_min_rows=0,
                mbx_scan_hist_min_rows=0, mbx_result_tail="true" if tail else "false")
    for k, v in dict(base, **opts).items():
        assert isinstance(cfg.set(k, str(v)), mbx.Ok), (k, v)
    r = mbx.connect_with_config(cfg)
    assert isinstance(r, mbx.Ok), r.error.message
    return r.value


class Pair:
    """the connection with the tail and the one without; tables go to both"""
    def __init__(self, mbx, **opts):
        self.mbx = mbx
        self.on, self.off = connect(mbx, True, **opts), connect(mbx, False, **opts)

    def __iter__(self):
        return iter((self.on, self.off))

    def run(self, sql):
        for c in self:
            q(c, sql)

    def load(self, name, decl, cols):
        """table `name` (`decl`) from numpy columns through the appender"""
        for c in self:
            q(c, f"CREATE TABLE {name} ({decl})")
            ap = c.create_appender("main", name).value
            for i, a in enumerate(cols):
                assert isinstance(ap.append_column(i, a), self.mbx.Ok)
            r = ap.commit(len(cols[0]))
            assert isinstance(r, self.mbx.Ok), r.error.message
            ap.close()

    def close(self):
        for c in self:
            c.close()


def rows_of(c, sql):
    """the statement's rows as text, None for NULL"""
    res = q(c, sql)
    return [[None if res.nulls[i][j] else res.rows[i][j] for j in range(len(res.rows[i]))] for i in range(res.row_count())]


def ran(c, f):
    """f()'s value and how many results took the tail and the copy kernel meanwhile"""
    s0 = c.result_tail_stats()
    v = f()
    s1 = c.result_tail_stats()
    return v, s1["tail"] - s0["tail"], s1["host_copy"] - s0["host_copy"]


def both(p, sql, tail=True):
    """the rows of `sql`, equal on both connections; the tail ran on the first alone (tail=False: on neither)"""
    got, t, h = ran(p.on, lambda: rows_of(p.on, sql))
    assert (t, h) == ((1, 0) if tail else (0, h)), (sql, t, h)
    ref, t, h = ran(p.off, lambda: rows_of(p.off, sql))
    assert t == 0 and (h == 1 or not tail), (sql, t, h)
    assert got == ref, (sql, got, ref)
    return got


def row(p, sql, tail=True):
    got = both(p, sql, tail)
    assert len(got) == 1, (sql, got)
    return got[0]


def table(n):
    """x in 1..50 (planes and histogram), y in 0..65535 (field codes), z wide (raw values), w INTEGER in -100..100"""
    r = np.random.default_rng(77 + n)
    x = r.integers(1, 51, size=n, dtype=np.int64)
    y = r.integers(0, 65536, size=n, dtype=np.int64)
    z = r.integers(-5, 6, size=n, dtype=np.int64) * WIDE + r.integers(0, 1000, size=n, dtype=np.int64)
    w = r.integers(-100, 101, size=n, dtype=np.int64).astype(np.int32)
    if n >= 2:
        x[0], x[-1], y[0], y[-1], z[0], z[-1] = 1, 50, 0, 65535, -5 * WIDE, 5 * WIDE + 999
    return x, y, z, w


DECL = "x BIGINT, y BIGINT, z BIGINT, w INTEGER"


def expect(v, lo, hi):
    """COUNT(*), COUNT, SUM, MIN, MAX as cells and AVG as a float, over the values lo <= v <= hi"""
    sel = v[(v >= lo) & (v <= hi)] if lo <= hi else v[:0]
    if not len(sel):
        return ["0", "0", None, None, None], None
    total = int(sel.sum())  # (|v| < 2^37 and at most 2^20 + 1 rows: no int64 overflow)
    return [str(len(sel)), str(len(sel)), str(total), str(int(sel.min())), str(int(sel.max()))], total / len(sel)


def check_aggs(p, t, col, v, where, lo, hi):
    cells, avg = expect(v, lo, hi)
    for a, want in zip(AGGS[:5], cells):
        assert row(p, f"SELECT {a.format(c=col)} FROM {t} WHERE {where}") == [want], (t, col, where, a)
    got = row(p, f"SELECT AVG({col}) FROM {t} WHERE {where}") + row(
        p, "SELECT " + ", ".join(a.format(c=col) for a in AGGS) + f" FROM {t} WHERE {where}")
    assert got[1:6] == cells, (t, col, where, got)
    for g in (got[0], got[6]):
        if avg is None:
            assert g is None, (t, col, where, got)
        else:
            assert abs(float(g) - avg) <= 2.0**-51 * abs(avg), (t, col, where, g, avg)


@pytest.mark.parametrize("hist", [True, False], ids=["hist", "planes"])
def test_scan_aggregate_branches(mbx, hist):
    """histogram or planes (x), field codes (y), raw values (z); a usual predicate, one the zone map
    rules out, one it lets through whole (the known count), and no predicate at all"""
    p = Pair(mbx, mbx_scan_hist="true" if hist else "false")
    for n in SIZES:
        t = f"t{n}"
        x, y, z, _ = cols = table(n)
        p.load(t, DECL, cols)
        for col, v in (("x", x), ("y", y), ("z", z)):
            if not hist and col != "x":
                continue  # mbx_scan_hist changes the path of x alone
            vmin, vmax = int(v.min()), int(v.max())
            mid = (vmin + vmax) // 2
            check_aggs(p, t, col, v, f"{col} > {mid}", mid + 1, vmax)
            check_aggs(p, t, col, v, f"{col} BETWEEN {vmin + 1} AND {mid}", vmin + 1, mid)
            check_aggs(p, t, col, v, f"{col} > {vmax}", vmax + 1, vmax)  # ruled out: NULLs beside COUNT 0
            check_aggs(p, t, col, v, f"{col} >= {vmin}", vmin, vmax)  # let through whole
        assert row(p, f"SELECT COUNT(*) FROM {t}") == [str(n)]
        assert row(p, f"SELECT COUNT(*), SUM(x) FROM {t}") == [str(n), str(int(x.sum()))]
        p.run(f"DROP TABLE {t}")
    p.close()


@pytest.fixture(scope="module")
def pt(mbx):
    """the pair with the 8193-row table t and the small typed tables"""
    p = Pair(mbx)
    p.cols = table(8193)
    p.load("t", DECL, p.cols)
    r = np.random.default_rng(5)
    p.d = r.integers(100, 5001, size=3001, dtype=np.int64)  # DECIMAL(15,2) 1.00 .. 50.00
    p.load("td", "d DECIMAL(15,2)", [p.d])
    p.f = r.integers(-4000, 4001, size=3001, dtype=np.int64).astype(np.float64) * 0.25  # exact in any order
    p.load("tf", "f DOUBLE", [p.f])
    yield p
    p.close()


def dec(v):
    return f"{v // 100}.{v % 100:02d}"


def test_cells_of_every_width_and_kind(pt):
    x, y, z, w = pt.cols
    # HUGEINT SUM (16 bytes), DOUBLE AVG, INTEGER MIN / MAX (4 bytes), BIGINT COUNT
    sel = [int(a) for a in w if a > 10]
    got = row(pt, "SELECT SUM(z), AVG(w), MIN(w), MAX(w), COUNT(w) FROM t WHERE w > 10")
    zs = [int(a) for a, b in zip(z, w) if b > 10]
    assert got[0] == str(sum(zs)) and got[2:] == [str(min(sel)), str(max(sel)), str(len(sel))], got
    assert abs(float(got[1]) - sum(sel) / len(sel)) <= 2.0**-51 * abs(sum(sel) / len(sel))
    assert row(pt, "SELECT MIN(w) FROM t") == [str(int(w.min()))]
    # DECIMAL SUM (16 bytes, scale kept) and AVG
    d = [int(a) for a in pt.d if a > 2500]
    got = row(pt, "SELECT SUM(d), AVG(d), MIN(d), COUNT(*) FROM td WHERE d > 25.00")
    assert got[0] == dec(sum(d)) and got[2] == dec(min(d)) and got[3] == str(len(d)), got
    assert abs(float(got[1]) - sum(d) / (len(d) * 100)) <= 2.0**-51 * (sum(d) / (len(d) * 100))
    # no passing row: SUM, MIN and AVG are NULL, the validity bit clear, beside COUNT 0
    for where in ("w > 1000", "w = 1000", "x = 0 AND w > 0"):
        assert row(pt, f"SELECT SUM(w), MIN(w), AVG(w), COUNT(w), COUNT(*) FROM t WHERE {where}") == [None, None, None, "0", "0"]
    assert row(pt, "SELECT SUM(d), AVG(d), COUNT(*) FROM td WHERE d > 99.00") == [None, None, "0"]
    assert row(pt, "SELECT MIN(f), AVG(f), COUNT(*) FROM tf WHERE f > 5000.0") == [None, None, "0"]


def test_global_reduce_sites(pt):
    """aggregates over an expression and over a DOUBLE column"""
    x, y, z, w = pt.cols
    sel = [(int(a), int(b)) for a, b in zip(x, y) if a > 24]
    got = row(pt, "SELECT SUM(x + y), MAX(x * 2), MIN(y - x), COUNT(*) FROM t WHERE x > 24")
    assert got == [str(sum(a + b for a, b in sel)), str(max(a * 2 for a, b in sel)), str(min(b - a for a, b in sel)),
                   str(len(sel))], got
    f = [float(a) for a in pt.f if a > 3.0]
    got = row(pt, "SELECT SUM(f), AVG(f), MIN(f), MAX(f), COUNT(f) FROM tf WHERE f > 3.0")
    assert [float(got[0]), float(got[2]), float(got[3])] == [sum(f), min(f), max(f)] and got[4] == str(len(f)), got
    assert abs(float(got[1]) - sum(f) / len(f)) <= 2.0**-51 * abs(sum(f) / len(f)), got


def test_column_count_boundary(pt):
    """15 aggregates are 31 pieces of one copy, 16 are 33: the first takes the tail, the second the DMAs"""
    aggs, want = [], []
    for col, v in zip("xyzw", pt.cols):
        sel = v[pt.cols[3] > 0].astype(np.int64)
        aggs += [f"SUM({col})", f"MIN({col})", f"MAX({col})", f"COUNT({col})"]
        want += [str(int(sel.sum())), str(int(sel.min())), str(int(sel.max())), str(len(sel))]
    for k, tail in ((15, True), (16, False)):
        assert row(pt, "SELECT " + ", ".join(aggs[:k]) + " FROM t WHERE w > 0", tail=tail) == want[:k], k


def test_join_aggregate(mbx):
    """a global aggregate over an inner join, fused into the probe and over the materialised pairs"""
    a = [(i % 7, i) for i in range(200)]
    b = [(i % 9, 1000 + i) for i in range(90)]
    pairs = [(v, w) for k, v in a for kk, w in b if k == kk]
    want = [str(len(pairs)), str(sum(v + w for v, w in pairs)), str(min(w for _, w in pairs)), str(max(v for v, _ in pairs))]
    for join_agg in ("true", "false"):
        p = Pair(mbx, mbx_join_agg=join_agg)
        p.load("ja", "k BIGINT, v BIGINT", [np.array([r[i] for r in a], dtype=np.int64) for i in range(2)])
        p.load("jb", "k BIGINT, w BIGINT", [np.array([r[i] for r in b], dtype=np.int64) for i in range(2)])
        assert row(p, "SELECT COUNT(*), SUM(ja.v + jb.w), MIN(jb.w), MAX(ja.v) FROM ja JOIN jb ON ja.k = jb.k") == want
        assert row(p, "SELECT COUNT(*), SUM(ja.v) FROM ja JOIN jb ON ja.k = jb.k WHERE ja.v < 0") == ["0", None]
        p.close()


def test_statements_that_keep_the_copy(pt, mbx):
    x, y, z, w = pt.cols
    n, hi = len(x), int((x > 24).sum())
    sx = int(x.sum())
    assert row(pt, "SELECT COUNT(*) FROM t WHERE x > 24 HAVING COUNT(*) > 0", tail=False) == [str(hi)]
    assert both(pt, "SELECT COUNT(*) FROM t WHERE x > 24 HAVING COUNT(*) < 0", tail=False) == []
    assert row(pt, "SELECT COUNT(*) AS c FROM t WHERE x > 24 ORDER BY c", tail=False) == [str(hi)]
    assert both(pt, "SELECT COUNT(*) FROM t WHERE x > 24 LIMIT 0", tail=False) == []
    assert row(pt, "SELECT COUNT(*) FROM t WHERE x > 24 LIMIT 1", tail=False) == [str(hi)]
    assert both(pt, "SELECT COUNT(*) FROM t WHERE x > 24 OFFSET 1", tail=False) == []
    assert both(pt, "SELECT COUNT(*) FROM t WHERE x > 24 UNION ALL SELECT COUNT(*) FROM t WHERE x <= 24",
                tail=False) == [[str(hi)], [str(n - hi)]]
    assert row(pt, "SELECT COUNT(*) + 1 FROM t WHERE x > 24", tail=False) == [str(hi + 1)]
    assert row(pt, "SELECT c + 1, s FROM (SELECT COUNT(*) AS c, SUM(x) AS s FROM t WHERE x > 24) q", tail=False) == [
        str(hi + 1), str(int(x[x > 24].sum()))]
    groups = both(pt, "SELECT x, COUNT(*) FROM t GROUP BY x", tail=False)
    assert sorted((int(a), int(b)) for a, b in groups) == sorted((int(k), int((x == k).sum())) for k in np.unique(x))
    assert row(pt, "SELECT w, COUNT(*), SUM(x) FROM t WHERE w = 7 GROUP BY w", tail=False) == [
        "7", str(int((w == 7).sum())), str(int(x[w == 7].sum()))]
    for c in pt:
        q(c, "CREATE TABLE r (c BIGINT)")
        _, t, _ = ran(c, lambda: q(c, "INSERT INTO r SELECT COUNT(*) FROM t WHERE x > 24"))
        assert t == 0
        _, t, _ = ran(c, lambda: q(c, "CREATE TABLE r2 AS SELECT COUNT(*) AS c, SUM(x) AS s FROM t"))
        assert t == 0
        a, t, _ = ran(c, lambda: c.query_arrow("SELECT COUNT(*), MAX(x) FROM t WHERE x > 24"))
        assert t == 0 and isinstance(a, mbx.Ok), a
        assert a.value.get_column_int64(0) == [hi] and a.value.get_column_int64(1) == [50]
    assert row(pt, "SELECT c FROM r", tail=False) == [str(hi)]
    assert row(pt, "SELECT c, s FROM r2", tail=False) == [str(n), str(sx)]
    pt.run("DROP TABLE r")
    pt.run("DROP TABLE r2")


def test_no_stale_buffer(pt):
    x = pt.cols[0]
    cnt = lambda k: str(int((x > k).sum()))
    tail = lambda k: row(pt, f"SELECT COUNT(*), SUM(x) FROM t WHERE x > {k}") == [cnt(k), str(int(x[x > k].sum()))]
    copy = lambda k: row(pt, f"SELECT COUNT(*) + 0, MAX(x) FROM t WHERE x > {k}", tail=False) == [cnt(k), "50"]
    assert tail(10) and copy(20) and tail(30)
    assert copy(35) and tail(40) and copy(45)
    for c in pt:  # a prepared statement executed with three values in a row
        st = c.prepare("SELECT COUNT(*), MIN(x) FROM t WHERE x > ?").value
        for k in (5, 48, 26):
            st.bind_bigint(1, k)
            res, t, h = ran(c, lambda: st.execute().value)
            assert res.rows == [[cnt(k), str(int(x[x > k].min()))]], (k, res.rows)
            assert (t, h) == ((1, 0) if c is pt.on else (0, 1)), (k, t, h)
        st.close()


def test_device_error_comes_back_and_clears(pt):
    """an out-of-range narrowing cast inside SUM: the same error with and without the tail, and the
    next statement on the connection answers"""
    msgs = []
    for c in pt:
        r = c.query("SELECT SUM(CAST(z AS INTEGER)), COUNT(*) FROM t")
        assert isinstance(r, pt.mbx.Err), r
        msgs.append(r.error.message)
    assert msgs[0] == msgs[1] and "out of range" in msgs[0].lower(), msgs
    assert row(pt, "SELECT COUNT(*) FROM t WHERE x > 24") == [str(int((pt.cols[0] > 24).sum()))]
    assert row(pt, "SELECT SUM(CAST(w AS SMALLINT)) FROM t") == [str(int(pt.cols[3].sum()))]


def test_shards_see_their_partials(mbx, oracle):
    """two shards on one device, combined on the host: the global answer and both shards' partials"""
    n = 8193
    x = oracle.synth_i64(n, 42, 0, 50, 1).astype(np.int64)
    p = Pair(mbx, gpu_devices="0,0", mbx_combine="host")
    one = Pair(mbx)
    for pr in (p, one):
        pr.run(f"CREATE TABLE t AS SELECT mbx_synth(42, i, 50) + 1 AS x FROM range({n}) tbl(i)")
    parts = [x[n * i // 2:n * (i + 1) // 2] for i in range(2)]
    for where, k in (("x > 24", 24), ("x > 49", 49)):
        sql = f"SELECT COUNT(*), SUM(x) FROM t WHERE {where}"
        want = row(one, sql)
        assert want == [str(int((x > k).sum())), str(int(x[x > k].sum()))]
        for c in p:
            assert rows_of(c, sql) == [want], where
            for i, part in enumerate(parts):
                sp = c.shard_partial(i)
                assert sp.value(0, 0) == str(int((part > k).sum())), (where, i, sp.cells())
                assert sp.value(1, 0) == str(int(part[part > k].sum())), (where, i, sp.cells())
                sp.close()
    p.close()
    one.close()
