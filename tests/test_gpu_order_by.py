"""ORDER BY on the device (SortRel: sort_key / sort_key_str / sort_key_null
kernels, hipCUB radix passes, then GatherRel) against sort_model.py.

Every query is SELECT id, <payload> FROM t ORDER BY <keys>, id.  The returned
id column must equal the model's order exactly, and every payload cell must be
the cell of the source row that id names, NULL flag included.  Nothing is
compared with a tolerance: integers and decimals as text, floats by bit
pattern (any NaN matches NaN), strings as text.

Sizes.  SortPairs runs hipcub::DeviceRadixSort::SortPairs, which rocPRIM
dispatches by size (rocprim/device/device_radix_sort.hpp): up to
block_size x items_per_thread = min(256, ..) x min(4, ..) = 1024 items one
single-block sort; above that and up to radix_sort_config<>::merge_sort_limit
= 1024 * 1024 = 1,048,576 items (device_radix_sort_config.hpp) a block sort
followed by merges; above that Onesweep.  The multi-key scheme (least
significant key first) needs every one of them to be stable, the 1-bit NULL
pass (end_bit = 1) included, so test_sizes crosses both boundaries with keys
full of ties."""
import math

import numpy as np
import pytest

import sort_model as M
import vm_cases as V
import vm_reference as R
from conftest import q
from gpu_tables import check_cell, fill, load, profiled, retable

pytestmark = pytest.mark.gpu

ORDERINGS = [("", False, None), (" NULLS FIRST", False, True), (" NULLS LAST", False, False),
             (" DESC", True, None), (" DESC NULLS FIRST", True, True), (" DESC NULLS LAST", True, False)]


def check_sorted(conn, sql, want, payload):
    """the result's id column (column 0) is `want`; column 1 + j holds payload[j] of the row id names"""
    res = conn.query_raw(sql)
    assert res.row_count() == len(want), (sql, res.row_count(), len(want))
    text, nulls = res.cells()
    got = [int(r[0]) for r in text]
    if got != want:
        k = next(i for i in range(len(want)) if got[i] != want[i])
        raise AssertionError(f"{sql}: order differs from row {k}: got ids {got[k:k + 8]}, want {want[k:k + 8]}; "
                             + "; ".join(f"{c.name}: got {[c.get(i) for i in got[k:k + 8]]}, want "
                                         f"{[c.get(i) for i in want[k:k + 8]]}" for c in payload))
    assert not any(x[0] for x in nulls), sql
    for j, c in enumerate(payload, 1):
        for k, r in enumerate(got):
            v = c.get(r)
            assert nulls[k][j] == (v is None), (sql, c.name, k, r)
            if v is not None:
                check_cell(c, v, text[k][j], lambda: res.raw(j, k), (sql, c.name, k, r))
    res.close()


class Db:
    def __init__(self, mbx):
        self.mbx, self.c, self.t = mbx, profiled(mbx), {}

    def table(self, name, make):
        if name not in self.t:
            self.t[name] = make(self.c, name)
        return self.t[name]


@pytest.fixture(scope="module")
def db(mbx):
    d = Db(mbx)
    yield d
    d.c.close()


# ---- 1. every key type, alone ----------------------------------------------------------------
def _dates():
    ti = V.TABLES["ti"]
    cols = [V.Col("id", "BIGINT", range(V.N))]
    for src, name, t, span in (("ia", "dt", "DATE", 100000), ("ian", "dtn", "DATE", 100000),
                               ("ba", "ts", "TIMESTAMP", 4 * 10 ** 16), ("ban", "tsn", "TIMESTAMP", 4 * 10 ** 16)):
        c = ti.cols[src]
        cols.append(V.Col(name, t, [v % (2 * span) - span for v in c.values], c.valid))  # both sides of 1970
    return V.Table("tdt", cols)


KEY_COLUMNS = {  # type -> (table, its columns of that type)
    "TINYINT": ("ti", ["ta", "tan"]), "SMALLINT": ("ti", ["sa", "san"]), "INTEGER": ("ti", ["ia", "ian"]),
    "BIGINT": ("ti", ["ba", "ban"]), "UTINYINT": ("tu", ["uta", "utan"]), "USMALLINT": ("tu", ["usa", "usan"]),
    "UINTEGER": ("tu", ["uia", "uian"]), "UBIGINT": ("tu", ["ula", "ulan"]), "BOOLEAN": ("tl", ["pn", "qn"]),
    "DECIMAL(9,2)": ("td", ["da", "dan"]), "DECIMAL(18,1)": ("td", ["ea", "ean"]), "DECIMAL(18,18)": ("td", ["va"]),
    "DOUBLE": ("tf", ["fc", "fcn"]), "FLOAT": ("tf", ["ra", "ran"]), "DATE": ("tdt", ["dt", "dtn"]),
    "TIMESTAMP": ("tdt", ["ts", "tsn"]), "UBIGINT/2^63": ("tub", ["ub", "ubn"]),
}
UB = [2 ** 63, 2 ** 63 - 1, 2 ** 63 + 1, 0, 2 ** 64 - 1, 1, 2 ** 62, 2 ** 63 + 2 ** 62]  # either side of the sign bit
_ub = [UB[(r * 3 + r // 8) % len(UB)] for r in range(V.N)]
_TABLES = dict(V.TABLES, tdt=_dates(), tub=V.Table("tub", [V.Col("id", "BIGINT", range(V.N)), V.Col("ub", "UBIGINT", _ub),
                                                          V.Col("ubn", "UBIGINT", _ub, V.null_mask(5))]))


def _key_table(db, tname):
    t = _TABLES[tname]
    cols = ["id"] + sorted({c for tn, cs in KEY_COLUMNS.values() if tn == tname for c in cs})

    def make(conn, name):
        load(db.mbx, conn, t, name, list(range(V.N)), cols)
        return t
    return db.table(tname, make)


def test_the_edge_values_are_keys():
    c = V.TABLES["tu"].cols["ula"].values
    assert 2 ** 64 - 1 in c and 2 ** 64 - 2 in c and {2 ** 63, 2 ** 63 - 1} <= set(_ub)
    fc = V.TABLES["tf"].cols["fc"]
    bits = {R.bits(v) for v in fc.values}
    assert {R.bits(0.0), R.bits(-0.0), R.bits(math.inf), R.bits(-math.inf), 0xFFF8000000000001, 1} <= bits
    assert sum(v != v for v in fc.values) >= 2
    assert V.TABLES["ti"].cols["ba"].values.count(R.INT_RANGE["BIGINT"][0]) > 0


@pytest.mark.parametrize("sqltype", list(KEY_COLUMNS))
def test_single_key(db, sqltype):
    tname, names = KEY_COLUMNS[sqltype]
    t = _key_table(db, tname)
    ident = M.key_of(t.cols["id"])
    for name in names:
        c = t.cols[name]
        assert c.sqltype == sqltype.split("/")[0]
        payload = [c]  # (a DATE / TIMESTAMP cell is compared as its stored number, not its spelling)
        for suffix, desc, nf in ORDERINGS:
            want = M.order(V.N, [M.key_of(c, desc, nf), ident])
            check_sorted(db.c, f"SELECT id, {name} FROM {tname} ORDER BY {name}{suffix}, id", want, payload)


# ---- 2. keys SortRel does not take; the same columns as payload ---------------------------------
def _wide(db):
    def make(conn, name):
        th, td = V.TABLES["th"], V.TABLES["td"]
        load(db.mbx, conn, th, "wh", list(range(V.N)), ["id", "ha", "han"])
        load(db.mbx, conn, td, "wd", list(range(V.N)), ["id", "ga", "gan"])
        q(conn, "CREATE TABLE wv (id BIGINT, iv INTERVAL, ivn INTERVAL)")
        days = [r * 7 % 40 + 2 for r in range(V.N)]
        ok = V.null_mask(3)
        for lo in range(0, V.N, 125):  # (INSERT ... VALUES: the appenders do not take INTERVAL columns)
            q(conn, "INSERT INTO wv VALUES " + ", ".join(
                f"({r}, INTERVAL {days[r]} day, " + (f"INTERVAL {days[r]} day" if ok[r] else "NULL") + ")"
                for r in range(lo, lo + 125)))
        text = [f"{d} days" for d in days]
        return {"wh": th, "wd": td, "wv": V.Table("wv", [V.Col("id", "BIGINT", range(V.N)), V.Col("iv", "INTERVAL", text),
                                                        V.Col("ivn", "INTERVAL", text, ok)])}
    return db.table("wide", make)


@pytest.mark.parametrize("tname,names", [("wh", ["ha", "han"]), ("wd", ["ga", "gan"]), ("wv", ["iv", "ivn"])])
def test_unsupported_keys_and_their_gather(db, tname, names):
    t = _wide(db)[tname]
    for name in names:
        for suffix in ("", " DESC NULLS FIRST"):
            r = db.c.query(f"SELECT id, {name} FROM {tname} ORDER BY {name}{suffix}, id")
            assert isinstance(r, db.mbx.Err), (name, suffix, "rows returned")
            assert r.error.message.startswith("Not implemented Error"), r.error.message
    # as payload: gather_fixed_kernel's 16-byte loads and stores, with validity
    want = list(range(V.N - 1, -1, -1))
    check_sorted(db.c, f"SELECT id, {', '.join(names)} FROM {tname} ORDER BY id DESC", want, [t.cols[k] for k in names])


# ---- 3. VARCHAR keys ---------------------------------------------------------------------------
P8, P16 = "prefix8_", "sixteen_byte_pre"
STR_EDGES = ["", None, "abcdefg", P8, P8 + "9", "fifteen_bytes_1", P16, P16 + "x", P8 + "a", P8 + "b", P16 + "a", P16 + "b",
             "é", "aé", "a\x7f", "a", "€uro", "😀", "z" * 200, P8[:7], P16[:15], "\x7f", "Zebra", "zebra"]
assert len(P8) == 8 and len(P16) == 16
assert sorted({len(s.encode()) for s in STR_EDGES if s is not None} & {0, 7, 8, 9, 15, 16, 17, 200}) == [0, 7, 8, 9, 15, 16, 17, 200]
WORDS = ["", "a", "ab", "abc", P8, P8 + "tail", P16, P16 + "tail", "é", "éa", "z", "Z", "mid", "mi", "m"]


def str_row(i):
    """row i of the string tables: the edge list first, then generated rows; one row in seven NULL"""
    if i < len(STR_EDGES):
        return STR_EDGES[i]
    if i % 7 == 3:
        return None
    return WORDS[(i * 7 + i // 13) % len(WORDS)] + ("" if i % 3 else str(i % 11))


def _str_table(db, n):
    def make(conn, name):
        s = [str_row(i) for i in range(n)]
        x = [(i * 37) % 50 for i in range(n)]
        fill(conn, name, "id BIGINT, s VARCHAR, x BIGINT", [(i, s[i], x[i]) for i in range(n)])
        return V.Table(name, [V.Col("id", "BIGINT", range(n)), V.Col("s", "VARCHAR", ["" if v is None else v for v in s],
                                                                     [v is not None for v in s]), V.Col("x", "BIGINT", x)])
    return db.table(f"s{n}", make)


@pytest.mark.parametrize("n", [1, 2, 257, 4097])
def test_varchar_key(db, n):
    t = _str_table(db, n)
    if n >= 257:
        assert max(len(v.encode()) for v in t.cols["s"].values) == 200  # 25 chunk passes
    ident = M.key_of(t.cols["id"])
    for suffix, desc, nf in ORDERINGS[1:3] + ORDERINGS[4:]:
        want = M.order(n, [M.key_of(t.cols["s"], desc, nf), ident])
        check_sorted(db.c, f"SELECT id, s, x FROM s{n} ORDER BY s{suffix}, id", want, [t.cols["s"], t.cols["x"]])


# ---- 4. several keys ---------------------------------------------------------------------------
MK_N = 1537
NAN2 = R.from_bits(0xFFF8000000000001)
MK_D = [0.0, -0.0, math.nan, NAN2, 1.5, -1.5, math.inf, -0.0, 0.0]


def _multi(db):
    def make(conn, name):
        n = MK_N
        tn = [(i * 5) % 3 - 1 for i in range(n)]
        tn_ok = [i % 5 != 1 for i in range(n)]
        s = [["", "k", "ka", P8 + "x", P8 + "y"][(i // 3) % 5] for i in range(n)]
        s_ok = [i % 11 != 4 for i in range(n)]
        d = [MK_D[(i * 7 + i // 9) % len(MK_D)] for i in range(n)]
        u = [(i * 13) % 4 for i in range(n)]
        u_ok = [i % 6 != 2 for i in range(n)]
        b = [i % 4 < 2 for i in range(n)]
        fill(conn, "mk0", "id BIGINT, tn BIGINT, s VARCHAR, d DOUBLE, u BIGINT, b BIGINT",
             [(i, tn[i] if tn_ok[i] else None, s[i] if s_ok[i] else None, d[i], u[i] if u_ok[i] else None, int(b[i]))
              for i in range(n)])
        q(conn, "CREATE TABLE mk AS SELECT id, CAST(tn AS TINYINT) AS tn, s, d, CAST(u AS UBIGINT) AS u, "
                "b = 1 AS b FROM mk0")
        return V.Table("mk", [V.Col("id", "BIGINT", range(n)), V.Col("tn", "TINYINT", tn, tn_ok), V.Col("s", "VARCHAR", s, s_ok),
                              V.Col("d", "DOUBLE", d), V.Col("u", "UBIGINT", u, u_ok),
                              V.Col("b", "BOOLEAN", b)])
    return db.table("mk", make)


MULTI = [
    [("tn", " DESC NULLS FIRST", True, True), ("s", "", False, None), ("d", " DESC", True, None), ("u", "", False, None)],
    [("b", "", False, None), ("s", " DESC NULLS LAST", True, False), ("d", "", False, None)],
    [("d", "", False, None), ("s", " NULLS FIRST", False, True), ("tn", "", False, None)],
    [("u", " NULLS FIRST", False, True), ("tn", " DESC", True, None), ("s", " DESC NULLS FIRST", True, True), ("d", " DESC", True, None)],
    [("b", " DESC", True, None), ("tn", " NULLS FIRST", False, True), ("u", " DESC NULLS LAST", True, False)],
]


@pytest.mark.parametrize("keys", MULTI, ids=lambda k: "-".join(x[0] for x in k))
def test_multi_key(db, keys):
    t = _multi(db)
    model = [M.key_of(t.cols[name], desc, nf) for name, _, desc, nf in keys] + [M.key_of(t.cols["id"])]
    want = M.order(MK_N, model)
    # the leading keys are low-cardinality: the later ones and id decide most positions
    assert len({(t.cols[keys[0][0]].get(r)) for r in range(MK_N)}) <= 6
    sql = "SELECT id, tn, s, d, u, b FROM mk ORDER BY " + ", ".join(name + sfx for name, sfx, _, _ in keys) + ", id"
    check_sorted(db.c, sql, want, [t.cols[k] for k in ("tn", "s", "d", "u", "b")])


# ---- 5. the sizes that reach each hipCUB algorithm -----------------------------------------------
def _i64(buf, n):
    assert len(buf) >= 4 + 8 * n and int.from_bytes(buf[:4], "little") == n, (len(buf), n)
    return np.frombuffer(buf, dtype="<i8", count=n, offset=4)


@pytest.mark.parametrize("n", [1, 2, 255, 1024, 1025, 70001, 1048576, 1048577, 1200003])
def test_sizes(mbx, n):
    g = np.random.default_rng(n)
    k = g.integers(-3, 4, size=n).astype(np.int64)  # seven values: ties everywhere
    j = g.integers(-2, 3, size=n).astype(np.int32)
    j_ok = g.integers(0, 5, size=n) != 0
    j[~j_ok] = 2 ** 31 - 1  # poison under the NULLs
    ident = np.arange(n, dtype=np.int64)
    conn = profiled(mbx)
    q(conn, "CREATE TABLE z (id BIGINT, k BIGINT, j INTEGER)")
    ap = conn.create_appender("main", "z").value
    for col, (a, ok) in enumerate(((ident, None), (k, None), (j, None if j_ok.all() else j_ok.astype(np.uint8)))):
        r = ap.append_column(col, a, ok)
        assert isinstance(r, mbx.Ok), r.error.message
    assert isinstance(ap.commit(n), mbx.Ok)
    ap.close()
    valid = None if j_ok.all() else j_ok
    for order, kd, jd, jnf in (("k, j, id", False, False, None), ("k DESC, j DESC NULLS FIRST, id", True, True, True)):
        want = np.array(M.order_np(n, [(k, None, "int", kd, None), (j, valid, "int", jd, jnf), (ident, None, "int", False, None)]))
        a = conn.query_arrow(f"SELECT id, k, CAST(j AS BIGINT) AS j FROM z ORDER BY {order}").value
        assert a.row_count() == n
        got = _i64(a._buf("int64", 0), n)
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, (n, order, int(bad[0]), got[bad[0]:bad[0] + 8], want[bad[0]:bad[0] + 8])
        assert np.array_equal(_i64(a._buf("int64", 1), n), k[want]), (n, order, "k")
        jb = a._buf("int64", 2, True)
        jv = np.frombuffer(jb, dtype=np.uint8, count=n, offset=4 + 8 * n) != 0
        assert np.array_equal(jv, j_ok[want]), (n, order, "j validity")
        assert np.array_equal(_i64(jb, n)[jv], j[want][jv].astype(np.int64)), (n, order, "j")
        a.close()
        if n > 1:
            assert "radix_sort" in [x["name"] for x in conn.last_profile()["kernels"]]
    conn.close()


# ---- 6. a sort over something other than a base table ---------------------------------------------
def test_sort_of_a_filtered_subquery(db):
    t = _str_table(db, 4097)
    s, x = t.cols["s"], t.cols["x"]
    rows = [r for r in range(4097) if x.values[r] < 25]
    want = M.order(rows, [M.key_of(s, True, None), M.key_of(x), M.key_of(t.cols["id"])])
    check_sorted(db.c, "SELECT id, s, x FROM (SELECT id, s, x FROM s4097 WHERE x < 25) u ORDER BY s DESC, x, id", want, [s, x])


def test_sort_of_a_group_by_result(db):
    n = 4097
    g = [(i * 7) % 1201 for i in range(n)]
    g_ok = [i % 9 != 5 for i in range(n)]
    x = [(i * 37) % 50 for i in range(n)]
    t = V.Table("gb", [V.Col("id", "BIGINT", range(n)), V.Col("g", "INTEGER", g, g_ok), V.Col("x", "BIGINT", x)])
    load(db.mbx, db.c, t, "gb", list(range(n)), ["id", "g", "x"])
    groups = {}
    for i in range(n):
        c, sm = groups.get(g[i] if g_ok[i] else None, (0, 0))
        groups[g[i] if g_ok[i] else None] = (c + 1, sm + x[i])
    keys = list(groups)
    assert None in keys and len(keys) > 1024
    cnt = V.Col("c", "BIGINT", [groups[k][0] for k in keys])
    sm = V.Col("s", "HUGEINT", [groups[k][1] for k in keys])
    gk = V.Col("g", "INTEGER", [0 if k is None else k for k in keys], [k is not None for k in keys])
    want = M.order(len(keys), [M.key_of(cnt, True, None), M.key_of(gk, False, True)])  # g is unique: the NULL group once
    res = db.c.query_raw("SELECT g, COUNT(*) AS c, SUM(x) AS s FROM gb GROUP BY g ORDER BY c DESC, g NULLS FIRST")
    text, nulls = res.cells()
    assert res.row_count() == len(keys)
    got = [(None if nulls[k][0] else int(text[k][0]), int(text[k][1]), int(text[k][2])) for k in range(len(keys))]
    assert got == [(keys[r],) + groups[keys[r]] for r in want], [(a, b) for a, b in zip(got, want) if a[0] != keys[b]][:5]
    assert not any(x_[1] or x_[2] for x_ in nulls)
    res.close()


def test_sort_of_a_union(db):
    t = _str_table(db, 4097)
    s, x = t.cols["s"], t.cols["x"]
    a = [r for r in range(4097) if x.values[r] < 10]
    b = [r for r in range(4097) if x.values[r] >= 37]
    rows = a + b
    u = retable(t, rows, ["s", "x"], "u")
    uid = V.Col("id", "BIGINT", [r if k < len(a) else r + 100000 for k, r in enumerate(rows)])
    pos = {v: k for k, v in enumerate(uid.values)}
    order = M.order(len(rows), [M.key_of(u.cols["s"], False, True), M.key_of(u.cols["x"], True, None), M.key_of(uid)])
    res = db.c.query_raw("SELECT id, s, x FROM s4097 WHERE x < 10 UNION ALL SELECT id + 100000, s, x FROM s4097 WHERE x >= 37 "
                         "ORDER BY s NULLS FIRST, x DESC, id")
    text, nulls = res.cells()
    assert res.row_count() == len(rows)
    got = [pos[int(r[0])] for r in text]
    assert got == order, next((k, got[k:k + 5], order[k:k + 5]) for k in range(len(rows)) if got[k] != order[k])
    for k, r in enumerate(got):
        assert nulls[k][1] == (u.cols["s"].get(r) is None) and (nulls[k][1] or text[k][1] == u.cols["s"].get(r)), (k, r)
        assert text[k][2] == str(u.cols["x"].get(r)), (k, r)
    res.close()
