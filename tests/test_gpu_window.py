"""Window functions on the device (window.cpp, window_kernels.hip) against
window_model.py.

Every statement has no ORDER BY of its own, so its rows come back in source
order and row r of the result is compared with the model's value for source
row r.  Integers, HUGEINTs and DECIMALs compare as the text the library prints;
DOUBLE results that are exact by construction (sums of integer-valued doubles
below 2^40, AVG of small integers: one correctly rounded division) compare by
value bit for bit through the shortest round-trip text; DOUBLE sums of
arbitrary values within 1e-9 * sum|x|.

T is the scan's tile in rows (window_plan.h: kWinTile = 256 lanes x 4 rows),
LANES the lanes of the one workgroup that scans the tiles' carries.  SIZES
crosses the wave (63, 64, 65), the tile (T - 1, T, T + 1), two tiles and a
bit, and BIG has more tiles than the carry workgroup has lanes, so its loop
runs twice."""
import math
import struct

import numpy as np
import pytest

import vm_cases as V
import window_model as W
from conftest import q
from gpu_tables import fill, kernels, load, profiled

pytestmark = pytest.mark.gpu

T = 1024
LANES = 256
MULTI = 2 * T + 1
BIG = LANES * T + T + 1  # 258 tiles
SIZES = [1, 2, 63, 64, 65, T - 1, T, T + 1, MULTI, BIG]


@pytest.fixture(scope="module")
def conn(mbx):
    c = profiled(mbx)
    yield c
    c.close()


_names = iter(range(10 ** 6))


def table(conn, n, exprs):
    """CREATE TABLE .. AS SELECT <exprs over i> FROM range(n) tbl(i); returns its name"""
    name = f"w{next(_names)}"
    q(conn, f"CREATE TABLE {name} AS SELECT i AS id, {exprs} FROM range({n}) tbl(i)")
    return name


def cells(conn, sql):
    res = conn.query_raw(sql)
    try:
        text, nulls = res.cells()
    finally:
        res.close()
    return text, nulls


def check(conn, sql, want, how=None):
    """column j of the result is want[j] row by row; how[j]: "text" (str of the
    value), "f64" (the exact double), ("dec", scale), "tol" ((value, abs_sum)
    within 1e-9 * abs_sum), "set" (a set of acceptable double bit patterns)"""
    text, nulls = cells(conn, sql)
    n = len(want[0])
    assert len(text) == n, (sql, len(text), n)
    how = how or ["text"] * len(want)
    for j, (col, h) in enumerate(zip(want, how)):
        got = [None if nulls[r][j] else text[r][j] for r in range(n)]
        if h == "text":
            exp = [None if v is None else str(v) for v in col]
        elif h == "f64":
            got = [None if g is None else struct.pack("<d", float(g)) for g in got]
            exp = [None if v is None else struct.pack("<d", float(v)) for v in col]
        elif isinstance(h, tuple):
            exp = [None if v is None else V.dec_text(v, h[1]) for v in col]
        else:
            exp = None
        if exp is not None:
            if got != exp:
                r = next(i for i in range(n) if got[i] != exp[i])
                raise AssertionError(f"{sql}: column {j} differs first at row {r}: got {got[r:r + 6]}, want {exp[r:r + 6]}")
            continue
        for r in range(n):
            v = col[r]
            assert (got[r] is None) == (v is None), (sql, j, r, got[r], v)
            if v is None:
                continue
            g = float(got[r])
            if h == "tol":
                val, abs_sum = v
                assert abs(g - val) <= 1e-9 * abs_sum, (sql, j, r, g, val, abs_sum)
            else:
                bits = struct.unpack("<Q", struct.pack("<d", g))[0]
                assert ("nan" in v and g != g) or bits in v, (sql, j, r, g, v)


def all_calls(spec_sql, v_sql, vals, ordered):
    """the select items and the model calls of every function, running and whole-partition"""
    items, calls, how = [], [], []
    for f in ("row_number", "rank", "dense_rank"):
        items.append(f"{f}() OVER ({spec_sql})")
        calls.append(W.Call(f))
        how.append("text")
    default = "range" if ordered else "part"
    for frame_sql, frame in (("", default), (" ROWS BETWEEN UNBOUNDED PRECEDING AND CURRENT ROW", "rows"),
                             (" ROWS BETWEEN UNBOUNDED PRECEDING AND UNBOUNDED FOLLOWING", "part")):
        items.append(f"count(*) OVER ({spec_sql}{frame_sql})")
        calls.append(W.Call("count_star", frame=frame))
        how.append("text")
        for f in ("count", "sum", "min", "max", "avg"):
            items.append(f"{f}({v_sql}) OVER ({spec_sql}{frame_sql})")
            calls.append(W.Call(f, vals, "int", frame))
            how.append("f64" if f == "avg" else "text")
    return items, calls, how


# ---- 1. every function at every size -------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
def test_sizes(conn, n):
    t = table(conn, n, "(i * 7919) % 13 AS k, (i * 104729) % 1000 - 500 AS v, "
                       "CASE WHEN i % 7 = 3 THEN NULL ELSE (i * 31) % 97 END AS o")
    k = [(i * 7919) % 13 for i in range(n)]
    v = [(i * 104729) % 1000 - 500 for i in range(n)]
    o = [None if i % 7 == 3 else (i * 31) % 97 for i in range(n)]
    ok = [x is not None for x in o]
    items, calls, how = all_calls("PARTITION BY k ORDER BY o", "v", v, True)
    want = W.window(n, [(k, None, "int")], [(o, ok, "int", False, None)], calls)
    check(conn, f"SELECT {', '.join(items)} FROM {t}", want, how)
    names = kernels(conn)
    assert names.count("window_bounds") == 1 and ("radix_sort" in names) == (n > 1)
    for nm in ("window_scan_reduce", "window_scan_carry", "window_scan_apply", "window_emit"):
        assert nm in names, names


# ---- 2. partition shapes at the multi-tile size -----------------------------------------------
def _shape(name, n):
    if name == "one":
        return [0] * n
    if name == "each":
        return list(range(n))
    if name == "tile":
        return [i // T for i in range(n)]
    if name == "tile+1":
        return [i // (T + 1) for i in range(n)]
    # skewed: one partition of half the rows among thousands of small ones
    return [0 if i % 2 == 0 else 1 + i // 6 for i in range(n)]


SHAPE_SQL = {"one": "0", "each": "i", "tile": f"i // {T}", "tile+1": f"i // {T + 1}",
             "skew": "CASE WHEN i % 2 = 0 THEN 0 ELSE 1 + i // 6 END"}


@pytest.mark.parametrize("shape", ["one", "each", "tile", "tile+1", "skew"])
def test_partition_shapes(conn, shape):
    n = 12 * T + 5 if shape == "skew" else 5 * T + 7  # several tiles; thousands of partitions for the skew
    t = table(conn, n, f"{SHAPE_SQL[shape]} AS k, (i * 104729) % 1000 - 500 AS v")
    k = _shape(shape, n)
    v = [(i * 104729) % 1000 - 500 for i in range(n)]
    idv = list(range(n))
    # data already in key order: ORDER BY id keeps every boundary where the layout puts it
    items, calls, how = all_calls("PARTITION BY k ORDER BY id", "v", v, True)
    want = W.window(n, [(k, None, "int")], [(idv, None, "int", False, None)], calls)
    check(conn, f"SELECT {', '.join(items)} FROM {t}", want, how)


def test_one_partition_carries_across_the_carry_loop(conn):
    # one partition over BIG rows: the carry crosses every tile and both rounds of the carry workgroup
    n = BIG
    t = table(conn, n, "(i * 104729) % 1000 - 500 AS v")
    v = [(i * 104729) % 1000 - 500 for i in range(n)]
    calls = [W.Call("sum", v, "int", "rows"), W.Call("min", v, "int", "rows"), W.Call("count_star", frame="part"),
             W.Call("row_number")]
    want = W.window(n, [], [(list(range(n)), None, "int", True, None)], calls)
    check(conn, f"SELECT sum(v) OVER (ORDER BY id DESC ROWS UNBOUNDED PRECEDING), min(v) OVER (ORDER BY id DESC ROWS "
                f"UNBOUNDED PRECEDING), count(*) OVER (), row_number() OVER (ORDER BY id DESC) FROM {t}", want)


@pytest.mark.parametrize("n", [MULTI, 5 * T + 7])
def test_peer_group_straddles_a_tile_edge(conn, n):
    # peers of 100 rows in key order: groups cross every tile edge (1024 is no multiple of 100),
    # and under the RANGE default a row reads its value from the next tile
    t = table(conn, n, "i // 100 AS o, i % 11 - 5 AS v")
    o = [i // 100 for i in range(n)]
    v = [i % 11 - 5 for i in range(n)]
    calls = [W.Call("sum", v, "int", "range"), W.Call("count", v, "int", "range"), W.Call("rank"),
             W.Call("dense_rank"), W.Call("max", v, "int", "range")]
    want = W.window(n, [], [(o, None, "int", False, None)], calls)
    check(conn, f"SELECT sum(v) OVER (ORDER BY o), count(v) OVER (ORDER BY o RANGE UNBOUNDED PRECEDING), "
                f"rank() OVER (ORDER BY o), dense_rank() OVER (ORDER BY o), max(v) OVER (ORDER BY o) FROM {t}", want)


# ---- 3. int128 ----------------------------------------------------------------------------------
@pytest.mark.parametrize("run", [8, 3 * T + 5])
def test_running_sum_crosses_2_64_and_comes_back(conn, run):
    # runs of +2^62 and then of -2^62: the sum passes 2^64 (after 4 rows) and returns, inside a
    # tile (run 8) and across tiles (run 3T + 5)
    n = 4 * run + 3
    t = table(conn, n, f"CASE WHEN (i // {run}) % 2 = 0 THEN 4611686018427387904 ELSE -4611686018427387904 END AS v")
    v = [2 ** 62 if (i // run) % 2 == 0 else -2 ** 62 for i in range(n)]
    idv = list(range(n))
    calls = [W.Call("sum", v, "int", "rows"), W.Call("sum", v, "int", "part"), W.Call("avg", v, "int", "part")]
    want = W.window(n, [], [(idv, None, "int", False, None)], calls)
    assert max(x for x in want[0]) > 2 ** 64 or run < 4
    text, nulls = cells(conn, f"SELECT sum(v) OVER (ORDER BY id ROWS UNBOUNDED PRECEDING), sum(v) OVER (), avg(v) OVER () FROM {t}")
    assert [r[0] for r in text] == [str(x) for x in want[0]]
    assert [r[1] for r in text] == [str(x) for x in want[1]]
    # AVG divides the int128 sum, converted once, by the count
    assert float(text[0][2]) == float(want[1][0]) / n


def test_hugeint_and_wide_decimal_arguments(conn):
    n = MULTI
    t = table(conn, n, "i % 3 AS k, (i * 1000003 - 1000000)::HUGEINT * 18446744073709551616 AS h, "
                       "((i * 7 - 5000) * 1000000000000::HUGEINT * 1000000000000)::DECIMAL(38,2) AS d")
    k = [i % 3 for i in range(n)]
    h = [(i * 1000003 - 1000000) * 2 ** 64 for i in range(n)]
    d = [(i * 7 - 5000) * 10 ** 24 * 100 for i in range(n)]  # unscaled, scale 2
    idv = list(range(n))
    calls = [W.Call("sum", h, "int", "rows"), W.Call("min", h, "int", "rows"), W.Call("max", h, "int", "part"),
             W.Call("lag", h, offset=2), W.Call("sum", d, "int", "rows"), W.Call("min", d, "int", "part"),
             W.Call("max", d, "int", "rows"), W.Call("lead", d, offset=1)]
    want = W.window(n, [(k, None, "int")], [(idv, None, "int", True, None)], calls)
    spec = "PARTITION BY k ORDER BY id DESC"
    check(conn, f"SELECT sum(h) OVER ({spec} ROWS UNBOUNDED PRECEDING), min(h) OVER ({spec} ROWS UNBOUNDED PRECEDING), "
                f"max(h) OVER (PARTITION BY k), lag(h, 2) OVER ({spec}), sum(d) OVER ({spec} ROWS UNBOUNDED PRECEDING), "
                f"min(d) OVER (PARTITION BY k), max(d) OVER ({spec} ROWS UNBOUNDED PRECEDING), lead(d) OVER ({spec}) "
                f"FROM {t}", want, ["text"] * 4 + [("dec", 2)] * 4)


# ---- 4. NULLs ----------------------------------------------------------------------------------
def test_null_partition_keys_form_one_partition(conn):
    n = MULTI
    t = table(conn, n, "CASE WHEN i % 3 = 0 THEN NULL ELSE i % 4 END AS k, i % 10 AS v")
    k = [None if i % 3 == 0 else i % 4 for i in range(n)]
    v = [i % 10 for i in range(n)]
    calls = [W.Call("count_star", frame="part"), W.Call("sum", v, "int", "part"), W.Call("row_number")]
    want = W.window(n, [(k, [x is not None for x in k], "int")], [], calls)
    check(conn, f"SELECT count(*) OVER (PARTITION BY k), sum(v) OVER (PARTITION BY k), row_number() OVER (PARTITION BY k) FROM {t}", want)


@pytest.mark.parametrize("desc", [False, True])
@pytest.mark.parametrize("nulls_first", [None, True, False])
def test_null_order_keys(conn, desc, nulls_first):
    n = T + 65
    t = table(conn, n, "i % 2 AS k, CASE WHEN i % 5 = 1 THEN NULL ELSE (i * 17) % 23 END AS o, i AS v")
    k = [i % 2 for i in range(n)]
    o = [None if i % 5 == 1 else (i * 17) % 23 for i in range(n)]
    v = list(range(n))
    sql = "PARTITION BY k ORDER BY o" + (" DESC" if desc else "") + \
          ("" if nulls_first is None else " NULLS FIRST" if nulls_first else " NULLS LAST")
    calls = [W.Call("row_number"), W.Call("rank"), W.Call("dense_rank"), W.Call("sum", v, "int", "range"),
             W.Call("lag", v, offset=1)]
    want = W.window(n, [(k, None, "int")], [(o, [x is not None for x in o], "int", desc, nulls_first)], calls)
    check(conn, f"SELECT row_number() OVER ({sql}), rank() OVER ({sql}), dense_rank() OVER ({sql}), sum(v) OVER ({sql}), "
                f"lag(v) OVER ({sql}) FROM {t}", want)


def test_null_arguments_with_a_leading_null_stretch(conn):
    n = MULTI
    lead = T + 10  # the all-NULL stretch crosses a tile edge
    t = table(conn, n, f"CASE WHEN i < {lead} OR i % 4 = 0 THEN NULL ELSE i % 100 - 50 END AS v, "
                       f"CASE WHEN i < {lead} THEN NULL ELSE (i % 64)::DOUBLE END AS d")
    v = [None if i < lead or i % 4 == 0 else i % 100 - 50 for i in range(n)]
    d = [None if i < lead else float(i % 64) for i in range(n)]
    idv = list(range(n))
    calls = [W.Call(f, v, "int", "rows") for f in ("count", "sum", "min", "max", "avg")] + \
            [W.Call(f, d, "f64", "rows") for f in ("count", "sum", "min", "max", "avg")]
    want = W.window(n, [], [(idv, None, "int", False, None)], calls)
    assert want[0][lead - 1] == 0 and want[1][lead - 1] is None and want[4][lead - 1] is None
    spec = "ORDER BY id ROWS BETWEEN UNBOUNDED PRECEDING AND CURRENT ROW"
    for col in (6, 9):
        want[col] = [None if x is None else x[0] for x in want[col]]  # exact: integer-valued doubles
    check(conn, "SELECT " + ", ".join(f"{f}({a}) OVER ({spec})" for a in ("v", "d")
                                      for f in ("count", "sum", "min", "max", "avg")) + f" FROM {t}",
          want, ["text", "text", "text", "text", "f64", "text", "f64", "set", "set", "f64"])


@pytest.mark.parametrize("k", [0, 1, 2, 50])
def test_lag_lead_at_partition_edges(conn, k):
    n = T + 30
    t = table(conn, n, "i // 7 AS p, CASE WHEN i % 9 = 0 THEN NULL ELSE i * 3 END AS v")  # partitions of 7 < 50
    p = [i // 7 for i in range(n)]
    v = [None if i % 9 == 0 else i * 3 for i in range(n)]
    idv = list(range(n))
    want = W.window(n, [(p, None, "int")], [(idv, None, "int", False, None)],
                    [W.Call("lag", v, offset=k), W.Call("lead", v, offset=k)])
    if k == 0:
        assert want[0] == v and want[1] == v
    check(conn, f"SELECT lag(v, {k}) OVER (PARTITION BY p ORDER BY id), lead(v, {k}) OVER (PARTITION BY p ORDER BY id) FROM {t}", want)


# ---- 5. key and argument types ----------------------------------------------------------------
# (type, the key as SQL over i, the same as Python: a value with the key's order and equality)
KEY_TYPES = [
    ("TINYINT", "((i * 37) % 200 - 100)::TINYINT", lambda i: (i * 37) % 200 - 100),
    ("SMALLINT", "((i * 37) % 2000 - 1000)::SMALLINT", lambda i: (i * 37) % 2000 - 1000),
    ("INTEGER", "((i * 7919) % 4001 - 2000)::INTEGER", lambda i: (i * 7919) % 4001 - 2000),
    ("BIGINT", "((i * 7919) % 4001 - 2000) * 4611686018427387", lambda i: ((i * 7919) % 4001 - 2000) * 4611686018427387),
    ("UTINYINT", "((i * 37) % 250)::UTINYINT", lambda i: (i * 37) % 250),
    ("USMALLINT", "((i * 37) % 60000)::USMALLINT", lambda i: (i * 37) % 60000),
    ("UINTEGER", "((i * 7919) % 4001 + 4294960000)::UINTEGER", lambda i: (i * 7919) % 4001 + 4294960000),
    ("UBIGINT", "((i * 7919) % 4001 + 18446744073709500000)::UBIGINT", lambda i: (i * 7919) % 4001 + 18446744073709500000),
    ("BOOLEAN", "(i % 3 = 0)", lambda i: int(i % 3 == 0)),
    ("DATE", None, lambda i: (i * 37) % 3000 - 1500),  # days, through the columnar appender
    ("TIMESTAMP", None, lambda i: ((i * 37) % 3000 - 1500) * 86400000000 + i % 7),  # microseconds
    ("DECIMAL(18,3)", "(((i * 7919) % 4001 - 2000) * 100000000000)::DECIMAL(18,3)", lambda i: (i * 7919) % 4001 - 2000),
    ("DOUBLE", "(((i * 37) % 201 - 100) / 8)::DOUBLE", lambda i: ((i * 37) % 201 - 100) / 8),
    ("FLOAT", "(((i * 37) % 201 - 100) / 8)::FLOAT", lambda i: ((i * 37) % 201 - 100) / 8),
]


@pytest.mark.parametrize("sqltype,expr,py", KEY_TYPES, ids=[t[0] for t in KEY_TYPES])
def test_key_types(conn, mbx, sqltype, expr, py):
    """every type ORDER BY sorts, as PARTITION BY key and as ORDER BY key, with NULL keys (no TIME: it has no
    constructor from an integer here)"""
    n = T + 65
    name = f"w{next(_names)}"
    if expr is None:
        tb = V.Table(name, [V.Col("id", "BIGINT", range(n)),
                            V.Col("kk", sqltype, [py(i) for i in range(n)], [i % 11 != 5 for i in range(n)]),
                            V.Col("v", "BIGINT", [i % 50 for i in range(n)])])
        load(mbx, conn, tb, name, list(range(n)), ["id", "kk", "v"])
    else:
        q(conn, f"CREATE TABLE {name} (id BIGINT, kk {sqltype}, v BIGINT)")
        q(conn, f"INSERT INTO {name} SELECT i, CASE WHEN i % 11 = 5 THEN NULL ELSE {expr} END, i % 50 FROM range({n}) tbl(i)")
    kv = [None if i % 11 == 5 else py(i) for i in range(n)]
    kind = "f64" if sqltype in ("DOUBLE", "FLOAT") else "int"
    ok = [x is not None for x in kv]
    v = [i % 50 for i in range(n)]
    idv = list(range(n))
    want = W.window(n, [(kv, ok, kind)], [(idv, None, "int", True, None)],
                    [W.Call("row_number"), W.Call("sum", v, "int", "range")]) + \
        W.window(n, [(kv, ok, kind)], [], [W.Call("count_star", frame="part")]) + \
        W.window(n, [], [(kv, ok, kind, True, True)], [W.Call("rank"), W.Call("dense_rank"), W.Call("count", v, "int", "range")])
    check(conn, f"SELECT row_number() OVER (PARTITION BY kk ORDER BY id DESC), sum(v) OVER (PARTITION BY kk ORDER BY id DESC), "
                f"count(*) OVER (PARTITION BY kk), rank() OVER (ORDER BY kk DESC NULLS FIRST), "
                f"dense_rank() OVER (ORDER BY kk DESC NULLS FIRST), count(v) OVER (ORDER BY kk DESC NULLS FIRST) FROM {name}", want)


def test_double_min_max_and_sums(conn):
    n = MULTI
    rows = []
    rng = np.random.default_rng(20261021)
    specials = [math.nan, math.inf, -math.inf, 0.0, -0.0]
    for i in range(n):
        x = float(rng.normal()) * 10.0 ** int(rng.integers(-3, 6))
        if i % 97 == 13:
            x = specials[(i // 97) % 5]
        rows.append((i, i % 5, None if i % 13 == 7 else x, float(int(rng.integers(-2 ** 39, 2 ** 39)))))
    fill(conn, "wdbl", "id BIGINT, k BIGINT, x DOUBLE, e DOUBLE", rows)
    k = [r[1] for r in rows]
    x = [r[2] for r in rows]
    e = [r[3] for r in rows]
    finite = [None if v is None or v != v or math.isinf(v) else v for v in x]
    idv = list(range(n))
    calls = [W.Call("min", x, "f64", "rows"), W.Call("max", x, "f64", "rows"), W.Call("min", x, "f64", "part"),
             W.Call("sum", e, "f64", "rows"), W.Call("sum", e, "f64", "part")]
    want = W.window(n, [(k, None, "int")], [(idv, None, "int", False, None)], calls)
    for col in (3, 4):
        want[col] = [None if v is None else v[0] for v in want[col]]
    spec = "PARTITION BY k ORDER BY id ROWS UNBOUNDED PRECEDING"
    check(conn, f"SELECT min(x) OVER ({spec}), max(x) OVER ({spec}), min(x) OVER (PARTITION BY k), sum(e) OVER ({spec}), "
                f"sum(e) OVER (PARTITION BY k) FROM wdbl", want, ["set", "set", "set", "f64", "f64"])
    # arbitrary finite doubles: within 1e-9 * sum|x|
    fill(conn, "wdbl2", "id BIGINT, k BIGINT, x DOUBLE", [(r[0], r[1], f) for r, f in zip(rows, finite)])
    calls = [W.Call("sum", finite, "f64", "rows"), W.Call("avg", finite, "f64", "range")]
    want = W.window(n, [(k, None, "int")], [(idv, None, "int", False, None)], calls)
    sql = f"SELECT sum(x) OVER ({spec}), avg(x) OVER (PARTITION BY k ORDER BY id) FROM wdbl2"
    check(conn, sql, want, ["tol", "tol"])
    first, _ = cells(conn, sql)
    again, _ = cells(conn, sql)
    assert first == again  # the scan's shape depends on the row count alone


# ---- 6. composition -----------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small(conn):
    n = T + 65
    t = "wsmall"
    fill(conn, t, "id BIGINT, k BIGINT, v BIGINT, s VARCHAR", [(i, i % 6, (i * 31) % 101, f"row{i % 4}") for i in range(n)])
    return t, n, [i % 6 for i in range(n)], [(i * 31) % 101 for i in range(n)], [f"row{i % 4}" for i in range(n)]


def test_shared_and_distinct_specifications(conn, small):
    t, n, k, v, s = small
    q(conn, f"SELECT row_number() OVER (PARTITION BY k ORDER BY v), sum(v) OVER (PARTITION BY k ORDER BY v) FROM {t}")
    assert kernels(conn).count("window_bounds") == 1
    q(conn, f"SELECT row_number() OVER (PARTITION BY k ORDER BY v), sum(v) OVER (PARTITION BY k ORDER BY v DESC) FROM {t}")
    assert kernels(conn).count("window_bounds") == 2
    q(conn, f"SELECT sum(v) OVER (), count(*) OVER () FROM {t}")
    names = kernels(conn)
    assert "radix_sort" not in names and names.count("window_bounds") == 1


def test_window_inside_arithmetic_with_passthrough_columns(conn, small):
    t, n, k, v, s = small
    idv = list(range(n))
    lag, tot, ptot = W.window(n, [(k, None, "int")], [(idv, None, "int", False, None)],
                              [W.Call("lag", v), W.Call("sum", v, "int", "part")]) + \
        W.window(n, [], [], [W.Call("sum", v, "int", "part")])
    want = [s, [None if l is None else x - l for x, l in zip(v, lag)],
            [100 * p / a for p, a in zip(tot, ptot)]]
    check(conn, f"SELECT s, v - lag(v) OVER (PARTITION BY k ORDER BY id), "
                f"100 * sum(v) OVER (PARTITION BY k) / sum(v) OVER () FROM {t}", want, ["text", "text", "f64"])


def test_window_over_a_filtered_table(conn, small):
    t, n, k, v, s = small
    keep = [i for i in range(n) if v[i] > 40]
    kk, vv = [k[i] for i in keep], [v[i] for i in keep]
    want = W.window(len(keep), [(kk, None, "int")], [(vv, None, "int", False, None)],
                    [W.Call("rank"), W.Call("sum", vv, "int", "range")])
    check(conn, f"SELECT id, rank() OVER (PARTITION BY k ORDER BY v), sum(v) OVER (PARTITION BY k ORDER BY v) FROM {t} "
                f"WHERE v > 40", [keep] + want)


def test_window_over_a_join_and_a_group_by_subquery(conn, small):
    t, n, k, v, s = small
    q(conn, "CREATE TABLE wdim AS SELECT i AS k, i * 10 AS w FROM range(6) tbl(i)")
    text, nulls = cells(conn, f"SELECT a.id, row_number() OVER (PARTITION BY b.w ORDER BY a.v, a.id) "
                              f"FROM {t} a JOIN wdim b ON a.k = b.k")
    assert len(text) == n
    ids = [int(r[0]) for r in text]
    kk, vv = [k[i] * 10 for i in ids], [v[i] for i in ids]
    want = W.window(n, [(kk, None, "int")], [(vv, None, "int", False, None), (ids, None, "int", False, None)],
                    [W.Call("row_number")])
    assert [int(r[1]) for r in text] == want[0]
    # the aggregate in a subquery, the window over it
    text, _ = cells(conn, f"SELECT k, c, rank() OVER (ORDER BY c DESC), sum(c) OVER () "
                          f"FROM (SELECT k, count(*) c FROM {t} GROUP BY k) g")
    ks, cs = [int(r[0]) for r in text], [int(r[1]) for r in text]
    assert sorted(ks) == list(range(6)) and all(cs[j] == k.count(ks[j]) for j in range(6))
    want = W.window(6, [], [(cs, None, "int", True, None)], [W.Call("rank")])
    assert [int(r[2]) for r in text] == want[0] and all(int(r[3]) == n for r in text)


def test_union_order_limit_ctas_and_prepared(conn, small, mbx):
    t, n, k, v, s = small
    idv = list(range(n))
    rn = W.window(n, [(k, None, "int")], [(v, None, "int", False, None), (idv, None, "int", False, None)],
                  [W.Call("row_number")])[0]
    check(conn, f"SELECT id FROM {t} WHERE id < 3 UNION ALL SELECT row_number() OVER (PARTITION BY k ORDER BY v, id) FROM {t}",
          [[0, 1, 2] + rn])
    text, _ = cells(conn, f"SELECT id, row_number() OVER (PARTITION BY k ORDER BY v, id) rn FROM {t} ORDER BY rn DESC, id LIMIT 5")
    top = sorted(range(n), key=lambda i: (-rn[i], i))[:5]
    assert [(int(r[0]), int(r[1])) for r in text] == [(i, rn[i]) for i in top]
    q(conn, f"CREATE TABLE wctas AS SELECT id, sum(v) OVER (PARTITION BY k ORDER BY id) AS run FROM {t}")
    run = W.window(n, [(k, None, "int")], [(idv, None, "int", False, None)], [W.Call("sum", v, "int", "range")])[0]
    check(conn, "SELECT id, run FROM wctas", [idv, run])
    st = conn.prepare(f"SELECT sum(v + ?) OVER (PARTITION BY k ORDER BY id) FROM {t}").value
    for add in (0, 1000):
        st.bind_bigint(1, add)
        r = st.execute()
        assert isinstance(r, mbx.Ok), r
        va = [x + add for x in v]
        want = W.window(n, [(k, None, "int")], [(idv, None, "int", False, None)], [W.Call("sum", va, "int", "range")])[0]
        assert [row[0] for row in r.value.rows] == [str(x) for x in want]
    st.close()


def test_unchanged_paths_run_no_window_kernel(conn, small):
    t, n, k, v, s = small
    for sql in (f"SELECT id, v FROM {t} ORDER BY v, id", f"SELECT k, sum(v) FROM {t} GROUP BY k"):
        q(conn, sql)
        assert not [nm for nm in kernels(conn) if nm.startswith("window_")], sql
