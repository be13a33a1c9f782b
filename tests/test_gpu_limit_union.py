"""LIMIT / OFFSET (RunSelectDev: the in-place slice of a top-level result whose
bitmaps start on a word, the gather otherwise, for strings and inside a
subquery) and UNION ALL (ConcatRels, BitmapAppend at destination offsets that
are no multiple of 64, a NULL-free branch next to a NULL-able one, string
branches with different character counts) against Python slices and
concatenations of the source rows.

Every result is read three ways: cell by cell, through the Arrow getters
(plain and _nullable, byte-exact against oracle/wire.py) and through a second
query over a CREATE TABLE AS of it.  Integers as text, doubles by bit pattern,
strings as text; nothing has a tolerance."""
import math
import struct

import pytest

import sort_model as M
from conftest import q
from gpu_tables import fill, profiled
from oracle import wire

pytestmark = pytest.mark.gpu

N = 300
H = 10 ** 20
OFFSETS = [0, 1, 63, 64, 65, 128, 299, 300, 305]
LIMITS = [None, 0, 1, 64, 1000]
DOUBLES = [0.0, -0.0, 1.5, -2.25, math.inf, -math.inf, 5e-324, 1e300, 0.1]


def source_rows():
    """(id, i, d, s, h): id plain, the others NULL-able, each on its own rows"""
    rows = []
    for k in range(N):
        rows.append((k,
                     None if k % 7 == 2 else (k * 37) % 11 - 5,
                     None if k % 5 == 1 else DOUBLES[(k * 3 + k // 9) % len(DOUBLES)],
                     None if k % 6 == 4 else ["", "a", "é", "limit", "x" * 17][(k * 5 + k // 7) % 5] + ("" if k % 4 else str(k)),
                     None if k % 9 == 3 else ((k * 7919) % 1000 - 500) * H))
    return rows


ROWS = source_rows()
NAMES = ["id", "i", "d", "s", "h"]
KINDS = {"id": "int64", "i": "int32", "d": "double", "s": "string", "h": "string"}


class Db:
    pass


@pytest.fixture(scope="module")
def db(mbx):
    d = Db()
    d.mbx, d.c, d.seq = mbx, profiled(mbx), 0
    fill(d.c, "l0", "id BIGINT, i BIGINT, d DOUBLE, s VARCHAR, hb BIGINT",
         [(r[0], r[1], r[2], r[3], None if r[4] is None else r[4] // H) for r in ROWS])
    q(d.c, f"CREATE TABLE l AS SELECT id, CAST(i AS INTEGER) AS i, d, s, CAST(hb AS HUGEINT) * {H} AS h FROM l0")
    for name, rows in PARTS.items():
        fill(d.c, name, "id BIGINT, a BIGINT, s VARCHAR", rows)
    yield d
    d.c.close()


def cell_text(name, v):
    return v if name == "s" else str(v)


def check_cells(conn, sql, names, want):
    res = conn.query_raw(sql)
    assert res.row_count() == len(want), (sql, res.row_count(), len(want))
    text, nulls = res.cells()
    for k, row in enumerate(want):
        for j, name in enumerate(names):
            v = row[j]
            assert nulls[k][j] == (v is None), (sql, k, name)
            if v is None:
                continue
            if name == "d":
                assert res.raw(j, k) == struct.pack("<d", v), (sql, k, res.raw(j, k), v)
            else:
                assert text[k][j] == cell_text(name, v), (sql, k, name, text[k][j], v)
    res.close()


def check_arrow(mbx, conn, sql, names, want):
    a = conn.query_arrow(sql).value
    assert a.row_count() == len(want), (sql, a.row_count())
    for j, name in enumerate(names):
        vals = [r[j] for r in want]
        kind = KINDS.get(name, "int64")
        if kind == "string":
            vals = [None if v is None else cell_text(name, v) for v in vals]
        for nullable in (False, True):
            got = a._buf(kind, j, nullable)
            exp = getattr(wire, kind)(vals, nullable)
            assert got == exp, (sql, name, nullable, len(got), len(exp), got[:48], exp[:48])
    a.close()


def check_three_ways(db, sql, names, want):
    check_cells(db.c, sql, names, want)
    check_arrow(db.mbx, db.c, sql, names, want)
    db.seq += 1
    q(db.c, f"CREATE TABLE ctas{db.seq} AS {sql}")
    check_cells(db.c, f"SELECT * FROM ctas{db.seq}", names, want)
    q(db.c, f"DROP TABLE ctas{db.seq}")


def _slice(rows, off, lim):
    return rows[off:] if lim is None else rows[off:off + lim]


ID_ORDER = M.order(N, [([r[1] for r in ROWS], [r[1] is not None for r in ROWS], "int", True, True),
                       (list(range(N)), None, "int", False, None)])


@pytest.mark.parametrize("off", OFFSETS)
def test_limit_offset(db, off):
    for names in (["id", "i", "d", "h"], NAMES):  # without a string column the top-level result can be sliced in place
        plain = [tuple(r[NAMES.index(n)] for n in names) for r in ROWS]
        ordered = [plain[k] for k in ID_ORDER]
        for lim in LIMITS:
            tail = ("" if lim is None else f" LIMIT {lim}") + (f" OFFSET {off}" if off or lim is None else "")
            if not tail:
                tail = " OFFSET 0"
            for order, rows in (("", plain), (" ORDER BY i DESC NULLS FIRST, id", ordered)):
                inner = f"SELECT {', '.join(names)} FROM l{order}{tail}"
                want = _slice(rows, off, lim)
                check_three_ways(db, inner, names, want)
                check_three_ways(db, f"SELECT * FROM ({inner}) u", names, want)


def test_limit_offset_of_range(db):
    check_three_ways(db, "SELECT i FROM range(300) tbl(i) LIMIT 70 OFFSET 65", ["r"], [(k,) for k in range(65, 135)])


# ---- UNION ALL ---------------------------------------------------------------------------------
def part(size, nulls, strings):
    """`size` rows (id, a, s); ids are unique across the parts"""
    rows = []
    for k in range(size):
        a = None if nulls and k % 3 == 1 else (k * 7 + size) % 9 - 4
        s = None if nulls and k % 4 == 2 else strings[(k + size) % len(strings)]
        rows.append((size * 1000 + k, a, s))
    return rows


PARTS = {"p1": part(1, False, ["one"]), "p63": part(63, True, ["", "u", "union", "é" * 9]), "p64": part(64, False, [""]),
         "p65": part(65, True, ["sixty-five", "s"]), "p130": part(130, True, ["", "long" * 10, "z"]),
         "q63": part(63, False, ["q"])}
for _n, _rows in PARTS.items():  # ids unique across parts of equal size too
    PARTS[_n] = [(r[0] + (500 if _n == "q63" else 0), r[1], r[2]) for r in _rows]
EMPTY = "p64 WHERE false"
UNIONS = [
    [EMPTY, "p63"], ["p65", EMPTY], ["p63", "p64"], ["q63", "p63"],
    ["p1", "p63", "p65"], ["p63", EMPTY, "p65"], ["p64", "p1", EMPTY], ["p65", "q63", "p130"],
    [EMPTY, "p65", "p63", "p1", "p130"], ["p130", "p63", EMPTY, "p1", "p64"], ["p1", "p1", "q63", "p65", EMPTY],
    ["p64", "p64", "p63", "q63", "p65"],
]


def test_the_parts_are_what_the_cases_need():
    assert all(r[1] is not None and r[2] is not None for n in ("p1", "p64", "q63") for r in PARTS[n])  # no bitmap at all
    assert {r[2] for r in PARTS["p64"]} == {""}  # a string branch without a single character
    assert any(r[1] is None for r in PARTS["p63"]) and any(r[2] is None for r in PARTS["p130"])
    assert sorted({len(b) for b in UNIONS}) == [2, 3, 5]
    assert {b.index(EMPTY) for b in UNIONS if EMPTY in b if len(b) > 2} >= {0, 1, 2, 4}


@pytest.mark.parametrize("branches", UNIONS, ids=lambda b: "+".join(x.split()[0] if x != EMPTY else "none" for x in b))
def test_union_all(db, branches):
    names = ["id", "a", "s"]
    sql = " UNION ALL ".join(f"SELECT id, a, s FROM {b}" for b in branches)
    want = [r for b in branches if b != EMPTY for r in PARTS[b]]
    if branches.count("p1") == 2 or branches.count("p64") == 2:  # the same table twice: its rows twice
        assert len(want) > len({r[0] for r in want})
    check_three_ways(db, sql, names, want)
    # and a sort with a limit on top, by the sort model; `pos` breaks the ties a repeated branch leaves
    n = len(want)
    a, s = [r[1] for r in want], [r[2] or "" for r in want]
    keys = [(a, [r[1] is not None for r in want], "int", True, True), (s, [r[2] is not None for r in want], "str", False, None),
            ([r[0] for r in want], None, "int", False, None), (list(range(n)), None, "int", False, None)]
    order = [want[k] for k in M.order(n, keys)]
    check_three_ways(db, sql + " ORDER BY a DESC NULLS FIRST, s, id LIMIT 50 OFFSET 3", names, order[3:53])
    check_cells(db.c, sql + " ORDER BY a DESC NULLS FIRST, s, id", names, order)
