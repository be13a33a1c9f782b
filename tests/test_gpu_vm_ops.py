"""Every expression-VM instruction on the device, by both device engines: the
tile interpreter (MBX_JIT=0: vm_filter / vm_project) and the run-time compiled
kernels (MBX_JIT=sync: jit_filter / jit_project), against the exact model of
tests/vm_reference.py over the tables of tests/vm_cases.py.  Integers,
decimals and booleans are compared as text, DOUBLE and FLOAT by bit pattern
(any NaN matches NaN; -0.0 and +0.0 differ)."""
import pytest

import vm_cases as V
import vm_reference as R
from conftest import q
from gpu_tables import _f64, load

pytestmark = pytest.mark.gpu

ENGINES = {"0": ("vm_filter", "vm_project"), "sync": ("jit_filter", "jit_project")}
CHUNK = 6  # expressions per SELECT: well inside VM_MAX_INS / VM_MAX_REGS / VM_MAX_COLS of one program


def _conn(mbx):
    cfg = mbx.Config.create()
    assert isinstance(cfg.set("mbx_profile", "true"), mbx.Ok)
    r = mbx.connect_with_config(cfg)
    assert isinstance(r, mbx.Ok), r.error.message
    return r.value


def _kernels(c):
    return [k["name"] for k in c.last_profile()["kernels"]]


def check_projection(conn, cases, source, rows, where=None):
    """SELECT <cases> FROM source [WHERE where]: row k of the result is row rows[k] of the model"""
    sql = "SELECT " + ", ".join(c.sql for c in cases) + f" FROM {source}" + (f" WHERE {where}" if where else "")
    res = conn.query_raw(sql)
    assert res.row_count() == len(rows), (sql, res.row_count(), len(rows))
    text, nulls = res.cells()
    bad = []
    for j, c in enumerate(cases):
        assert conn_type(res, j) == c.rtype, (c.sql, conn_type(res, j))
        for k, r in enumerate(rows):
            st, want = c.expect(r)
            assert st == "ok", (c.sql, r)
            if want is None or nulls[k][j]:
                ok = (want is None) and nulls[k][j]
                got = None if nulls[k][j] else text[k][j]
            elif c.out in ("f64", "f32"):
                got = _f64(res.raw(j, k))
                ok = (got != got) if want != want else R.bits(got) == R.bits(want)
                if not ok:
                    got, want = (got, hex(R.bits(got))), (want, hex(R.bits(want)))
            else:
                got = text[k][j]
                ok = got == c.text(want)
            if not ok:
                bad.append((c.sql, r, {n: c.table.cols[n].get(r) for n in c.cols}, got, want))
    res.close()
    assert not bad, (len(bad), bad[:8])


_mbx = None


def conn_type(res, j):
    return _mbx.column_type_from_id(res.column_type(j))


def chunks(cases):
    for lo in range(0, len(cases), CHUNK):
        yield cases[lo:lo + CHUNK]


def usable(cases):
    return [r for r in range(V.N) if all(c.expect(r)[0] == "ok" for c in cases)]


@pytest.fixture()
def engine(request, mbx, monkeypatch):
    global _mbx
    _mbx = mbx
    monkeypatch.setenv("MBX_JIT", request.param)
    c = _conn(mbx)
    yield c, ENGINES[request.param]
    c.close()


def _source(mbx, conn, cases, rows, name):
    t = cases[0].table
    if t.source != t.name:  # range(): nothing to load, every row usable
        assert rows == list(range(V.N))
        return t.source
    cols = ["id"] + sorted({k for c in cases for k in c.cols} - {"id"})
    load(mbx, conn, t, name, rows, cols)
    return name


@pytest.mark.parametrize("engine", list(ENGINES), indirect=True)
@pytest.mark.parametrize("fam", V.FAMILIES)
def test_projection(mbx, engine, fam):
    conn, (_, kproject) = engine
    for n, part in enumerate(chunks(V.family(fam))):
        rows = usable(part)
        assert len(rows) > 3 * 256  # still three full tiles and a tail
        src = _source(mbx, conn, part, rows, f"p{n}")
        check_projection(conn, part, src, rows)
        assert _kernels(conn) == [kproject], (fam, n, _kernels(conn))


@pytest.mark.parametrize("engine", list(ENGINES), indirect=True)
@pytest.mark.parametrize("fam", [f for f in V.FAMILIES if any(c.is_bool for c in V.family(f))])
def test_filter(mbx, engine, fam):
    conn, (kfilter, kproject) = engine
    for n, c in enumerate(x for x in V.family(fam) if x.is_bool):
        rows = usable([c])
        src = _source(mbx, conn, [c], rows, f"f{n}")
        idc = "id" if "id" in c.table.cols else "i"
        got = [int(r[0]) for r in q(conn, f"SELECT {idc} FROM {src} WHERE {c.sql}").rows]
        want = [r for r in rows if c.expect(r)[1] is True]  # a NULL predicate selects nothing
        assert got == want, (c.sql, len(got), len(want), sorted(set(got) ^ set(want))[:10])
        assert _kernels(conn) == [kfilter] + ([kproject] if want else []), (c.sql, _kernels(conn))


# ---- structure: tile boundaries and empty tiles --------------------------------------------
_T = "ti"
STRUCT_CASES = [
    V.Case("struct", _T, "ba % bb", "BigInt", "int", lambda r: R.imod("BIGINT", r["ba"], r["bb"]), ""),
    V.Case("struct", _T, "ba / bb", "Double", "f64", lambda r: R.fop("/", R.int_to_f64(r["ba"]), R.int_to_f64(r["bb"])), ""),
    V.Case("struct", _T, "CAST(ia AS BIGINT) * ib", "BigInt", "int", lambda r: R.mul("BIGINT", r["ia"], r["ib"]), ""),
    V.Case("struct", _T, "COALESCE(ban, bbn)", "BigInt", "int", lambda r: R.coalesce(r["ban"], r["bbn"]), ""),
    V.Case("struct", _T, "ban < bbn", "Boolean", "bool", lambda r: R.compare("<", r["ban"], r["bbn"]), ""),
    V.Case("struct", _T, "id", "BigInt", "int", lambda r: r["id"], ""),
]
PREDICATES = {"all": ("id % 1 = 0", lambda i: True), "none": ("id % 1 = 1", lambda i: False),
              "tile1": ("id // 256 = 1", lambda i: i // 256 == 1), "alternate": ("id % 2 = 0", lambda i: i % 2 == 0)}


@pytest.mark.parametrize("engine", list(ENGINES), indirect=True)
@pytest.mark.parametrize("n", [1, 255, 256, 257, 1000])
def test_structure(mbx, engine, n):
    conn, (kfilter, kproject) = engine
    rows = list(range(n))
    assert usable(STRUCT_CASES) == list(range(V.N))
    src = _source(mbx, conn, STRUCT_CASES, rows, "s")
    for name, (pred, keep) in PREDICATES.items():
        sel = [r for r in rows if keep(r)]
        check_projection(conn, STRUCT_CASES, src, sel, pred)
        assert _kernels(conn) == [kfilter] + ([kproject] if sel else []), (n, name, _kernels(conn))


# ---- errors: raise, NULL operand, row filtered out --------------------------------------------
@pytest.fixture()
def errconn(engine, mbx):
    conn, names = engine
    t = V.TABLES["te"]
    load(mbx, conn, t, "te", list(range(V.N)), list(t.cols))
    return conn, names


@pytest.mark.parametrize("engine", list(ENGINES), indirect=True)
@pytest.mark.parametrize("part", range(4))
def test_errors(mbx, errconn, part):
    conn, (kfilter, kproject) = errconn
    for e in V.ERR_CASES[part::4]:
        r = conn.query(f"SELECT {e.sql} FROM te")
        assert isinstance(r, mbx.Err) and r.error.message.startswith(e.kind + " Error"), (e.name, r)
        res = q(conn, f"SELECT {e.sql_null} FROM te")  # the offending operand NULL: no error, NULL there
        assert [k for k in range(V.N) if res.nulls[k][0]] == [V.ERR_ROW], e.name
        assert _kernels(conn) == [kproject], (e.name, _kernels(conn))
        res = q(conn, f"SELECT {e.sql} FROM te WHERE {V.ERR_KEEP_OTHERS}")  # the row removed by the VM's own predicate
        assert res.row_count() == V.N - 1 and not any(x[0] for x in res.nulls), e.name
        assert _kernels(conn) == [kfilter, kproject], (e.name, _kernels(conn))


def test_aggregate_carries_the_rule(mbx, monkeypatch):
    """the fused aggregate kernel (jit_aggregate) has its own copy of `active`"""
    global _mbx
    _mbx = mbx
    monkeypatch.setenv("MBX_JIT", "sync")
    conn = _conn(mbx)
    t = V.TABLES["te"]
    load(mbx, conn, t, "te", list(range(V.N)), list(t.cols))
    byname = {e.name: e for e in V.ERR_CASES}
    for name, unit in (("add64", (V.I64MAX % 1000)), ("mul128", (2 ** 126 % 1000))):
        e = byname[name]
        r = conn.query(f"SELECT COUNT(*), SUM(({e.sql}) % 1000) FROM te WHERE id % 2 = 0")
        assert isinstance(r, mbx.Err) and r.error.message.startswith(e.kind + " Error"), (name, r)
        got = q(conn, f"SELECT COUNT(*), SUM(({e.sql_null}) % 1000) FROM te WHERE id % 2 = 0").rows
        assert got == [["500", str(499 * unit)]], (name, got)
        assert _kernels(conn) == ["jit_aggregate"], _kernels(conn)
        got = q(conn, f"SELECT COUNT(*), SUM(({e.sql}) % 1000) FROM te WHERE id % 2 = 0 AND {V.ERR_KEEP_OTHERS}").rows
        assert got == [["499", str(499 * unit)]], (name, got)
        assert _kernels(conn) == ["jit_aggregate"], _kernels(conn)
    # the fused GROUP BY kernel (jit_group: 64-bit arguments, a key column with a zone map,
    # which CREATE TABLE AS computes) is generated with the same mask
    q(conn, "CREATE TABLE teg AS SELECT CAST(id % 4 AS INTEGER) AS gk, id, one FROM te")
    e, unit = byname["add64"], V.I64MAX % 1000
    grouped = f"SELECT gk, COUNT(*), SUM(({e.sql}) % 1000) FROM teg WHERE {{}} GROUP BY gk"
    r = conn.query(grouped.format("id % 2 = 0"))
    assert isinstance(r, mbx.Err) and r.error.message.startswith(e.kind + " Error"), r
    got = q(conn, grouped.format(f"id % 2 = 0 AND {V.ERR_KEEP_OTHERS}")).rows
    assert got == [["0", "249", str(249 * unit)], ["2", "250", str(250 * unit)]], got
    assert _kernels(conn) == ["jit_group"], _kernels(conn)
    conn.close()


# ---- ORDER BY over doubles: f64_order must agree with V_CMP_F ---------------------------------------
def test_double_ordering(mbx):
    global _mbx
    _mbx = mbx
    conn = _conn(mbx)
    tf = V.TABLES["tf"]
    n = 300
    # fc: the double edge list first; fcn / ran: their NULL-able twins
    t = V.Table("so", [V.Col("id", "BIGINT", range(n)), V.Col("d", "DOUBLE", tf.cols["fcn"].values[:n], tf.cols["fcn"].valid[:n]),
                       V.Col("f", "FLOAT", tf.cols["ran"].values[:n], tf.cols["ran"].valid[:n])])
    load(mbx, conn, t, "so", list(range(n)), ["id", "d", "f"])
    for col, order, nulls_first in (("d", "d", False), ("d", "d DESC NULLS FIRST", True), ("f", "f", False)):
        res = conn.query_raw(f"SELECT {col} FROM so ORDER BY {order}")
        assert res.row_count() == n
        _, nulls = res.cells()
        isnull = [x[0] for x in nulls]
        nn = isnull.count(True)
        assert nn == t.cols[col].valid.count(False) > 0
        assert isnull == ([True] * nn + [False] * (n - nn) if nulls_first else [False] * (n - nn) + [True] * nn), order
        got = [_f64(res.raw(0, k)) for k in range(n) if not isnull[k]]
        res.close()
        sign = -1 if "DESC" in order else 1
        assert all(sign * R.cmp3(got[k], got[k + 1]) <= 0 for k in range(len(got) - 1)), order
        canon = lambda v: "nan" if v != v else R.bits(v)
        src = [v for v, ok in zip(t.cols[col].values, t.cols[col].valid) if ok]
        assert sorted(map(str, map(canon, got))) == sorted(map(str, map(canon, src))), order
    conn.close()
