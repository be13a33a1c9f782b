"""x [NOT] IN (subquery) on the device: the subquery's keys go into the join's
table once per statement (join_keys, radix_sort, join_build), join_probe_mark
writes one BOOLEAN byte per probe row and, where join_mark_plan.h asks for one,
its validity word per wave64 ballot, and the expression VM reads that column
wherever the leaf stood.

The model is in3(x, S) -> True / False / None, SQL's three-valued IN as DuckDB
answers it; NOT IN is its three-valued negation; a WHERE keeps True only.  Rows
are compared as sorted multisets of text cells (None for NULL), as in
test_gpu_join.py.  Probe sizes straddle the 64 rows of a validity word and the
256 rows a wave owns per step (0, 1, 63, 64, 65, 255, 256, 257, 4097), each with
NULL keys in its last, partial validity word; the large case (1 200 003 rows)
is more than one sweep of the grid."""
import numpy as np
import pytest

from conftest import one, q
from gpu_tables import fill, kernels, profiled

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def c(mbx):
    conn = profiled(mbx)
    yield conn
    conn.close()


# ---- the model ----------------------------------------------------------------------------------------
def in3(x, S):
    """x IN S with SQL's NULLs: S is the list of the subquery's rows (None for NULL)"""
    if len(S) == 0:
        return False
    if x is None:
        return None
    if any(s is not None and s == x for s in S):
        return True
    if any(s is None for s in S):
        return None
    return False


def not3(v):
    return None if v is None else not v


class Lit(str):
    """SQL text used as it stands (DATE '...', a DECIMAL literal) whose result cell is `cell`"""
    def __new__(cls, sql, cell):
        s = super().__new__(cls, sql)
        s.cell = cell
        return s


def _sql(v):
    if v is None:
        return "NULL"
    if isinstance(v, Lit):
        return str(v)
    if isinstance(v, bool):
        return "true" if v else "false"
    if isinstance(v, str):
        return "'" + v.replace("'", "''") + "'"
    return repr(v)


def _cell(v):
    if v is None:
        return None
    if isinstance(v, Lit):
        return v.cell
    if isinstance(v, bool):
        return "true" if v else "false"
    return str(v)


def make(c, name, cols, rows):
    q(c, f"DROP TABLE IF EXISTS {name}")
    q(c, f"CREATE TABLE {name} ({cols})")
    for at in range(0, len(rows), 400):
        q(c, f"INSERT INTO {name} VALUES " + ", ".join("(" + ", ".join(_sql(v) for v in r) + ")" for r in rows[at:at + 400]))


def got(c, sql):
    res = q(c, sql)
    return [tuple(None if res.nulls[i][j] else res.rows[i][j] for j in range(len(res.rows[i]))) for i in range(len(res.rows))]


def cells(rows):
    return [tuple(_cell(v) for v in r) for r in rows]


def same(got_rows, want_rows):
    key = lambda r: tuple((x is None, x or "") for x in r)
    assert sorted(got_rows, key=key) == sorted(cells(want_rows), key=key)


def check_both_places(c, table, rows, sub, S, key=lambda r: r[0], left="k"):
    """`left` [NOT] IN (sub) over `table` (rows: (k, id)), read in a WHERE and in the select list"""
    marks = [in3(key(r), S) for r in rows]
    same(got(c, f"SELECT id FROM {table} WHERE {left} IN ({sub})"), [(r[1],) for r, m in zip(rows, marks) if m is True])
    same(got(c, f"SELECT id FROM {table} WHERE {left} NOT IN ({sub})"),
         [(r[1],) for r, m in zip(rows, marks) if not3(m) is True])
    same(got(c, f"SELECT id, {left} IN ({sub}), {left} NOT IN ({sub}) FROM {table}"),
         [(r[1], m, not3(m)) for r, m in zip(rows, marks)])


# ---- sizes --------------------------------------------------------------------------------------------
SIZES = [0, 1, 63, 64, 65, 255, 256, 257, 4097]
SETS = {0: [], 1: [7], 3: [0, 7, 1499], 1000: [k for k in range(1500) if k % 3 != 2]}


def probe_rows(n):
    """(k, id): keys in [0, 1500); NULL keys in the last, partial validity word (every other row of
    it, its first and the table's last row among them) and sprinkled before it"""
    last = 64 * ((n - 1) // 64) if n else 0
    rows = []
    for i in range(n):
        null = (i >= last and (i - last) % 2 == 0) or i == n - 1 or i % 11 == 3
        rows.append((None if null else (i * 7) % 1500, i))
    return rows


@pytest.fixture(scope="module")
def sized(c):
    for n in SIZES:
        make(c, f"pn{n}", "k BIGINT, id BIGINT", probe_rows(n))
    for m, S in SETS.items():
        make(c, f"sm{m}", "k BIGINT", [(k,) for k in S])
    return True


@pytest.mark.parametrize("m", list(SETS))
@pytest.mark.parametrize("n", SIZES)
def test_probe_and_set_sizes(c, sized, n, m):
    rows = probe_rows(n)
    if n:
        assert rows[-1][0] is None and (n == 1 or any(r[0] is not None for r in rows))
    check_both_places(c, f"pn{n}", rows, f"SELECT k FROM sm{m}", SETS[m])
    if n and m:
        names = kernels(c)  # of the select-list statement: two identical leaves and their negation
        assert names.count("join_probe_mark") == 1 and names.count("join_build") == 1, names


# ---- the NULL matrix ----------------------------------------------------------------------------------
SET_KINDS = {
    "an empty table": ("SELECT k FROM ne", []),
    "empty after its own WHERE": ("SELECT k FROM nn WHERE k > 1000000", []),
    "rows, no NULL": ("SELECT k FROM nv", [1, 5, 9, 64, 129]),
    "rows and a NULL": ("SELECT k FROM nn", [1, 5, None, 9, 64, 129, None]),
    "NULLs only": ("SELECT k FROM nn WHERE k IS NULL", [None, None]),
}


@pytest.fixture(scope="module")
def nullm(c):
    make(c, "ne", "k BIGINT", [])
    make(c, "nv", "k BIGINT", [(k,) for k in SET_KINDS["rows, no NULL"][1]])
    make(c, "nn", "k BIGINT", [(k,) for k in SET_KINDS["rows and a NULL"][1]])
    P = {True: [(None if i % 4 == 2 or i >= 128 else i, i) for i in range(131)], False: [(i, i) for i in range(131)]}
    make(c, "npn", "k BIGINT, id BIGINT", P[True])
    make(c, "npv", "k BIGINT, id BIGINT", P[False])
    return P


@pytest.mark.parametrize("kind", list(SET_KINDS))
@pytest.mark.parametrize("nullable", [False, True])
def test_null_matrix(c, nullm, nullable, kind):
    sub, S = SET_KINDS[kind]
    rows = nullm[nullable]
    check_both_places(c, "npn" if nullable else "npv", rows, sub, S)
    marks = [in3(r[0], S) for r in rows]
    assert one(c, f"SELECT COUNT(*) FROM {'npn' if nullable else 'npv'} WHERE k NOT IN ({sub})") == \
        [str(sum(1 for m in marks if m is False))]
    if any(s is None for s in S):  # one NULL in the set empties every NOT IN filter
        assert all(not3(m) is not True for m in marks)
    if not S:  # no row at all: FALSE even for a NULL key, and nothing is launched
        assert all(m is False for m in marks)
        assert "join_probe_mark" not in kernels(c)


# ---- key types ----------------------------------------------------------------------------------------
def _date(d):
    return Lit(f"DATE '2024-01-{d:02d}'", f"2024-01-{d:02d}")


def _dec(cents):
    t = f"{cents // 100}.{cents % 100:02d}"
    return Lit(t, t)


I64_MIN, I64_MAX = -9223372036854775808, 9223372036854775807

KEY_CASES = {
    "negative INTEGER with BIGINT": ("INTEGER", [-5, -1, 0, 3, -2147483648, 2147483647],
                                     "BIGINT", [-1, -5, 3, 4294967295, -2147483648, 2147483648, 2147483647]),
    "UINTEGER above 2^31 with INTEGER": ("UINTEGER", [4294967295, 2147483648, 7, 0, 4294967291],
                                         "INTEGER", [-1, -2147483648, 7, 0, -5, 2147483647]),
    "TINYINT": ("TINYINT", [-128, -1, 0, 127, 5, 5], "TINYINT", [127, -128, 5, 6, -1]),
    "DATE": ("DATE", [_date(1), _date(5), _date(31), _date(5)], "DATE", [_date(5), _date(31), _date(2)]),
    "BOOLEAN": ("BOOLEAN", [True, False, True, None], "BOOLEAN", [True, None]),
    "DECIMAL(9,2)": ("DECIMAL(9,2)", [_dec(1250), _dec(5), _dec(999999999), _dec(1250), _dec(777)],
                     "DECIMAL(9,2)", [_dec(1250), _dec(500), _dec(999999999), _dec(5)]),
    "both ends of int64": ("BIGINT", [I64_MIN, I64_MAX, 0, -1, I64_MIN + 1, I64_MAX - 1, None],
                           "BIGINT", [I64_MAX, I64_MIN, 1]),
    "multiples of 2^32": ("BIGINT", [k << 32 for k in (-3, -1, 0, 1, 2, 5, 2**31 - 1)] + [1, (1 << 32) + 1],
                          "BIGINT", [k << 32 for k in (-3, 1, 3, 5, 2**31 - 1, -2**31)]),
    "SMALLINT with USMALLINT": ("SMALLINT", [-1, 32767, 0, -32768], "USMALLINT", [65535, 32767, 0]),
}


@pytest.mark.parametrize("case", list(KEY_CASES))
def test_key_types_cast_on_either_side(c, case):
    lt, lk, rt, rk = KEY_CASES[case]
    L = [(k, i) for i, k in enumerate(lk)]
    R = [(k, 100 + i) for i, k in enumerate(rk)]
    make(c, "kl", f"k {lt}, id BIGINT", L)
    make(c, "kr", f"k {rt}, id BIGINT", R)
    text = lambda r: _cell(r[0])  # keys are equal when their text is: one value, one spelling
    SL, SR = [text(r) for r in L], [text(r) for r in R]
    assert any(in3(x, SR) for x in SL) and any(in3(x, SR) is not True for x in SL), case
    check_both_places(c, "kl", L, "SELECT k FROM kr", SR, key=text)
    check_both_places(c, "kr", R, "SELECT k FROM kl", SL, key=text)


# ---- subquery shapes ----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def shapes(c):
    P = [(None if i == 4 else i * 50, i) for i in range(10)]
    D = [((i * 37) % 500, i % 7) for i in range(3000)]  # every key six times, more rows than the probe side
    E = [(k, 1000 + k) for k in (100, 150, 250, 777)]
    make(c, "hp", "k BIGINT, id BIGINT", P)
    make(c, "hd", "k BIGINT, g BIGINT", D)
    make(c, "he", "k BIGINT, w BIGINT", E)
    return P, D, E


def test_duplicates_and_a_set_larger_than_the_probe_side(c, shapes):
    P, D, E = shapes
    check_both_places(c, "hp", P, "SELECT k FROM hd", [r[0] for r in D])


def test_subquery_with_group_by_union_limit_and_join(c, shapes):
    P, D, E = shapes
    grouped = sorted({r[0] for r in D if r[1] < 3})
    check_both_places(c, "hp", P, "SELECT k FROM hd WHERE g < 3 GROUP BY k", grouped)
    check_both_places(c, "hp", P, "SELECT MAX(k) FROM hd GROUP BY g HAVING COUNT(*) > 1",
                      [max(r[0] for r in D if r[1] == g) for g in range(7)])
    check_both_places(c, "hp", P, "SELECT k FROM he UNION ALL SELECT k + 300 FROM he UNION ALL SELECT NULL",
                      [r[0] for r in E] + [r[0] + 300 for r in E] + [None])
    check_both_places(c, "hp", P, "SELECT k FROM hd ORDER BY k DESC, g LIMIT 13", sorted((r[0] for r in D), reverse=True)[:13])
    joined = [d[0] for d in D for e in E if d[0] == e[0] and d[1] > 2]
    check_both_places(c, "hp", P, "SELECT hd.k FROM hd JOIN he ON hd.k = he.k AND hd.g > 2", joined)
    nested = [e[0] for e in E if in3(e[0], [r[0] for r in D])]
    check_both_places(c, "hp", P, "SELECT k FROM he WHERE k IN (SELECT k FROM hd)", nested)


def test_probe_over_range_and_an_expression_on_the_left(c, shapes):
    P, D, E = shapes
    S = [r[0] for r in E]
    same(got(c, "SELECT range FROM range(300) WHERE range IN (SELECT k FROM he)"), [(k,) for k in range(300) if in3(k, S)])
    same(got(c, "SELECT range, range * 50 NOT IN (SELECT k FROM he) FROM range(7)"),
         [(k, not3(in3(k * 50, S))) for k in range(7)])
    check_both_places(c, "hp", P, "SELECT k FROM he", S, key=lambda r: None if r[0] is None else r[0] + 100, left="k + 100")


def test_one_row_select(c, shapes, nullm):
    assert got(c, "SELECT 100 IN (SELECT k FROM he), 101 IN (SELECT k FROM he), 101 NOT IN (SELECT k FROM he)") == \
        [("true", "false", "true")]
    assert got(c, "SELECT 2 IN (SELECT k FROM nn), 5 IN (SELECT k FROM nn), 2 NOT IN (SELECT k FROM nn)") == [(None, "true", None)]
    assert got(c, "SELECT CAST(NULL AS BIGINT) IN (SELECT k FROM he), CAST(NULL AS BIGINT) IN (SELECT k FROM ne), "
                  "3 NOT IN (SELECT k FROM ne)") == [(None, "false", "true")]


# ---- the leaf in other positions ----------------------------------------------------------------------
@pytest.fixture(scope="module")
def pos(c):
    T = [(None if i % 13 == 5 else i % 40, i, ["apple", "avocado", "banana", None, "cherry"][i % 5], i % 6) for i in range(333)]
    fill(c, "ot", "k BIGINT, v BIGINT, s VARCHAR, g BIGINT", T)
    S = [3, 8, 8, 21, 39, 500]
    SN = S + [None]
    make(c, "os", "k BIGINT", [(k,) for k in S])
    make(c, "osn", "k BIGINT", [(k,) for k in SN])
    B = [(k, 10 * k) for k in range(0, 40, 3)]
    make(c, "ob", "k BIGINT, w BIGINT", B)
    return T, S, SN, B


def test_under_or_with_a_varchar_like(c, pos):
    T, S, SN, B = pos
    like = lambda s: None if s is None else s.startswith("a")
    or3 = lambda a, b: True if a is True or b is True else (None if a is None or b is None else False)
    same(got(c, "SELECT v FROM ot WHERE k IN (SELECT k FROM osn) OR s LIKE 'a%'"),
         [(r[1],) for r in T if or3(in3(r[0], SN), like(r[2])) is True])
    same(got(c, "SELECT v, k NOT IN (SELECT k FROM osn) OR s LIKE 'a%' FROM ot"),
         [(r[1], or3(not3(in3(r[0], SN)), like(r[2]))) for r in T])
    names = kernels(c)
    assert "str_match" in names and "join_probe_mark" in names


def test_as_a_group_by_key(c, pos):
    T, S, SN, B = pos
    for tab, X in (("os", S), ("osn", SN)):
        want = {}
        for r in T:
            m = in3(r[0], X)
            cnt, tot = want.get(m, (0, 0))
            want[m] = (cnt + 1, tot + r[1])
        same(got(c, f"SELECT k IN (SELECT k FROM {tab}) AS m, COUNT(*), SUM(v) FROM ot GROUP BY k IN (SELECT k FROM {tab})"),
             [(m, n, t) for m, (n, t) in want.items()])


def test_inside_sum_case(c, pos):
    T, S, SN, B = pos
    assert one(c, "SELECT SUM(CASE WHEN k IN (SELECT k FROM os) THEN v END), SUM(CASE WHEN k NOT IN (SELECT k FROM os) THEN 1 "
                  "ELSE 0 END), COUNT(*) FROM ot WHERE g < 5") == \
        [str(sum(r[1] for r in T if r[3] < 5 and in3(r[0], S) is True)),
         str(sum(1 for r in T if r[3] < 5 and in3(r[0], S) is False)), str(sum(1 for r in T if r[3] < 5))]
    same(got(c, "SELECT g, SUM(CASE WHEN k IN (SELECT k FROM osn) THEN v ELSE -1 END) FROM ot GROUP BY g"),
         [(g, sum(r[1] if in3(r[0], SN) is True else -1 for r in T if r[3] == g)) for g in range(6)])


def test_in_having(c, pos):
    T, S, SN, B = pos
    groups = {}
    for r in T:
        if r[0] is not None:
            groups.setdefault(r[0], []).append(r[1])
    same(got(c, "SELECT k, COUNT(*) FROM ot WHERE k IS NOT NULL GROUP BY k HAVING k IN (SELECT k FROM os)"),
         [(k, len(v)) for k, v in groups.items() if in3(k, S) is True])
    same(got(c, "SELECT g, MIN(v) FROM ot GROUP BY g HAVING MIN(v) NOT IN (SELECT k FROM os)"),
         [(g, mn) for g in range(6) for mn in [min(r[1] for r in T if r[3] == g)] if not3(in3(mn, S)) is True])


def test_in_a_join_on_residual(c, pos):
    T, S, SN, B = pos
    want = [tuple(t) + tuple(b) for t in T for b in B if t[0] is not None and t[0] == b[0] and in3(t[3], S) is True]
    same(got(c, "SELECT * FROM ot JOIN ob ON ot.k = ob.k AND ot.g IN (SELECT k FROM os)"), want)
    want = [(t[1], b[1]) for t in T for b in B if t[0] is not None and t[0] == b[0] and not3(in3(b[1] // 10, S)) is True]
    assert want
    same(got(c, "SELECT ot.v, ob.w FROM ot JOIN ob ON ot.k = ob.k AND ob.w // 10 NOT IN (SELECT k FROM os)"), want)


def test_global_aggregate_over_a_join_takes_the_materialising_path(c, pos, mbx):
    T, S, SN, B = pos
    sql = "SELECT COUNT(*), SUM(ot.v + ob.w) FROM ot JOIN ob ON ot.k = ob.k WHERE ot.g IN (SELECT k FROM os) OR ob.w = 30"
    pairs = [(t, b) for t in T for b in B if t[0] is not None and t[0] == b[0] and (in3(t[3], S) is True or b[1] == 30)]
    want = [str(len(pairs)), str(sum(t[1] + b[1] for t, b in pairs))]
    assert one(c, sql) == want
    names = kernels(c)
    assert "join_probe_agg" not in names and "join_probe_mark" in names and "join_expand" in names
    # without the leaf the same statement is fused: the decline is the leaf's
    q(c, "SELECT COUNT(*), SUM(ot.v + ob.w) FROM ot JOIN ob ON ot.k = ob.k WHERE ot.g = 3 OR ob.w = 30")
    assert "join_probe_agg" in kernels(c)
    cfg = mbx.Config.create()
    assert isinstance(cfg.set("mbx_join_agg", "false"), mbx.Ok)
    plain = mbx.connect_with_config(cfg).value
    make(plain, "ot", "k BIGINT, v BIGINT, g BIGINT", [(r[0], r[1], r[3]) for r in T])
    make(plain, "ob", "k BIGINT, w BIGINT", B)
    make(plain, "os", "k BIGINT", [(k,) for k in S])
    assert one(plain, sql) == want
    plain.close()


# ---- one set per statement, prepared statements, CTAS, refusals ---------------------------------------
def test_identical_leaves_share_one_build_and_one_probe(c, pos):
    T, S, SN, B = pos
    n = sum(1 for r in T if in3(r[0], S) is True and (r[1] > 100 or in3(r[0], S) is True))
    assert one(c, "SELECT COUNT(*) FROM ot WHERE k IN (SELECT k FROM os) AND (v > 100 OR k IN (SELECT k FROM os))") == [str(n)]
    names = kernels(c)
    assert names.count("join_build") == 1 and names.count("join_probe_mark") == 1, names
    # lowered in two places (the aggregation and the HAVING): still one subquery run and one table
    groups = {}
    for r in T:
        groups.setdefault(in3(r[0], S), []).append(r[0])
    same(got(c, "SELECT k IN (SELECT k FROM os) AS m, COUNT(*) FROM ot GROUP BY k IN (SELECT k FROM os) "
                "HAVING MAX(k) IN (SELECT k FROM os)"),
         [(m, len(v)) for m, v in groups.items() if in3(max((x for x in v if x is not None), default=None), S) is True])
    names = kernels(c)
    assert names.count("join_build") == 1 and names.count("join_probe_mark") == 2, names
    # another subquery is another set
    q(c, "SELECT COUNT(*) FROM ot WHERE k IN (SELECT k FROM os) AND g IN (SELECT k FROM osn)")
    names = kernels(c)
    assert names.count("join_build") == 2 and names.count("join_probe_mark") == 2, names


def test_prepared_statement_with_three_parameter_values(c, pos):
    T, S, SN, B = pos
    st = c.prepare("SELECT COUNT(*), SUM(v) FROM ot WHERE k NOT IN (SELECT k FROM os WHERE k > ?) AND v >= ?").value
    for lo, vmin in ((0, 0), (8, 100), (1000, 7)):
        st.bind_bigint(1, lo)
        st.bind_bigint(2, vmin)
        X = [k for k in S if k > lo]
        keep = [r for r in T if not3(in3(r[0], X)) is True and r[1] >= vmin]
        assert st.execute().value.rows == [[str(len(keep)), str(sum(r[1] for r in keep))]], (lo, vmin)
    assert st.plan_stats() == {"binds": 1, "reuses": 2}
    st.close()


def test_ctas_and_insert_select(c, pos):
    T, S, SN, B = pos
    q(c, "DROP TABLE IF EXISTS oc")
    q(c, "CREATE TABLE oc AS SELECT v, k IN (SELECT k FROM osn) AS m FROM ot WHERE g NOT IN (SELECT k FROM os)")
    want = [(r[1], in3(r[0], SN)) for r in T if not3(in3(r[3], S)) is True]
    same(got(c, "SELECT * FROM oc"), want)
    q(c, "INSERT INTO oc SELECT v, true FROM ot WHERE k IN (SELECT k FROM os)")
    assert one(c, "SELECT COUNT(*) FROM oc") == [str(len(want) + sum(1 for r in T if in3(r[0], S) is True))]


def test_sharded_tables_are_refused_by_name(mbx):
    cfg = mbx.Config.create()
    assert isinstance(cfg.set("gpu_devices", "0,0"), mbx.Ok)
    conn = mbx.connect_with_config(cfg).value
    make(conn, "ha", "k BIGINT, v BIGINT", [(i, i) for i in range(10)])
    make(conn, "hb", "k BIGINT, w BIGINT", [(i, i) for i in range(10)])
    r = conn.query("SELECT * FROM range(5) WHERE range IN (SELECT k FROM hb)")
    assert isinstance(r, mbx.Err)
    assert r.error.message.startswith("Not implemented Error: IN (subquery) over table \"hb\", which is sharded by gpu_devices")
    r = conn.query("SELECT * FROM ha WHERE k NOT IN (SELECT range FROM range(5))")
    assert isinstance(r, mbx.Err)
    assert r.error.message.startswith("Not implemented Error: IN (subquery) over table \"ha\", which is sharded by gpu_devices")
    assert one(conn, "SELECT COUNT(*), SUM(v) FROM ha") == ["10", "45"]
    conn.close()


# ---- more than one sweep of the grid ------------------------------------------------------------------
def _i64(buf, n):
    assert len(buf) >= 4 + 8 * n and int.from_bytes(buf[:4], "little") == n, (len(buf), n)
    return np.frombuffer(buf, dtype="<i8", count=n, offset=4)


def test_large_probe_against_100003_keys(c, oracle):
    n, nd = 1_200_003, 100_003
    q(c, f"CREATE TABLE lf AS SELECT mbx_synth(5, i, 150000) AS k, i AS id FROM range({n}) tbl(i)")
    q(c, f"CREATE TABLE ld AS SELECT i AS k FROM range({nd}) tbl(i)")
    fk = oracle.synth_i64(n, 5, 0, 150000, 0)
    hit = np.isin(fk, np.arange(nd))
    assert 0 < int(hit.sum()) < n
    assert one(c, "SELECT COUNT(*) FROM lf WHERE k IN (SELECT k FROM ld)") == [str(int(hit.sum()))]
    assert one(c, "SELECT COUNT(*) FROM lf WHERE k NOT IN (SELECT k FROM ld)") == [str(int((~hit).sum()))]
    for op, mask in (("IN", hit), ("NOT IN", ~hit)):
        a = c.query_arrow(f"SELECT id FROM lf WHERE k {op} (SELECT k FROM ld)").value
        m = int(mask.sum())
        assert a.row_count() == m
        ids = _i64(a._buf("int64", 0), m)
        a.close()
        assert np.array_equal(np.sort(ids), np.nonzero(mask)[0])
