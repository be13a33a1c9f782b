"""Inner equi-joins on the device (csrc/join.cpp, join_kernels.hip): the
smaller input is sorted and hashed (join_build), the other one probes
(join_probe_count, join_expand), GatherRel fetches the columns of both sides
and the ON clause's other conjuncts filter the pairs.

The model is a plain Python dict join (numpy for the large cases).  Rows are
compared as sorted multisets unless the statement has ORDER BY, every value
exactly, as the text the library prints (NULL cells as None).  Small typed
tables come from INSERT ... VALUES, VARCHAR tables from the row appender
(gpu_tables.fill), large ones from CTAS over range() with mbx_synth."""
from collections import defaultdict

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


class Lit(str):
    """SQL text used as it stands (DATE '...', a DECIMAL or HUGEINT literal)
    whose result cell is `cell`"""
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
    """table `name` from Python rows through INSERT ... VALUES"""
    q(c, f"DROP TABLE IF EXISTS {name}")
    q(c, f"CREATE TABLE {name} ({cols})")
    for at in range(0, len(rows), 400):
        q(c, f"INSERT INTO {name} VALUES " + ", ".join("(" + ", ".join(_sql(v) for v in r) + ")" for r in rows[at:at + 400]))


def got(c, sql):
    """the statement's rows as tuples of text, None for NULL"""
    res = q(c, sql)
    return [tuple(None if res.nulls[i][j] else res.rows[i][j] for j in range(len(res.rows[i]))) for i in range(len(res.rows))]


def pyjoin(left, right, lk, rk, residual=None):
    """inner join of two row lists on lk(l) == rk(r); NULL keys match nothing"""
    idx = defaultdict(list)
    for r in right:
        if rk(r) is not None:
            idx[rk(r)].append(r)
    out = []
    for l in left:
        if lk(l) is None:
            continue
        for r in idx.get(lk(l), []):
            if residual is None or residual(l, r):
                out.append(tuple(l) + tuple(r))
    return out


def cells(rows):
    return [tuple(_cell(v) for v in r) for r in rows]


def same(got_rows, want_rows):
    key = lambda r: tuple((x is None, x or "") for x in r)
    assert sorted(got_rows, key=key) == sorted(cells(want_rows), key=key)


def _i64(buf, n):
    assert len(buf) >= 4 + 8 * n and int.from_bytes(buf[:4], "little") == n, (len(buf), n)
    return np.frombuffer(buf, dtype="<i8", count=n, offset=4)


K0 = lambda r: r[0]


# ---- sizes ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nl, nr", [(0, 5), (5, 0), (0, 0), (1, 1), (3, 4)])
def test_small_and_empty_inputs(c, nl, nr):
    L = [(i, 10 * i) for i in range(nl)]
    R = [(i, f"r{i}") for i in range(nr)]
    make(c, "sl", "k BIGINT, v BIGINT", L)
    make(c, "sr", "k BIGINT, s VARCHAR", R)
    same(got(c, "SELECT * FROM sl JOIN sr ON sl.k = sr.k"), pyjoin(L, R, K0, K0))
    assert one(c, "SELECT COUNT(*) FROM sl JOIN sr ON sl.k = sr.k") == [str(min(nl, nr))]


def test_no_key_in_common(c):
    L = [(i, i) for i in range(0, 200, 2)]
    R = [(i, i) for i in range(1, 301, 2)]
    make(c, "el", "k BIGINT, v BIGINT", L)
    make(c, "er", "k BIGINT, w BIGINT", R)
    assert got(c, "SELECT * FROM el JOIN er ON el.k = er.k") == []
    assert one(c, "SELECT COUNT(*), SUM(el.v) FROM el JOIN er ON el.k = er.k") == ["0", ""]


def test_unique_keys_one_to_one_70001(c):
    # more than 65 536 rows, several workgroups, a ragged last wave; an equal
    # row count on both sides builds the right one
    n = 70001
    q(c, f"CREATE TABLE u1 AS SELECT i AS k, i * 3 AS v FROM range({n}) tbl(i)")
    q(c, f"CREATE TABLE u2 AS SELECT (i * 7919) % {n} AS k, i AS w FROM range({n}) tbl(i)")
    a = c.query_arrow("SELECT u1.k, u1.v, u2.w, u2.k FROM u1 JOIN u2 ON u1.k = u2.k").value
    assert a.row_count() == n
    k, v, w, k2 = (_i64(a._buf("int64", j), n) for j in range(4))
    a.close()
    assert np.array_equal(k, k2) and np.array_equal(np.sort(k), np.arange(n)) and np.array_equal(v, 3 * k)
    assert np.array_equal((w * 7919) % n, k)
    assert {"join_build", "join_probe_count", "join_expand"} <= set(kernels(c))


def test_large_probe_against_100003_keys(c, oracle):
    n, nd = 1_200_003, 100_003
    q(c, f"CREATE TABLE f AS SELECT mbx_synth(5, i, 150000) AS k, mbx_synth(6, i, 1000) AS v FROM range({n}) tbl(i)")
    q(c, f"CREATE TABLE d AS SELECT i AS k, i * 2 + 1 AS w FROM range({nd}) tbl(i)")
    fk, fv = oracle.synth_i64(n, 5, 0, 150000, 0), oracle.synth_i64(n, 6, 0, 1000, 0)
    hit = fk < nd
    want = [str(int(hit.sum())), str(int((fv[hit] + 2 * fk[hit] + 1).sum()))]
    assert one(c, "SELECT COUNT(*), SUM(f.v + d.w) FROM f JOIN d ON f.k = d.k") == want
    assert one(c, "SELECT COUNT(*), SUM(f.v + d.w) FROM d JOIN f ON d.k = f.k") == want


# ---- duplicates -------------------------------------------------------------------------------------
def test_duplicate_keys_on_both_sides(c):
    B = [(k, 100 * k + j) for k in range(70) for j in range(k % 7)]
    P = [(k, -(10 * k + j)) for k in range(70) for j in range(k % 5)] + [(k, 0) for k in range(70, 700)]
    make(c, "db", "k BIGINT, b BIGINT", B)
    make(c, "dp", "k BIGINT, p BIGINT", P)
    assert len(B) < len(P)
    same(got(c, "SELECT * FROM dp JOIN db ON dp.k = db.k"), pyjoin(P, B, K0, K0))


def test_long_run_and_the_output_order(c):
    # one key with 70 000 build rows, hit by 3 of 80 000 probe rows: 210 000
    # pairs, probe-row-major, build rows ascending -- without ORDER BY
    q(c, "CREATE TABLE rp AS SELECT CASE WHEN i IN (10, 40000, 79999) THEN 42 ELSE -i - 1 END AS k, i AS id "
         "FROM range(80000) tbl(i)")
    q(c, "CREATE TABLE rb AS SELECT CASE WHEN i % 14001 = 14000 THEN 7 ELSE 42 END AS k, i AS id FROM range(70005) tbl(i)")
    bid = np.array([i for i in range(70005) if i % 14001 != 14000], dtype=np.int64)
    assert bid.size == 70000
    for sql in ("SELECT rp.id, rb.id FROM rp JOIN rb ON rp.k = rb.k", "SELECT rp.id, rb.id FROM rb JOIN rp ON rp.k = rb.k"):
        a = c.query_arrow(sql).value
        assert a.row_count() == 210000
        pid, gid = _i64(a._buf("int64", 0), 210000), _i64(a._buf("int64", 1), 210000)
        a.close()
        assert np.array_equal(pid, np.repeat(np.array([10, 40000, 79999]), 70000))
        assert np.array_equal(gid, np.tile(bid, 3))


def test_either_side_may_be_the_build_side(c):
    big = [(i % 97, i) for i in range(5000)]
    small = [(k, f"s{k}") for k in range(0, 120, 3)] + [(3, "again")]
    make(c, "bb", "k BIGINT, id BIGINT", big)
    fill(c, "bs", "k BIGINT, s VARCHAR", small)
    want = pyjoin(big, small, K0, K0)
    same(got(c, "SELECT * FROM bb JOIN bs ON bb.k = bs.k"), want)
    same(got(c, "SELECT * FROM bs JOIN bb ON bb.k = bs.k"), [r[2:] + r[:2] for r in want])


# ---- NULL keys --------------------------------------------------------------------------------------
@pytest.mark.parametrize("null_left, null_right", [(True, False), (False, True), (True, True)])
def test_null_keys_match_nothing(c, null_left, null_right):
    L = [(None if null_left and i % 3 == 0 else i % 10, i) for i in range(40)]
    R = [(None if null_right and i % 4 == 1 else i % 12, 100 + i) for i in range(25)]
    make(c, "nl", "k BIGINT, v BIGINT", L)
    make(c, "nr", "k BIGINT, w BIGINT", R)
    want = pyjoin(L, R, K0, K0)
    assert all(r[0] is not None and r[2] is not None for r in want)
    same(got(c, "SELECT * FROM nl JOIN nr ON nl.k = nr.k"), want)
    same(got(c, "SELECT * FROM nr JOIN nl ON nl.k = nr.k"), [r[2:] + r[:2] for r in want])
    # an expression over a NULL key is NULL too
    same(got(c, "SELECT * FROM nl JOIN nr ON nl.k + 1 = nr.k"),
         pyjoin(L, R, lambda r: None if r[0] is None else r[0] + 1, K0))


# ---- key types --------------------------------------------------------------------------------------
def _date(d):
    return Lit(f"DATE '2024-01-{d:02d}'", f"2024-01-{d:02d}")


def _dec(cents):
    t = f"{cents // 100}.{cents % 100:02d}"
    return Lit(t, t)


KEY_CASES = {
    "negative INTEGER with BIGINT": ("INTEGER", [-5, -1, 0, 3, -2147483648, 2147483647],
                                     "BIGINT", [-1, -5, 3, 4294967295, -2147483648, 2147483648, 2147483647]),
    "UINTEGER above 2^31 with INTEGER": ("UINTEGER", [4294967295, 2147483648, 7, 0, 4294967291],
                                         "INTEGER", [-1, -2147483648, 7, 0, -5, 2147483647]),
    "TINYINT": ("TINYINT", [-128, -1, 0, 127, 5, 5], "TINYINT", [127, -128, 5, 6, -1]),
    "DATE": ("DATE", [_date(1), _date(5), _date(31), _date(5)], "DATE", [_date(5), _date(31), _date(2)]),
    "BOOLEAN": ("BOOLEAN", [True, False, True, None], "BOOLEAN", [False, True, None]),
    "DECIMAL(9,2)": ("DECIMAL(9,2)", [_dec(1250), _dec(5), _dec(999999999), _dec(1250)],
                     "DECIMAL(9,2)", [_dec(1250), _dec(500), _dec(999999999), _dec(5)]),
}


@pytest.mark.parametrize("case", list(KEY_CASES))
def test_key_types(c, case):
    lt, lk, rt, rk = KEY_CASES[case]
    L = [(k, i) for i, k in enumerate(lk)]
    R = [(k, 100 + i) for i, k in enumerate(rk)]
    make(c, "kl", f"k {lt}, v BIGINT", L)
    make(c, "kr", f"k {rt}, w BIGINT", R)
    model = lambda r: None if r[0] is None else _cell(r[0])  # keys are equal when their text is: one value, one spelling
    want = pyjoin(L, R, model, model)
    assert want, case
    same(got(c, "SELECT * FROM kl JOIN kr ON kl.k = kr.k"), want)


def test_expression_key_and_range_input(c):
    T = [(k, 7 * k) for k in (0, 2, 3, 3, 9, 11, -1)]
    make(c, "xt", "k BIGINT, v BIGINT", T)
    R = [(i,) for i in range(10)]
    same(got(c, "SELECT * FROM range(10) r JOIN xt t ON r.range = t.k"), pyjoin(R, T, K0, K0))
    same(got(c, "SELECT * FROM xt t JOIN range(10) r ON r.range = t.k"), pyjoin(T, R, K0, K0))
    same(got(c, "SELECT * FROM range(10) r JOIN xt t ON r.range * 2 = t.k + 1"),
         pyjoin(R, T, lambda r: 2 * r[0], lambda r: r[0] + 1))
    G = [(i,) for i in range(2, 13, 3)]
    same(got(c, "SELECT * FROM generate_series(2, 12, 3) g JOIN xt t ON t.k = g.generate_series"), pyjoin(G, T, K0, K0))


# ---- payload columns through the gather -------------------------------------------------------------
HUGE = [Lit(t, t) for t in ("170141183460469231731687303715884105727", "-170141183460469231731687303715884105727", "0")]
DEC38 = [Lit(t, t) for t in ("123456789012345678901234567890123456.78", "-0.01", "99999999999999999999999999999999999.99")]


def test_payload_columns_of_every_storage(c):
    L = [(i % 6, ["", "abc", None, "a longer string, to be sure", "é"][i % 5], [0.5, -2.25, 1234.125][i % 3],
          None if i % 4 == 0 else i * 1000003) for i in range(23)]
    R = [(i % 8, HUGE[i % 3], None if i % 5 == 2 else DEC38[i % 3], ["", None, "right"][i % 3]) for i in range(17)]
    make(c, "pl", "k BIGINT, s VARCHAR, d DOUBLE, nb BIGINT", L)
    make(c, "pr", "k BIGINT, h HUGEINT, m DECIMAL(38,2), t VARCHAR", R)
    want = pyjoin(L, R, K0, K0)
    same(got(c, "SELECT * FROM pl JOIN pr ON pl.k = pr.k"), want)
    same(got(c, "SELECT pr.t, pl.s, pr.m, pl.nb, pr.h, pl.d FROM pr JOIN pl ON pl.k = pr.k"),
         [(r[7], r[1], r[6], r[3], r[5], r[2]) for r in want])


# ---- residuals --------------------------------------------------------------------------------------
def test_residuals(c):
    A = [(i % 5, i % 3, i) for i in range(60)]
    B = [(i % 7, i % 2, 2 * i) for i in range(35)]
    make(c, "ra", "k BIGINT, k2 BIGINT, v BIGINT", A)
    make(c, "rbb", "k BIGINT, k2 BIGINT, w BIGINT", B)
    same(got(c, "SELECT * FROM ra a JOIN rbb b ON a.k = b.k AND a.k2 = b.k2"),
         pyjoin(A, B, K0, K0, lambda l, r: l[1] == r[1]))
    same(got(c, "SELECT * FROM ra a JOIN rbb b ON a.k = b.k AND a.v < b.w"), pyjoin(A, B, K0, K0, lambda l, r: l[2] < r[2]))
    same(got(c, "SELECT * FROM ra a JOIN rbb b ON a.v < b.w AND b.k = a.k AND a.k2 <> b.k2"),
         pyjoin(A, B, K0, K0, lambda l, r: l[2] < r[2] and l[1] != r[1]))
    assert got(c, "SELECT * FROM ra a JOIN rbb b ON a.k = b.k AND a.v > 1000") == []
    assert one(c, "SELECT COUNT(*) FROM ra a JOIN rbb b ON a.k = b.k AND a.v + b.w < 0") == ["0"]


# ---- composition ------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def star(c):
    """a fact table and two dimensions"""
    F = [(i, i % 11, i % 4, (i * 37) % 101 - 50) for i in range(300)]
    D = [(k, ["red", "green", "", None, "blue"][k % 5]) for k in range(9)]  # keys 9, 10 of f.a have no row
    E = [(k, 1000 * k) for k in (0, 1, 3)]
    make(c, "sf", "id BIGINT, a BIGINT, b BIGINT, v BIGINT", F)
    fill(c, "sd", "k BIGINT, name VARCHAR", D)
    make(c, "se", "k BIGINT, bonus BIGINT", E)
    return F, D, E


def test_three_table_chain(c, star):
    F, D, E = star
    fd = pyjoin(F, D, lambda r: r[1], K0)
    same(got(c, "SELECT * FROM sf JOIN sd ON sf.a = sd.k JOIN se ON se.k = sf.b"), pyjoin(fd, E, lambda r: r[2], K0))
    same(got(c, "SELECT x.id, y.id FROM sf x JOIN sf y ON x.v = y.v JOIN se ON se.k = y.b AND x.id < y.id"),
         [(r[0], r[4]) for r in pyjoin(pyjoin(F, F, lambda r: r[3], lambda r: r[3]), E, lambda r: r[6], K0,
                                       lambda l, r: l[0] < l[4])])


def test_subquery_and_values_inputs(c, star):
    F, D, E = star
    V = [(1, "one"), (3, "three"), (8, "eight")]
    sub = [(r[0], r[1] + 1) for r in F if r[3] > 0]
    same(got(c, "SELECT * FROM (SELECT id, a + 1 AS a1 FROM sf WHERE v > 0) q JOIN (VALUES (1, 'one'), (3, 'three'), (8, 'eight')) "
                "t(k, s) ON q.a1 = t.k"), pyjoin(sub, V, lambda r: r[1], K0))
    agg = defaultdict(int)
    for r in F:
        agg[r[1]] += r[3]
    same(got(c, "SELECT sd.name, g.t FROM (SELECT a, SUM(v) AS t FROM sf GROUP BY a) g JOIN sd ON g.a = sd.k"),
         [(r[3], r[1]) for r in pyjoin(sorted(agg.items()), D, K0, K0)])


def test_where_over_both_sides(c, star):
    F, D, E = star
    want = [r for r in pyjoin(F, D, lambda r: r[1], K0) if r[3] > 10 and r[5] is not None and r[5] != "red"]
    same(got(c, "SELECT * FROM sf JOIN sd ON sf.a = sd.k WHERE sf.v > 10 AND sd.name <> 'red'"), want)


def test_group_by_right_varchar_sum_left(c, star):
    F, D, E = star
    agg = defaultdict(lambda: [0, 0])
    for r in pyjoin(F, D, lambda r: r[1], K0):
        agg[r[5]][0] += r[3]
        agg[r[5]][1] += 1
    same(got(c, "SELECT sd.name, SUM(sf.v), COUNT(*) FROM sf JOIN sd ON sf.a = sd.k GROUP BY sd.name"),
         [(k, s, n) for k, (s, n) in agg.items()])


def test_order_by_limit_offset(c, star):
    F, D, E = star
    want = sorted(((r[3], r[0], r[5]) for r in pyjoin(F, D, lambda r: r[1], K0)), key=lambda r: (-r[0], r[1]))
    assert got(c, "SELECT sf.v, sf.id, sd.name FROM sf JOIN sd ON sf.a = sd.k ORDER BY sf.v DESC, sf.id LIMIT 17 OFFSET 5") == \
        cells(want[5:22])


def test_union_all_of_two_joins(c, star):
    F, D, E = star
    want = [(r[0], r[4], r[5]) for r in pyjoin(F, D, lambda r: r[1], K0)] + \
           [(r[0], r[5], "bonus") for r in pyjoin(F, E, lambda r: r[2], K0)]
    same(got(c, "SELECT sf.id, sd.k, sd.name FROM sf JOIN sd ON sf.a = sd.k UNION ALL "
                "SELECT sf.id, se.bonus, 'bonus' FROM sf JOIN se ON sf.b = se.k"), want)


def test_ctas_from_a_join(c, star):
    F, D, E = star
    q(c, "DROP TABLE IF EXISTS sj")
    q(c, "CREATE TABLE sj AS SELECT sf.id, sd.name, sf.v + se.bonus AS total FROM sf JOIN sd ON sf.a = sd.k JOIN se ON sf.b = se.k")
    want = [(r[0], r[5], r[3] + r[7]) for r in pyjoin(pyjoin(F, D, lambda r: r[1], K0), E, lambda r: r[2], K0)]
    same(got(c, "SELECT * FROM sj"), want)
    assert one(c, "SELECT COUNT(*), SUM(total) FROM sj WHERE name = 'green'") == \
        [str(sum(1 for r in want if r[1] == "green")), str(sum(r[2] for r in want if r[1] == "green"))]
    q(c, "INSERT INTO sj SELECT sf.id, sd.name, 0 FROM sf JOIN sd ON sf.a = sd.k WHERE sf.id < 5")
    assert one(c, "SELECT COUNT(*) FROM sj") == [str(len(want) + 5)]


def test_query_arrow_of_a_join(c, star):
    F, D, E = star
    want = sorted((r[0], r[3], r[5]) for r in pyjoin(F, E, lambda r: r[2], K0))
    a = c.query_arrow("SELECT sf.id, sf.v, se.bonus FROM sf JOIN se ON sf.b = se.k ORDER BY sf.id").value
    n = a.row_count()
    assert n == len(want)
    cols = [_i64(a._buf("int64", j), n).tolist() for j in range(3)]
    a.close()
    assert list(zip(*cols)) == want


def test_prepared_join_patches_its_constants(c, star):
    F, D, E = star
    st = c.prepare("SELECT COUNT(*), SUM(se.bonus) FROM sf JOIN se ON sf.b = se.k + ? WHERE sf.v > ?").value
    for add, lo in ((0, -100), (1, 0), (-1, 20)):
        st.bind_bigint(1, add)
        st.bind_bigint(2, lo)
        want = [r for r in pyjoin(F, E, lambda r: r[2], lambda r: r[0] + add) if r[3] > lo]
        assert want, (add, lo)
        assert st.execute().value.rows == [[str(len(want)), str(sum(r[5] for r in want))]], (add, lo)
    assert st.plan_stats() == {"binds": 1, "reuses": 2}
    st.close()


# ---- limits, refusals, the profile ------------------------------------------------------------------
def test_join_max_rows(mbx):
    cfg = mbx.Config.create()
    assert isinstance(cfg.set("mbx_join_max_rows", "1000"), mbx.Ok)
    conn = mbx.connect_with_config(cfg).value
    make(conn, "ml", "k BIGINT, v BIGINT", [(0, i) for i in range(91)])
    make(conn, "mr", "k BIGINT, w BIGINT", [(0, i) for i in range(11)] + [(1, 0)])
    r = conn.query("SELECT * FROM ml JOIN mr ON ml.k = mr.k")  # 91 x 11 = 1 001 rows
    assert isinstance(r, mbx.Err)
    assert r.error.message == "Out of Range Error: join produces 1001 rows, more than mbx_join_max_rows"
    # the next statement is clean, and a join at the limit runs
    assert one(conn, "SELECT COUNT(*) FROM ml") == ["91"]
    assert one(conn, "SELECT COUNT(*) FROM ml JOIN (SELECT * FROM mr WHERE w < 10) m ON ml.k = m.k") == ["910"]
    # the limit is on the join's own pairs, whatever a residual or a WHERE would keep of them
    assert isinstance(conn.query("SELECT COUNT(*) FROM ml JOIN mr ON ml.k = mr.k AND ml.v < 0"), mbx.Err)
    assert one(conn, "SELECT COUNT(*) FROM mr") == ["12"]
    conn.close()


def test_sharded_tables_are_refused(mbx):
    cfg = mbx.Config.create()
    assert isinstance(cfg.set("gpu_devices", "0,0"), mbx.Ok)
    conn = mbx.connect_with_config(cfg).value
    make(conn, "ha", "k BIGINT, v BIGINT", [(i, i) for i in range(10)])
    make(conn, "hb", "k BIGINT, w BIGINT", [(i, i) for i in range(10)])
    r = conn.query("SELECT * FROM ha JOIN hb ON ha.k = hb.k")
    assert isinstance(r, mbx.Err)
    assert r.error.message.startswith("Not implemented Error: a join over table \"ha\", which is sharded by gpu_devices")
    assert one(conn, "SELECT COUNT(*), SUM(v) FROM ha") == ["10", "45"]
    conn.close()


def test_profile_names_the_three_kernels(c, star):
    q(c, "SELECT sf.id, sd.name FROM sf JOIN sd ON sf.a = sd.k")
    names = kernels(c)
    for k in ("join_build", "join_probe_count", "join_expand"):
        assert names.count(k) == 1, names
    assert names.index("join_build") < names.index("join_probe_count") < names.index("join_expand")
