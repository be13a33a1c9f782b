"""A global aggregate over an inner join, fused into the probe
(csrc/join.cpp JoinAggregate, join_kernels.hip join_probe_agg / join_agg_fold,
join_agg_plan.h): the pairs exist only in registers, and the residual, the WHERE
and the aggregate arguments are interpreted per pair.

Every statement runs on two profiled connections with tables of the same
contents: `fused` (mbx_join_agg=true, mbx_join_agg_max_run=8 unless a test sets
its own) and `plain` (mbx_join_agg=false), which materialises the pairs as
before.  Both must give the answer of the model, a Python dict join (numpy for
the large case); integers compare exactly, as the text the library prints.  The
profile says which path ran: join_probe_agg and join_agg_fold, or
join_probe_count, join_expand and join_gather."""
from collections import defaultdict
from decimal import Decimal

import numpy as np
import pytest

from conftest import q
from gpu_tables import fill, kernels

pytestmark = pytest.mark.gpu

FUSED = ("join_probe_agg", "join_agg_fold")
OLD = ("join_probe_count", "join_expand", "join_gather")
BIG = 2 ** 63 - 1


def connect(mbx, **opts):
    cfg = mbx.Config.create()
    for k, v in dict(mbx_profile="true", **opts).items():
        assert isinstance(cfg.set(k, str(v)), mbx.Ok), (k, v)
    r = mbx.connect_with_config(cfg)
    assert isinstance(r, mbx.Ok), r.error.message
    return r.value


class Pair:
    """the two connections; statements that load tables go to both"""
    def __init__(self, fused, plain):
        self.fused, self.plain = fused, plain

    def __iter__(self):
        return iter((self.fused, self.plain))

    def run(self, sql):
        for c in self:
            q(c, sql)

    def close(self):
        for c in self:
            c.close()


@pytest.fixture(scope="module")
def cc(mbx):
    p = Pair(connect(mbx, mbx_join_agg="true", mbx_join_agg_max_run=8), connect(mbx, mbx_join_agg="false"))
    yield p
    p.close()


def _sql(v):
    if v is None:
        return "NULL"
    if isinstance(v, str):  # SQL text as it stands (a DATE, DECIMAL or HUGEINT literal)
        return v
    return repr(v)


def make(conns, name, cols, rows):
    """table `name` from Python rows through INSERT ... VALUES, on every connection"""
    for c in conns:
        q(c, f"DROP TABLE IF EXISTS {name}")
        q(c, f"CREATE TABLE {name} ({cols})")
        for at in range(0, len(rows), 400):
            q(c, f"INSERT INTO {name} VALUES " + ", ".join("(" + ", ".join(_sql(v) for v in r) + ")" for r in rows[at:at + 400]))


def row(c, sql):
    """the statement's one row as text, None for NULL"""
    res = q(c, sql)
    assert res.row_count() == 1, (sql, res.rows)
    return [None if res.nulls[0][j] else res.rows[0][j] for j in range(len(res.rows[0]))]


def took_fused(c):
    names = kernels(c)
    return all(names.count(k) == 1 for k in FUSED) and names.count("join_build") >= 1 and not any(k in names for k in OLD)


def took_old(c):
    names = kernels(c)
    return "join_probe_count" in names and not any(k in names for k in FUSED)


def check(cc, sql, want, fused=True, nested=False):
    """the same answer on both connections; the fused one takes the fused path
    (or declines: fused=False), the plain one never does.  nested: an input of
    the join is itself a join, so the old kernels appear as well"""
    want = [None if w is None else str(w) for w in want]
    assert row(cc.fused, sql) == want, sql
    names = kernels(cc.fused)
    if fused and nested:
        assert all(names.count(k) == 1 for k in FUSED), (sql, names)
    elif fused:
        assert took_fused(cc.fused), (sql, names)
    else:
        assert took_old(cc.fused), (sql, names)
    assert row(cc.plain, sql) == want, sql
    assert not any(k in kernels(cc.plain) for k in FUSED), sql


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


K0 = lambda r: r[0]


def vals(rows, f):
    """f over the rows, without the NULLs"""
    return [x for x in (f(r) for r in rows) if x is not None]


def ssum(xs):
    return sum(xs) if xs else None


# ---- the path -----------------------------------------------------------------------------------------
def test_path(cc):
    A = [(i % 40, i) for i in range(300)]
    B = [(k, 1000 * k) for k in range(0, 60, 2)]
    make(cc, "pa", "k BIGINT, v BIGINT", A)
    make(cc, "pb", "k BIGINT, w BIGINT", B)
    J = pyjoin(A, B, K0, K0)
    sql = "SELECT COUNT(*), SUM(a.v + b.w) FROM pa a JOIN pb b ON a.k = b.k"
    want = [str(len(J)), str(sum(r[1] + r[3] for r in J))]
    assert row(cc.fused, sql) == want
    names = kernels(cc.fused)
    for k in ("join_build",) + FUSED:
        assert names.count(k) == 1, names
    assert not any(k in names for k in OLD), names
    assert names.index("join_build") < names.index("join_probe_agg") < names.index("join_agg_fold")
    assert row(cc.plain, sql) == want
    names = kernels(cc.plain)
    for k in OLD:
        assert names.count(k) == 1, names
    assert not any(k in names for k in FUSED), names
    # a select without aggregates and a GROUP BY over the join materialise on both
    for sql in ("SELECT a.v, b.w FROM pa a JOIN pb b ON a.k = b.k",
                "SELECT a.k, SUM(b.w) FROM pa a JOIN pb b ON a.k = b.k GROUP BY a.k"):
        for c in cc:
            assert q(c, sql).row_count() == (len(J) if "GROUP" not in sql else len({r[0] for r in J}))
            names = kernels(c)
            for k in OLD:
                assert names.count(k) == 1, (sql, names)
            assert not any(k in names for k in FUSED), (sql, names)


# ---- sizes --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 255, 256, 257, 70001])
def test_probe_rows_at_the_tile_edges(cc, n):
    # unique build keys; the probe side's keys 0 .. 129 meet keys 0 .. 99
    nd = 1 if n == 1 else 100
    for sql in ("DROP TABLE IF EXISTS zp", "DROP TABLE IF EXISTS zd",
                f"CREATE TABLE zp AS SELECT (i * 7) % 130 AS k, i * 3 - 1000 AS v FROM range({n}) tbl(i)",
                f"CREATE TABLE zd AS SELECT i AS k, i * 2 + 1 AS w FROM range({nd}) tbl(i)"):
        cc.run(sql)
    i = np.arange(n, dtype=np.int64)
    k, v = (i * 7) % 130, i * 3 - 1000
    hit = k < nd
    want = [int(hit.sum()), int((v[hit] + 2 * k[hit] + 1).sum()) if hit.any() else None, int(v[hit].min()) if hit.any() else None]
    check(cc, "SELECT COUNT(*), SUM(zp.v + zd.w), MIN(zp.v) FROM zp JOIN zd ON zp.k = zd.k", want)


def test_large_probe_against_100003_keys(cc, oracle):
    n, nd = 1_200_003, 100_003
    cc.run(f"CREATE TABLE f AS SELECT mbx_synth(5, i, 150000) AS k, mbx_synth(6, i, 1000) AS v FROM range({n}) tbl(i)")
    cc.run(f"CREATE TABLE d AS SELECT i AS k, i * 2 + 1 AS w FROM range({nd}) tbl(i)")
    fk, fv = oracle.synth_i64(n, 5, 0, 150000, 0), oracle.synth_i64(n, 6, 0, 1000, 0)
    hit = fk < nd
    want = [int(hit.sum()), int((fv[hit] + 2 * fk[hit] + 1).sum())]
    check(cc, "SELECT COUNT(*), SUM(f.v + d.w) FROM f JOIN d ON f.k = d.k", want)
    check(cc, "SELECT COUNT(*), SUM(f.v + d.w) FROM d JOIN f ON d.k = f.k", want)


# ---- runs ---------------------------------------------------------------------------------------------
def test_runs_of_0_to_6_and_the_run_limit(cc, mbx):
    B = [(k, 100 * k + j) for k in range(70) for j in range(k % 7)]
    P = [(k, -(10 * k + j)) for k in range(70) for j in range(k % 5)] + [(k, 0) for k in range(70, 700)]
    assert len(B) < len(P)
    tight = connect(mbx, mbx_join_agg="true", mbx_join_agg_max_run=4)
    exact = connect(mbx, mbx_join_agg="true", mbx_join_agg_max_run=6)
    make(list(cc) + [tight, exact], "db", "k BIGINT, b BIGINT", B)
    make(list(cc) + [tight, exact], "dp", "k BIGINT, p BIGINT", P)
    J = pyjoin(P, B, K0, K0)
    sql = "SELECT COUNT(*), SUM(dp.p * 1000 + db.b), MIN(db.b), MAX(dp.p), COUNT(db.b) FROM dp JOIN db ON dp.k = db.k"
    want = [len(J), sum(r[1] * 1000 + r[3] for r in J), min(r[3] for r in J), max(r[1] for r in J), len(J)]
    check(cc, sql, want)  # the longest run is 6, the limit 8
    want = [str(w) for w in want]
    assert row(exact, sql) == want and took_fused(exact), kernels(exact)  # a run as long as the limit is taken
    assert row(tight, sql) == want and took_old(tight), kernels(tight)    # one longer than the limit falls back
    tight.close()
    exact.close()


def test_a_run_of_70000_falls_back(cc):
    cc.run("CREATE TABLE rp AS SELECT CASE WHEN i IN (10, 40000, 79999) THEN 42 ELSE -i - 1 END AS k, i AS id "
           "FROM range(80000) tbl(i)")
    cc.run("CREATE TABLE rb AS SELECT CASE WHEN i % 14001 = 14000 THEN 7 ELSE 42 END AS k, i AS id FROM range(70005) tbl(i)")
    bid = sum(i for i in range(70005) if i % 14001 != 14000)
    want = [210000, 70000 * (10 + 40000 + 79999) + 3 * bid]
    check(cc, "SELECT COUNT(*), SUM(rp.id + rb.id) FROM rp JOIN rb ON rp.k = rb.k", want, fused=False)
    check(cc, "SELECT COUNT(*), SUM(rp.id + rb.id) FROM rb JOIN rp ON rp.k = rb.k", want, fused=False)


# ---- sides --------------------------------------------------------------------------------------------
def test_arguments_from_either_side_in_either_order(cc):
    big = [(i % 97, i - 2500) for i in range(5000)]
    small = [(k, k * k - 50) for k in range(0, 120, 3)]
    make(cc, "bb", "k BIGINT, x BIGINT", big)
    make(cc, "bs", "k BIGINT, y BIGINT", small)
    J = pyjoin(big, small, K0, K0)
    want = [len(J), sum(r[1] for r in J), sum(r[3] for r in J), sum(r[1] * r[3] for r in J), min(r[3] - r[1] for r in J)]
    aggs = "COUNT(*), SUM(bb.x), SUM(bs.y), SUM(bb.x * bs.y), MIN(bs.y - bb.x)"
    check(cc, f"SELECT {aggs} FROM bb JOIN bs ON bb.k = bs.k", want)  # the right input builds
    check(cc, f"SELECT {aggs} FROM bs JOIN bb ON bb.k = bs.k", want)  # the left one
    check(cc, "SELECT SUM(bb.x), MAX(bb.x) FROM bs JOIN bb ON bb.k = bs.k", [want[1], max(r[1] for r in J)])  # probe side only
    check(cc, "SELECT SUM(bs.y), MAX(bs.y) FROM bb JOIN bs ON bb.k = bs.k", [want[2], max(r[3] for r in J)])  # build side only


# ---- NULLs --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("null_left, null_right", [(True, False), (False, True), (True, True)])
def test_null_keys_and_nullable_arguments(cc, null_left, null_right):
    L = [(None if null_left and i % 3 == 0 else i % 10, None if i % 4 == 1 else i - 20) for i in range(40)]
    R = [(None if null_right and i % 4 == 1 else i % 12, None if i % 3 == 0 else 100 - 7 * i) for i in range(25)]
    make(cc, "nl", "k BIGINT, v BIGINT", L)
    make(cc, "nr", "k BIGINT, w BIGINT", R)
    J = pyjoin(L, R, K0, K0)
    assert J and any(r[1] is None for r in J) and any(r[3] is None for r in J)
    both = vals(J, lambda r: None if r[1] is None or r[3] is None else r[1] + r[3])
    v, w = vals(J, lambda r: r[1]), vals(J, lambda r: r[3])
    want = [len(J), len(v), len(w), sum(v), sum(both), min(w), max(v)]
    aggs = "COUNT(*), COUNT(nl.v), COUNT(nr.w), SUM(nl.v), SUM(nl.v + nr.w), MIN(nr.w), MAX(nl.v)"
    check(cc, f"SELECT {aggs} FROM nl JOIN nr ON nl.k = nr.k", want)
    check(cc, f"SELECT {aggs} FROM nr JOIN nl ON nl.k = nr.k", want)
    for c in cc:
        avg = row(c, "SELECT AVG(nr.w), AVG(nl.v + nr.w) FROM nl JOIN nr ON nl.k = nr.k")
        assert abs(float(avg[0]) - sum(w) / len(w)) <= 1e-9 * sum(abs(x) for x in w) / len(w)
        assert abs(float(avg[1]) - sum(both) / len(both)) <= 1e-9 * sum(abs(x) for x in both) / len(both)
    assert took_fused(cc.fused)


def test_an_argument_that_is_null_for_every_kept_pair(cc):
    L = [(i % 6, i) for i in range(30)]
    R = [(k, None if k < 4 else k) for k in range(6)]
    make(cc, "al", "k BIGINT, v BIGINT", L)
    make(cc, "ar", "k BIGINT, w BIGINT", R)
    kept = [r for r in pyjoin(L, R, K0, K0) if r[0] < 4]
    check(cc, "SELECT COUNT(*), COUNT(ar.w), SUM(ar.w), MIN(ar.w), AVG(ar.w), SUM(al.v + ar.w), SUM(al.v) "
              "FROM al JOIN ar ON al.k = ar.k WHERE al.k < 4", [len(kept), 0, None, None, None, None, sum(r[1] for r in kept)])


def test_no_key_in_common(cc):
    L = [(i, i) for i in range(0, 200, 2)]
    R = [(i, i) for i in range(1, 301, 2)]
    make(cc, "el", "k BIGINT, v BIGINT", L)
    make(cc, "er", "k BIGINT, w BIGINT", R)
    check(cc, "SELECT COUNT(*), SUM(el.v), MIN(er.w), COUNT(er.w) FROM el JOIN er ON el.k = er.k", [0, None, None, 0])
    # an empty input, and a build side that is empty once its NULL keys have left
    make(cc, "ee", "k BIGINT, w BIGINT", [])
    make(cc, "en", "k BIGINT, w BIGINT", [(None, 1), (None, 2)])
    for t in ("ee", "en"):
        for c in cc:
            assert row(c, f"SELECT COUNT(*), SUM(el.v + {t}.w) FROM el JOIN {t} ON el.k = {t}.k") == ["0", None]


# ---- stages -------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def stages(cc):
    A = [(i % 5, i % 3, i) for i in range(60)]
    B = [(i % 7, i % 2, 2 * i) for i in range(35)]
    make(cc, "ra", "k BIGINT, k2 BIGINT, v BIGINT", A)
    make(cc, "rbb", "k BIGINT, k2 BIGINT, w BIGINT", B)
    return A, B


def test_residual_and_where_together_and_apart(cc, stages):
    A, B = stages
    res = lambda l, r: l[2] < r[2] and l[1] != r[1]
    whr = lambda r: r[2] + r[5] > 30 and r[4] == 0
    aggs = "COUNT(*), SUM(a.v - b.w), MAX(b.w)"
    out = lambda J: [len(J), ssum([r[2] - r[5] for r in J]), max(r[5] for r in J) if J else None]
    J = pyjoin(A, B, K0, K0, res)
    check(cc, f"SELECT {aggs} FROM ra a JOIN rbb b ON a.k = b.k AND a.v < b.w AND a.k2 <> b.k2", out(J))
    check(cc, f"SELECT {aggs} FROM ra a JOIN rbb b ON a.k = b.k WHERE a.v + b.w > 30 AND b.k2 = 0",
          out([r for r in pyjoin(A, B, K0, K0) if whr(r)]))
    check(cc, f"SELECT {aggs} FROM ra a JOIN rbb b ON a.v < b.w AND b.k = a.k AND a.k2 <> b.k2 WHERE a.v + b.w > 30 AND b.k2 = 0",
          out([r for r in J if whr(r)]))
    check(cc, f"SELECT {aggs} FROM ra a JOIN rbb b ON a.k = b.k AND a.v + b.w < 0", [0, None, None])
    check(cc, f"SELECT {aggs} FROM ra a JOIN rbb b ON a.k = b.k WHERE a.v > 1000", [0, None, None])


def test_overflow_raises_only_for_kept_pairs(cc, mbx):
    L = [(0, BIG), (1, 5), (2, BIG - 1)]
    R = [(0, 1), (1, 6), (2, 1)]
    make(cc, "ol", "k BIGINT, v BIGINT", L)
    make(cc, "orr", "k BIGINT, w BIGINT", R)
    # the pair of key 0 overflows v + w; the residual, or the WHERE, rejects it
    check(cc, "SELECT COUNT(*), SUM(ol.v + orr.w) FROM ol JOIN orr ON ol.k = orr.k AND ol.k > 0", [2, 11 + BIG])
    check(cc, "SELECT COUNT(*), SUM(ol.v + orr.w) FROM ol JOIN orr ON ol.k = orr.k WHERE orr.k <> 0", [2, 11 + BIG])
    # kept, it raises: the same message on both connections, and the next statement is clean
    msgs = []
    for c in cc:
        r = c.query("SELECT COUNT(*), SUM(ol.v + orr.w) FROM ol JOIN orr ON ol.k = orr.k")
        assert isinstance(r, mbx.Err)
        msgs.append(r.error.message)
        assert row(c, "SELECT COUNT(*) FROM ol JOIN orr ON ol.k = orr.k") == ["3"]
    assert msgs[0] == msgs[1] == "Out of Range Error: Overflow in addition!"
    # INTEGER + INTEGER overflows at 32 bits
    make(cc, "il", "k INTEGER, v INTEGER", [(0, 2147483647), (1, 5)])
    make(cc, "ir", "k INTEGER, w INTEGER", [(0, 1), (1, 6)])
    msgs = []
    for c in cc:
        r = c.query("SELECT SUM(il.v + ir.w) FROM il JOIN ir ON il.k = ir.k")
        assert isinstance(r, mbx.Err)
        msgs.append(r.error.message)
    assert msgs[0] == msgs[1] == "Out of Range Error: Overflow in addition!"
    check(cc, "SELECT SUM(il.v + ir.w) FROM il JOIN ir ON il.k = ir.k AND il.k = 1", [11])


# ---- types --------------------------------------------------------------------------------------------
def test_int128_sums_over_several_workgroups(cc):
    # 4000 probe rows (16 tiles, one workgroup each) of +-(2^63 - 1): the sum is 2000 (2^63 - 1)
    cc.run(f"CREATE TABLE cp AS SELECT i % 50 AS k, CASE WHEN i % 4 = 3 THEN -{BIG} ELSE {BIG} END AS v FROM range(4000) tbl(i)")
    cc.run("CREATE TABLE cd AS SELECT i AS k, i AS w FROM range(50) tbl(i)")
    check(cc, "SELECT COUNT(*), SUM(cp.v), MIN(cp.v), MAX(cp.v) FROM cp JOIN cd ON cp.k = cd.k", [4000, 2000 * BIG, -BIG, BIG])
    check(cc, f"SELECT SUM(cp.v) FROM cp JOIN cd ON cp.k = cd.k WHERE cp.v < 0", [-1000 * BIG])


def test_decimal_double_date_and_negative_values(cc):
    cents = [(i * 7919) % 2000003 - 1000000 for i in range(600)]
    dbl = [((i * 37) % 101 - 50) * 0.37 + 1e6 * (i % 3) for i in range(600)]
    day = [(i * 13) % 28 + 1 for i in range(600)]
    T = [(i % 20, f"{Decimal(cents[i]) / 100:.2f}", dbl[i], f"DATE '2024-02-{day[i]:02d}'", -5 - i) for i in range(600)]
    D = [(k, k) for k in range(0, 20, 2)]
    make(cc, "tt", "k BIGINT, m DECIMAL(15,2), x DOUBLE, d DATE, neg BIGINT", T)
    make(cc, "td", "k BIGINT, w BIGINT", D)
    hit = [i for i in range(600) if (i % 20) % 2 == 0]
    dec = f"{Decimal(sum(cents[i] for i in hit)) / 100:.2f}"
    check(cc, "SELECT SUM(tt.m), MIN(tt.neg), MAX(tt.neg), MIN(tt.d), MAX(tt.d), MIN(tt.neg + td.w) FROM tt JOIN td ON tt.k = td.k",
          [dec, min(-5 - i for i in hit), max(-5 - i for i in hit), f"2024-02-{min(day[i] for i in hit):02d}",
           f"2024-02-{max(day[i] for i in hit):02d}", min(-5 - i + i % 20 for i in hit)])
    xs = [dbl[i] for i in hit]
    tol = 1e-9 * sum(abs(x) for x in xs)
    for c in cc:
        got = row(c, "SELECT SUM(tt.x), AVG(tt.x), MIN(tt.x), MAX(tt.x), SUM(tt.x * td.w) FROM tt JOIN td ON tt.k = td.k")
        assert abs(float(got[0]) - sum(xs)) <= tol
        assert abs(float(got[1]) - sum(xs) / len(xs)) <= tol / len(xs)
        # MIN / MAX pick one of the values: exact (DOUBLE text is shortest round-trip)
        assert float(got[2]) == min(xs) and float(got[3]) == max(xs), got
        assert abs(float(got[4]) - sum(dbl[i] * (i % 20) for i in hit)) <= 20 * tol
    assert took_fused(cc.fused)
    # a double sum is the same every time: the partials merge in a fixed order
    again = [row(cc.fused, "SELECT SUM(tt.x) FROM tt JOIN td ON tt.k = td.k") for _ in range(3)]
    assert again[0] == again[1] == again[2]


def test_declined_shapes_are_still_right(cc):
    H = [(i % 9, f"{(-1) ** i * (2 ** 100 + i)}", ["red", "green", None, "blue"][i % 4], i) for i in range(90)]
    D = [(k, 10 * k) for k in range(6)]
    for c in cc:
        q(c, "DROP TABLE IF EXISTS hh")
    for c in cc:
        fill(c, "hh", "k BIGINT, s VARCHAR, v BIGINT", [(r[0], r[2], r[3]) for r in H])
    make(cc, "hg", "k BIGINT, h HUGEINT", [(r[0], r[1]) for r in H])
    make(cc, "hd", "k BIGINT, w BIGINT", D)
    hit = [r for r in H if r[0] < 6]
    # MIN of a HUGEINT argument
    check(cc, "SELECT COUNT(*), MIN(hg.h) FROM hg JOIN hd ON hg.k = hd.k", [len(hit), min(int(r[1]) for r in hit)], fused=False)
    check(cc, "SELECT MIN(hg.h), MAX(hg.h) FROM hd JOIN hg ON hg.k = hd.k WHERE hd.w <> 20",
          [min(int(r[1]) for r in hit if r[0] != 2), max(int(r[1]) for r in hit if r[0] != 2)], fused=False)
    # ... while its COUNT is taken
    check(cc, "SELECT COUNT(hg.h) FROM hg JOIN hd ON hg.k = hd.k WHERE hg.h > 0", [sum(1 for r in hit if int(r[1]) > 0)])
    # a VARCHAR predicate in WHERE
    kept = [r for r in hit if r[2] is not None and r[2] != "red"]
    check(cc, "SELECT COUNT(*), SUM(hh.v + hd.w) FROM hh JOIN hd ON hh.k = hd.k WHERE hh.s <> 'red'",
          [len(kept), sum(r[3] + 10 * r[0] for r in kept)], fused=False)
    # a DISTINCT aggregate
    check(cc, "SELECT COUNT(DISTINCT hd.w) FROM hh JOIN hd ON hh.k = hd.k", [6], fused=False)


# ---- composition --------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def star(cc):
    """a fact table and two dimensions"""
    F = [(i, i % 11, i % 4, (i * 37) % 101 - 50) for i in range(300)]
    D = [(k, k * k) for k in range(9)]  # keys 9, 10 of f.a have no row
    E = [(k, 1000 * k) for k in (0, 1, 3)]
    make(cc, "sf", "id BIGINT, a BIGINT, b BIGINT, v BIGINT", F)
    make(cc, "sd", "k BIGINT, sq BIGINT", D)
    make(cc, "se", "k BIGINT, bonus BIGINT", E)
    return F, D, E


def test_three_table_chain(cc, star):
    F, D, E = star
    J = pyjoin(pyjoin(F, D, lambda r: r[1], K0), E, lambda r: r[2], K0)
    check(cc, "SELECT COUNT(*), SUM(sf.v + sd.sq + se.bonus), MAX(se.bonus - sd.sq) FROM sf JOIN sd ON sf.a = sd.k "
              "JOIN se ON se.k = sf.b", [len(J), sum(r[3] + r[5] + r[7] for r in J), max(r[7] - r[5] for r in J)], nested=True)


def test_subquery_values_and_range_inputs(cc, star):
    F, D, E = star
    V = [(1, 10), (3, 30), (8, 80)]
    sub = [(r[0], r[1] + 1) for r in F if r[3] > 0]
    J = pyjoin(sub, V, lambda r: r[1], K0)
    check(cc, "SELECT COUNT(*), SUM(q.id + t.x) FROM (SELECT id, a + 1 AS a1 FROM sf WHERE v > 0) q JOIN "
              "(VALUES (1, 10), (3, 30), (8, 80)) t(k, x) ON q.a1 = t.k", [len(J), sum(r[0] + r[3] for r in J)])
    J = pyjoin([(i,) for i in range(7)], F, K0, lambda r: r[1])
    check(cc, "SELECT COUNT(*), SUM(r.range * sf.v), MIN(r.range) FROM range(7) r JOIN sf ON r.range = sf.a",
          [len(J), sum(r[0] * r[4] for r in J), 0])
    check(cc, "SELECT COUNT(*), SUM(r.range * sf.v), MIN(r.range) FROM sf JOIN range(7) r ON r.range = sf.a",
          [len(J), sum(r[0] * r[4] for r in J), 0])


def test_prepared_statement_patches_its_constants(cc, star):
    F, D, E = star
    for c in cc:
        st = c.prepare("SELECT COUNT(*), SUM(se.bonus + sf.v) FROM sf JOIN se ON sf.b = se.k + ? WHERE sf.v > ?").value
        for add, lo in ((0, -100), (1, 0), (-1, 20)):
            st.bind_bigint(1, add)
            st.bind_bigint(2, lo)
            want = [r for r in pyjoin(F, E, lambda r: r[2], lambda r: r[0] + add) if r[3] > lo]
            assert want, (add, lo)
            assert st.execute().value.rows == [[str(len(want)), str(sum(r[5] + r[3] for r in want))]], (add, lo)
            assert took_fused(c) if c is cc.fused else took_old(c)
        assert st.plan_stats() == {"binds": 1, "reuses": 2}
        st.close()


def test_having_over_the_result(cc, star):
    F, D, E = star
    J = pyjoin(F, E, lambda r: r[2], K0)
    total = sum(r[5] for r in J)
    check(cc, f"SELECT COUNT(*), SUM(se.bonus) FROM sf JOIN se ON sf.b = se.k HAVING SUM(se.bonus) = {total}", [len(J), total])
    for c in cc:
        assert q(c, f"SELECT COUNT(*) FROM sf JOIN se ON sf.b = se.k HAVING SUM(se.bonus) > {total}").row_count() == 0
    assert took_fused(cc.fused)
    n1 = sum(1 for r in J if r[4] == 1)
    check(cc, "SELECT SUM(se.bonus) + COUNT(*) FROM sf JOIN se ON sf.b = se.k WHERE se.k = 1", [1001 * n1])


# ---- the limit ----------------------------------------------------------------------------------------
def test_join_max_rows(mbx):
    pair = Pair(connect(mbx, mbx_join_agg="true", mbx_join_agg_max_run=16, mbx_join_max_rows=1000),
                connect(mbx, mbx_join_agg="false", mbx_join_max_rows=1000))
    make(pair, "ml", "k BIGINT, v BIGINT", [(0, i) for i in range(91)])
    make(pair, "mr", "k BIGINT, w BIGINT", [(0, i) for i in range(11)] + [(1, 0)])
    text = "Out of Range Error: join produces 1001 rows, more than mbx_join_max_rows"
    for c in pair:
        # 91 x 11 = 1 001 pairs, whatever a residual would keep of them; an argument that overflows does not come first
        for sql in ("SELECT COUNT(*) FROM ml JOIN mr ON ml.k = mr.k",
                    "SELECT COUNT(*) FROM ml JOIN mr ON ml.k = mr.k AND ml.v < 0",
                    f"SELECT SUM(ml.v + {BIG}) FROM ml JOIN mr ON ml.k = mr.k"):
            r = c.query(sql)
            assert isinstance(r, mbx.Err), sql
            assert r.error.message == text, sql
            # the next statement is clean
            assert row(c, "SELECT COUNT(*), SUM(v) FROM ml") == ["91", str(sum(range(91)))]
        assert row(c, "SELECT COUNT(*) FROM ml JOIN (SELECT * FROM mr WHERE w < 10) m ON ml.k = m.k") == ["910"]
    assert took_fused(pair.fused) and took_old(pair.plain)
    pair.close()


def test_the_options(mbx):
    cfg = mbx.Config.create()
    for k, v in (("mbx_join_agg", "maybe"), ("mbx_join_agg_max_run", "0"), ("mbx_join_agg_max_run", "-3"),
                 ("mbx_join_agg_max_run", "many")):
        assert isinstance(cfg.set(k, v), mbx.Err), (k, v)
    for k, v in (("mbx_join_agg", "true"), ("mbx_join_agg", "false"), ("mbx_join_agg_max_run", "1"),
                 ("mbx_join_agg_max_run", "1024")):
        assert isinstance(cfg.set(k, v), mbx.Ok), (k, v)
