"""Partitioned GROUP BY (group_part.hip) under a WHERE: a conjunction of integer
range predicates on up to three columns without NULLs is tested inside the hist
and scatter passes (csrc/group_pred_plan.h), rows that fail never become
records, and start[np] holds the selected row count.  Dense and hashed
partitions, single keys and group codes, every record form (packed, one and two
value columns, none).  Every answer is checked against numpy over the oracle's
restatement of the generator, every group compared; the kernel that ran is
read from the query profile.  Sums stay exact in int64: |v| <= 1e6, n < 2^23."""
import numpy as np
import pytest

from conftest import q

pytestmark = pytest.mark.gpu

I64 = np.iinfo(np.int64)
NULL = I64.max  # stands for NULL in the numpy keys: above every key these tests make

NS = [65_536, 65_537, 8 * 8192 + 8191]  # the hashed / code floor, one past it, one row short of a scatter tile
OLD_PATHS = ("hash_group_assign", "group_assign", "vm_filter", "jit_group")
AGG4 = [("count",), ("sum", "v"), ("min", "v"), ("max", "v")]
AGG_SQL = {("count",): "COUNT(*)", ("sum", "v"): "SUM(v)", ("min", "v"): "MIN(v)", ("max", "v"): "MAX(v)",
           ("sum", "w"): "SUM(w)"}


def _conn(mbx, devices=None):
    cfg = mbx.Config.create()
    cfg.set("mbx_profile", "true")
    if devices:
        assert isinstance(cfg.set("gpu_devices", devices), mbx.Ok)
    r = mbx.connect_with_config(cfg)
    assert isinstance(r, mbx.Ok), r.error.message
    return r.value


def _kernels(c):
    return [kk["name"] for kk in c.last_profile()["kernels"]]


def _entry_bytes(c, name):
    e = [kk for kk in c.last_profile()["kernels"] if kk["name"] == name]
    assert len(e) == 1, c.last_profile()
    return e[0]["bytes"]


def _np_group(keys, vals, aggs, mask):
    """numpy GROUP BY over the rows of `mask`, stacked key columns (NULL sorts
    last): rows of strings in key order, NULL cells empty, and their NULL flags."""
    K = np.stack([np.asarray(k, dtype=np.int64)[mask] for k in keys], axis=1)
    if len(K) == 0:
        return [], []
    uk, inv = np.unique(K, axis=0, return_inverse=True)
    inv = inv.reshape(-1)
    cnt = np.bincount(inv, minlength=len(uk))
    cols = []
    for a in aggs:
        if a[0] == "count":
            cols.append(cnt.tolist())
            continue
        v = np.asarray(vals[a[1]], dtype=np.int64)[mask]
        if a[0] == "sum":
            s = np.zeros(len(uk), dtype=np.int64)
            np.add.at(s, inv, v)
            cols.append(s.tolist())
        elif a[0] == "min":
            m = np.full(len(uk), I64.max)
            np.minimum.at(m, inv, v)
            cols.append(m.tolist())
        else:
            m = np.full(len(uk), I64.min)
            np.maximum.at(m, inv, v)
            cols.append(m.tolist())
    rows, nulls = [], []
    for g in range(len(uk)):
        kr = ["" if x == NULL else str(x) for x in uk[g].tolist()]
        rows.append(kr + [str(c[g]) for c in cols])
        nulls.append([x == "" for x in kr] + [False] * len(cols))
    return rows, nulls


# ---- one table per row count ------------------------------------------------
# Built in stages: one expression program pins a register per output column
# (12 registers), so twelve computed columns do not fit one CREATE TABLE AS.
def _make(c, n):
    x = "mbx_synth(42, pos, 50) + 1"
    for t in ("t", "t2", "t1"):
        q(c, f"DROP TABLE IF EXISTS {t}")
    q(c, f"CREATE TABLE t1 AS SELECT CASE WHEN mbx_synth(19, i, 7) = 0 THEN NULL "
         f"ELSE CAST(mbx_synth(23, i, 50000) AS INTEGER) END AS kn, mbx_synth(7, i, 3000) AS kd, "
         f"CAST(mbx_synth(17, i, 300) AS INTEGER) AS a, CAST(mbx_synth(13, i, 100) - 50 AS INTEGER) AS b, "
         f"i AS pos FROM range({n}) tbl(i)")
    q(c, f"CREATE TABLE t2 AS SELECT CAST({x} AS INTEGER) AS x32, {x} AS x, ({x}) * 2 AS xh, "
         f"mbx_synth(9, pos, 2000000) - 1000000 AS v, mbx_synth(11, pos, 1000) AS w, kn, kd, a, b, pos FROM t1")
    q(c, "CREATE TABLE t AS SELECT kd * 1000003 AS ks, CAST(kn AS BIGINT) * 1000003 AS kns, kd, a, b, kn, x, xh, x32, "
         "v, w, pos FROM t2")


def _make_declines(c, n):
    """... and with xn: x with every fifth row NULL (a NULL-able predicate column)."""
    x = "mbx_synth(42, pos, 50) + 1"
    for t in ("t", "t1"):
        q(c, f"DROP TABLE IF EXISTS {t}")
    q(c, f"CREATE TABLE t1 AS SELECT CASE WHEN mbx_synth(29, i, 5) = 0 THEN NULL ELSE mbx_synth(42, i, 50) + 1 END "
         f"AS xn, mbx_synth(7, i, 3000) AS kd, CAST(mbx_synth(17, i, 300) AS INTEGER) AS a, "
         f"CAST(mbx_synth(13, i, 100) - 50 AS INTEGER) AS b, i AS pos FROM range({n}) tbl(i)")
    q(c, f"CREATE TABLE t AS SELECT CAST({x} AS INTEGER) AS x32, {x} AS x, mbx_synth(9, pos, 2000000) - 1000000 AS v, "
         f"mbx_synth(11, pos, 1000) AS w, kd * 1000003 AS ks, xn, kd, a, b, pos FROM t1")


def _columns(oracle, n):
    d = {}
    d["kd"] = oracle.synth_i64(n, 7, 0, 3000, 0)
    d["ks"] = d["kd"] * 1_000_003
    d["a"] = oracle.synth_i64(n, 17, 0, 300, 0)
    d["b"] = oracle.synth_i64(n, 13, 0, 100, -50)
    knull = oracle.synth_i64(n, 19, 0, 7, 0) == 0
    kn = oracle.synth_i64(n, 23, 0, 50000, 0)
    d["kn"] = np.where(knull, NULL, kn)
    d["kns"] = np.where(knull, NULL, kn * 1_000_003)
    d["x"] = oracle.synth_i64(n, 42, 0, 50, 1)
    d["xh"] = d["x"] * 2
    d["x32"] = d["x"]
    d["xn_valid"] = oracle.synth_i64(n, 29, 0, 5, 0) != 0
    d["v"] = oracle.synth_i64(n, 9, 0, 2_000_000, -1_000_000)
    d["w"] = oracle.synth_i64(n, 11, 0, 1000, 0)
    d["pos"] = np.arange(n, dtype=np.int64)
    return d


class _Tables:
    """One profiled connection and one numpy restatement per row count, made
    when a test first asks and shared by every test after it."""

    def __init__(self, mbx, oracle):
        self.mbx, self.oracle, self.made = mbx, oracle, {}

    def get(self, n):
        if n not in self.made:
            c = _conn(self.mbx)
            _make(c, n)
            self.made[n] = (c, _columns(self.oracle, n))
        return self.made[n]

    def close(self):
        for c, _ in self.made.values():
            c.close()


@pytest.fixture(scope="module")
def tables(mbx, oracle):
    t = _Tables(mbx, oracle)
    yield t
    t.close()


def _sql(keys, aggs, where):
    return (f"SELECT {', '.join(keys)}, {', '.join(AGG_SQL[tuple(a)] for a in aggs)} FROM t "
            f"{'WHERE ' + where if where else ''} GROUP BY {', '.join(keys)}")


def _on_new_path(ks, kern):
    assert kern in ks, ks
    for old in OLD_PATHS:
        assert old not in ks, ks


def _check(c, d, keys, aggs, where, mask, kern, ordered):
    """Runs the statement, asserts the path, compares every group."""
    res = q(c, _sql(keys, aggs, where))
    ks = _kernels(c)
    if kern:
        _on_new_path(ks, kern)
    else:
        assert "group_part" not in ks and "group_part_hashed" not in ks, ks
    want, wnulls = _np_group([d[k] for k in keys], d, aggs, mask)
    assert len(res.rows) == len(want), (where, len(res.rows), len(want))
    if ordered:
        assert res.rows == want and res.nulls == wnulls, where
    else:
        assert sorted(zip(res.rows, res.nulls)) == sorted(zip(want, wnulls)), where
    return res


# (keys, kernel, dense): dense results come in key order without ORDER BY
FORMS = [(["kd"], "group_part", True), (["ks"], "group_part_hashed", False), (["a", "b"], "group_part", True),
         (["ks", "b"], "group_part_hashed", False), (["kn"], "group_part", True),
         (["kns"], "group_part_hashed", False)]


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("keys,kern,dense", FORMS, ids=["-".join(f[0]) for f in FORMS])
def test_key_forms_where_x(tables, n, keys, kern, dense):
    """Every key form under WHERE x > 24 (a BIGINT column of its own), with
    every record form: values with MIN / MAX, two value columns (dense), the
    packed COUNT / SUM record, and no value column."""
    c, d = tables.get(n)
    mask = d["x"] > 24
    agg_sets = [AGG4, [("count",), ("sum", "v")], [("count",)]]
    if dense:
        agg_sets.append(AGG4 + [("sum", "w")])
    for aggs in agg_sets:
        _check(c, d, keys, aggs, "x > 24", mask, kern, dense)


PRED_FORMS = [  # (where, numpy mask, dense keys, sparse keys)
    ("{k} >= {t}", lambda d, k: d[k] >= (1500 if k == "kd" else 1500 * 1_000_003), ["kd"], ["ks"]),  # on the key
    ("v < 0", lambda d, k: d["v"] < 0, ["kd"], ["ks"]),  # on the value column
    ("b < -10", lambda d, k: d["b"] < -10, ["a", "b"], ["ks", "b"]),  # on one of two composite keys
    ("x > 24 AND w < 500", lambda d, k: (d["x"] > 24) & (d["w"] < 500), ["kd"], ["ks"]),
    ("x > 24 AND w < 500 AND b >= 0", lambda d, k: (d["x"] > 24) & (d["w"] < 500) & (d["b"] >= 0), ["kd"], ["ks"]),
    ("x32 > 24", lambda d, k: d["x32"] > 24, ["kd"], ["ks"]),  # an INT32 column
    ("x = 25", lambda d, k: d["x"] == 25, ["kd"], ["ks"]),
    ("x BETWEEN 10 AND 20", lambda d, k: (d["x"] >= 10) & (d["x"] <= 20), ["kd"], ["ks"]),
    ("x > 10 AND x <= 30", lambda d, k: (d["x"] > 10) & (d["x"] <= 30), ["kd"], ["ks"]),
]


@pytest.mark.parametrize("sparse", [False, True], ids=["dense", "sparse"])
@pytest.mark.parametrize("form", PRED_FORMS, ids=[f[0] for f in PRED_FORMS])
def test_predicate_forms(tables, form, sparse):
    c, d = tables.get(65_537)
    where, mask, dk, sk = form
    keys = sk if sparse else dk
    where = where.format(k=keys[0], t=1500 * 1_000_003 if sparse else 1500)
    kern = "group_part_hashed" if sparse else "group_part"
    _check(c, d, keys, AGG4, where, mask(d, keys[0]), kern, not sparse)
    if not sparse:  # two value columns: a predicate on w is one on value column 1
        _check(c, d, keys, AGG4 + [("sum", "w")], where, mask(d, keys[0]), kern, True)


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("keys,kern", [(["kd"], "group_part"), (["ks"], "group_part_hashed")], ids=["dense", "sparse"])
def test_selection_edges(tables, monkeypatch, n, keys, kern):
    c, d = tables.get(n)
    dense = kern == "group_part"
    # whole leading chunks and tiles rejected; fewer rows than one tile, all in the first chunk; one row
    for where, mask in (("pos >= 20000", d["pos"] >= 20000), ("pos < 100", d["pos"] < 100),
                        ("pos = 40000", d["pos"] == 40000)):
        res = _check(c, d, keys, AGG4, where, mask, kern, dense)
        if where == "pos = 40000":
            assert len(res.rows) == 1 and res.rows[0][1] == "1"
    # inside the zone map, held by no row (xh is even): no group, the statement's columns
    res = q(c, _sql(keys, AGG4, "xh = 25"))
    _on_new_path(_kernels(c), kern)
    assert res.rows == [] and len(res.columns) == 5
    monkeypatch.setenv("MBX_PART_GROUP", "0")
    old = q(c, _sql(keys, AGG4, "xh = 25"))
    oks = _kernels(c)
    monkeypatch.delenv("MBX_PART_GROUP")
    assert "group_part" not in oks and "group_part_hashed" not in oks, oks
    assert old.rows == [] and list(old.columns) == list(res.columns)
    # outside the zone map, and a comparison with NULL
    for where in ("x > 50", "x > NULL"):
        res = q(c, _sql(keys, AGG4, where))
        assert res.rows == [] and len(res.columns) == 5, where
    # covers the zone map: the no-WHERE kernels, rows and profile bytes
    plain = q(c, _sql(keys, AGG4, None)).rows
    _on_new_path(_kernels(c), kern)
    plain_bytes = _entry_bytes(c, kern)
    allrows = q(c, _sql(keys, AGG4, "x > 0")).rows
    _on_new_path(_kernels(c), kern)
    assert _entry_bytes(c, kern) == plain_bytes
    assert allrows == plain if dense else sorted(allrows) == sorted(plain)
    want, _ = _np_group([d[k] for k in keys], d, AGG4, np.ones(n, dtype=bool))
    assert sorted(plain) == sorted(want)


@pytest.mark.parametrize("n", NS)
def test_profile_bytes(tables, n):
    """Key, value and the predicate's own column, each once."""
    c, d = tables.get(n)
    aggs = [("count",), ("sum", "v")]
    _check(c, d, ["kd"], aggs, "x > 24", d["x"] > 24, "group_part", True)
    assert _entry_bytes(c, "group_part") == 24 * n
    _check(c, d, ["kd"], aggs, "v < 0", d["v"] < 0, "group_part", True)
    assert _entry_bytes(c, "group_part") == 16 * n
    _check(c, d, ["ks"], aggs, "x > 24", d["x"] > 24, "group_part_hashed", False)
    assert _entry_bytes(c, "group_part_hashed") == 24 * n
    # two INT32 keys, an INT32 predicate column of its own
    _check(c, d, ["a", "b"], aggs, "x32 > 24", d["x32"] > 24, "group_part", True)
    assert _entry_bytes(c, "group_part") == (4 + 4 + 8 + 4) * n
    # a NULL-able INT32 key: n / 8 for its bitmap
    _check(c, d, ["kn"], aggs, "x > 24", d["x"] > 24, "group_part", True)
    assert _entry_bytes(c, "group_part") == float("%.0f" % ((4 + 8 + 8) * n + n / 8))  # (printed to whole bytes)


@pytest.mark.parametrize("n", [65_536 + 1, 8 * 8192 + 8191])
@pytest.mark.parametrize("mult,kern", [(1, "group_part"), (1_000_003, "group_part_hashed")])
def test_skew_with_filter(mbx, n, mult, kern):
    """90 % of the rows in one (a, b) group, a filter that keeps every third row."""
    c = _conn(mbx)
    q(c, f"CREATE TABLE sk AS SELECT CASE WHEN i % 10 = 0 THEN ((i * 7) % 3000) * {mult} "
         f"ELSE CAST(4242 AS BIGINT) * {mult} END AS a, "
         f"CAST(CASE WHEN i % 10 = 0 THEN i % 37 ELSE 5 END AS INTEGER) AS b, i % 1000 - 500 AS v, i % 3 AS m3 "
         f"FROM range({n}) tbl(i)")
    i = np.arange(n, dtype=np.int64)
    a = np.where(i % 10 == 0, ((i * 7) % 3000) * mult, 4242 * mult)
    b = np.where(i % 10 == 0, i % 37, 5)
    v = i % 1000 - 500
    got = q(c, "SELECT a, b, COUNT(*), SUM(v), MIN(v), MAX(v) FROM sk WHERE m3 = 0 GROUP BY a, b").rows
    _on_new_path(_kernels(c), kern)
    want, _ = _np_group([a, b], {"v": v}, AGG4, i % 3 == 0)
    assert len(got) == len(want)
    assert sorted(got) == sorted(want)
    if mult == 1:
        assert got == want
    c.close()


@pytest.mark.parametrize("key,kern", [("kd", "group_part"), ("ks", "group_part_hashed")])
def test_over_the_filtered_result(tables, monkeypatch, key, kern):
    """HAVING, ORDER BY ... LIMIT, a projection over the key and a stream over
    the filtered groups give what the hash path gives."""
    c, d = tables.get(65_537)
    stmts = [f"SELECT {key}, COUNT(*), SUM(v) FROM t WHERE x > 24 GROUP BY {key} HAVING COUNT(*) > 12",
             f"SELECT {key}, COUNT(*), SUM(v) FROM t WHERE x > 24 GROUP BY {key} ORDER BY COUNT(*) DESC, {key} LIMIT 7",
             f"SELECT {key} + 1, SUM(v) FROM t WHERE x > 24 GROUP BY {key}"]
    stream_sql = f"SELECT {key}, COUNT(*), MIN(v) FROM t WHERE x > 24 GROUP BY {key}"

    def stream():
        st = c.query_stream(stream_sql).value
        rows = []
        while True:
            ch = st.next().value
            if ch is None or not ch.rows:
                break
            rows += ch.rows
        st.close()
        return rows

    new = []
    for sql in stmts:
        new.append(q(c, sql).rows)
        _on_new_path(_kernels(c), kern)
    new_stream = stream()
    _on_new_path(_kernels(c), kern)
    monkeypatch.setenv("MBX_PART_GROUP", "0")
    old = []
    for sql in stmts:
        old.append(q(c, sql).rows)
        ks = _kernels(c)
        assert "group_part" not in ks and "group_part_hashed" not in ks, ks
    old_stream = stream()
    monkeypatch.delenv("MBX_PART_GROUP")
    assert sorted(new[0]) == sorted(old[0]) and len(new[0]) > 0
    assert new[1] == old[1] and len(new[1]) == 7  # (the order is total: COUNT(*), then the key)
    assert sorted(new[2]) == sorted(old[2])
    assert sorted(new_stream) == sorted(old_stream)
    want, _ = _np_group([d[key]], d, [("count",), ("min", "v")], d["x"] > 24)
    assert sorted(new_stream) == sorted(want)


def test_sharded(mbx, oracle, tables):
    n = 65_537
    c1, d = tables.get(n)
    c = _conn(mbx, "0,0")
    _make(c, n)
    sql = _sql(["kd"], AGG4, "x > 24")
    got = q(c, sql).rows
    ks = _kernels(c)
    assert ks.count("group_part") == 2, ks  # each shard plans against its own zone maps
    for old in OLD_PATHS:
        assert old not in ks, ks
    want, _ = _np_group([d["kd"]], d, AGG4, d["x"] > 24)
    assert sorted(got) == sorted(want)
    assert sorted(got) == sorted(q(c1, sql).rows)
    c.close()


def test_declines_stay_exact(mbx, oracle, monkeypatch):
    """What the predicate plan does not take stays off the partitioned path and exact."""
    n = 65_537
    d = _columns(oracle, n)
    c = _conn(mbx)
    _make_declines(c, n)
    for keys in (["kd"], ["ks"], ["a", "b"]):
        # a NULL-able predicate column: a NULL fails the comparison
        _check(c, d, keys, AGG4, "xn > 24", d["xn_valid"] & (d["x"] > 24), None, False)
        # not a range comparison
        _check(c, d, keys, AGG4, "v % 7 <> 3", np.fmod(d["v"], 7) != 3, None, False)
        # four predicate columns
        _check(c, d, keys, AGG4, "x > 24 AND w < 500 AND x32 < 45 AND pos >= 10",
               (d["x"] > 24) & (d["w"] < 500) & (d["x32"] < 45) & (d["pos"] >= 10), None, False)
        monkeypatch.setenv("MBX_PART_GROUP", "0")
        _check(c, d, keys, AGG4, "x > 24", d["x"] > 24, None, False)
        monkeypatch.delenv("MBX_PART_GROUP")
    # the code path and the hashed form below 2^16 rows
    _make(c, 65_535)
    d2 = _columns(oracle, 65_535)
    for keys in (["a", "b"], ["ks"], ["kn"]):
        _check(c, d2, keys, AGG4, "x > 24", d2["x"] > 24, None, False)
    c.close()
