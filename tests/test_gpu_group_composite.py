"""Partitioned GROUP BY (group_part.hip) over composite and NULL-able integer
keys: the key columns and their validity fold into one group code in the hist
and scatter passes (csrc/group_code.h), dense codes reduce in LDS tables in
code order (key order, NULLs last per key), sparse ones in the hashed tables,
and the emit kernel decodes the code back into the key columns.  Every answer
is checked against numpy over the oracle's restatement of the generator, and
the kernel that ran is read from the query profile."""
import numpy as np
import pytest

from conftest import q

pytestmark = pytest.mark.gpu

I64 = np.iinfo(np.int64)
NULL = I64.max  # stands for NULL in the numpy keys: above every key these tests make (the edge case maps its own)


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


def _np_group(keys, vals, aggs, null=NULL):
    """numpy GROUP BY over stacked key columns (`null` = NULL, sorts last):
    rows of strings in key order, NULL cells empty, and their NULL flags.
    aggs: ("count",) | ("sum", name) | ("min", name) | ("max", name)."""
    K = np.stack([np.asarray(k, dtype=np.int64) for k in keys], axis=1)
    uk, inv = np.unique(K, axis=0, return_inverse=True)
    inv = inv.reshape(-1)
    cnt = np.bincount(inv, minlength=len(uk))
    cols = []
    for a in aggs:
        if a[0] == "count":
            cols.append(cnt.tolist())
            continue
        v = np.asarray(vals[a[1]], dtype=np.int64)
        if a[0] == "sum":  # exact: |v| < 2^40 and n < 2^23 in every test here, so int64 holds
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
        kr = ["" if x == null else str(x) for x in uk[g].tolist()]
        rows.append(kr + [str(c[g]) for c in cols])
        nulls.append([x == "" for x in kr] + [False] * len(cols))
    return rows, nulls


# ---- the case-1 table: a in [0, 300), b in [-50, 50): 30 000 codes ----------
AB_SQL = "SELECT a, b, COUNT(*), SUM(v), MIN(v), MAX(v), SUM(w) FROM ab GROUP BY a, b"
AB_AGGS = [("count",), ("sum", "v"), ("min", "v"), ("max", "v"), ("sum", "w")]


def _make_ab(c, n):
    q(c, "DROP TABLE IF EXISTS ab")
    q(c, f"CREATE TABLE ab AS SELECT CAST(mbx_synth(7, i, 300) AS INTEGER) AS a, "
         f"CAST(mbx_synth(13, i, 100) - 50 AS INTEGER) AS b, mbx_synth(9, i, 2000000) - 1000000 AS v, "
         f"mbx_synth(11, i, 1000) AS w FROM range({n}) tbl(i)")


_ab_cache = {}


def _expect_ab(oracle, n):
    if n not in _ab_cache:
        a = oracle.synth_i64(n, 7, 0, 300, 0)
        b = oracle.synth_i64(n, 13, 0, 100, -50)
        v = oracle.synth_i64(n, 9, 0, 2_000_000, -1_000_000)
        w = oracle.synth_i64(n, 11, 0, 1000, 0)
        _ab_cache[n] = _np_group([a, b], {"v": v, "w": w}, AB_AGGS)
    return _ab_cache[n]


@pytest.mark.parametrize("n", [65_536, 65_537, 200_003])
def test_dense_two_keys_in_key_order(mbx, oracle, n):
    c = _conn(mbx)
    _make_ab(c, n)
    got = q(c, AB_SQL).rows
    ks = _kernels(c)
    assert "group_part" in ks and "hash_group_assign" not in ks and "jit_group" not in ks, ks
    want, _ = _expect_ab(oracle, n)
    assert len(got) == len(want)
    assert got == want  # key order, no ORDER BY
    c.close()


def test_hashed_two_keys(mbx, oracle):
    n = 300_007
    c = _conn(mbx)
    q(c, f"CREATE TABLE hk AS SELECT mbx_synth(7, i, 1000) * 1000003 AS a, CAST(mbx_synth(13, i, 50) AS INTEGER) AS b, "
         f"mbx_synth(9, i, 2000000) - 1000000 AS v FROM range({n}) tbl(i)")
    a = oracle.synth_i64(n, 7, 0, 1000, 0) * 1_000_003
    b = oracle.synth_i64(n, 13, 0, 50, 0)
    v = oracle.synth_i64(n, 9, 0, 2_000_000, -1_000_000)
    got = q(c, "SELECT a, b, COUNT(*), SUM(v), MIN(v), MAX(v) FROM hk GROUP BY a, b").rows
    ks = _kernels(c)
    assert "group_part_hashed" in ks and "hash_group_assign" not in ks, ks
    want, _ = _np_group([a, b], {"v": v}, [("count",), ("sum", "v"), ("min", "v"), ("max", "v")])
    assert sorted(got) == sorted(want)
    got = q(c, "SELECT a, b, COUNT(*) FROM hk GROUP BY a, b").rows  # no value column
    ks = _kernels(c)
    assert "group_part_hashed" in ks and "hash_group_assign" not in ks, ks
    assert sorted(got) == sorted(r[:3] for r in want)
    c.close()


def _null_key_sql(seed, nseed, mod, every, mult=1, ktype="INTEGER"):
    return (f"CASE WHEN mbx_synth({nseed}, i, {every}) = 0 THEN NULL "
            f"ELSE CAST(mbx_synth({seed}, i, {mod}) * {mult} AS {ktype}) END")


def _null_key_np(oracle, n, seed, nseed, mod, every, mult=1):
    k = oracle.synth_i64(n, seed, 0, mod, 0) * mult
    return np.where(oracle.synth_i64(n, nseed, 0, every, 0) == 0, NULL, k)


@pytest.mark.parametrize("mult,kern", [(1, "group_part"), (1_000_003, "group_part_hashed")])
def test_one_nullable_key(mbx, oracle, mult, kern):
    """One NULL-able key over a range of 50 000 (x 1 000 003: sparse), 1/7 NULL:
    the NULL group comes last on the dense path, its cell empty and flagged."""
    n = 200_003
    c = _conn(mbx)
    ktype = "INTEGER" if mult == 1 else "BIGINT"
    q(c, f"CREATE TABLE nk AS SELECT {_null_key_sql(7, 19, 50000, 7, mult, ktype)} AS k, "
         f"mbx_synth(9, i, 2000000) - 1000000 AS v FROM range({n}) tbl(i)")
    k = _null_key_np(oracle, n, 7, 19, 50000, 7, mult)
    v = oracle.synth_i64(n, 9, 0, 2_000_000, -1_000_000)
    res = q(c, "SELECT k, COUNT(*), SUM(v), MIN(v), MAX(v) FROM nk GROUP BY k")
    ks = _kernels(c)
    assert kern in ks and "hash_group_assign" not in ks, ks
    want, wnulls = _np_group([k], {"v": v}, [("count",), ("sum", "v"), ("min", "v"), ("max", "v")])
    if mult == 1:
        assert res.rows == want and res.nulls == wnulls
        assert res.rows[-1][0] == "" and res.nulls[-1][0]
    else:
        assert sorted(zip(res.rows, res.nulls)) == sorted(zip(want, wnulls))
    c.close()


def test_two_nullable_keys(mbx, oracle):
    """Both keys NULL-able (1/7 and 1/5, independent, so both-NULL rows exist):
    301 x 41 = 12 341 codes, dense, key order with NULLs last per key."""
    n = 200_003
    c = _conn(mbx)
    q(c, f"CREATE TABLE n2 AS SELECT {_null_key_sql(7, 19, 300, 7)} AS a, "
         f"{_null_key_sql(13, 23, 40, 5, 1, 'BIGINT')} AS b, mbx_synth(9, i, 2000000) - 1000000 AS v "
         f"FROM range({n}) tbl(i)")
    a = _null_key_np(oracle, n, 7, 19, 300, 7)
    b = _null_key_np(oracle, n, 13, 23, 40, 5)
    assert ((a == NULL) & (b == NULL)).any()
    v = oracle.synth_i64(n, 9, 0, 2_000_000, -1_000_000)
    res = q(c, "SELECT a, b, COUNT(*), SUM(v) FROM n2 GROUP BY a, b")
    ks = _kernels(c)
    assert "group_part" in ks and "hash_group_assign" not in ks, ks
    want, wnulls = _np_group([a, b], {"v": v}, [("count",), ("sum", "v")])
    assert res.rows == want and res.nulls == wnulls
    assert res.rows[-1][:2] == ["", ""]
    c.close()


KEY_DEFS = [  # (seed, mod, add, type): 20 x 30 x 7 x 11 x 3 codes
    (7, 20, -10, "INTEGER"), (13, 30, 1 << 33, "BIGINT"), (17, 7, 0, "BIGINT"), (23, 11, -5, "INTEGER"),
    (29, 3, 0, "INTEGER")]


@pytest.mark.parametrize("nk,kern", [(3, "group_part"), (4, "group_part"), (5, "hash_group_assign")])
def test_three_to_five_mixed_keys(mbx, oracle, nk, kern):
    """Three and four keys of mixed INTEGER / BIGINT (4200 and 46 200 codes);
    five keys are beyond the code plan and stay exact on the hash path."""
    n = 150_001
    c = _conn(mbx)
    defs = KEY_DEFS[:nk]
    cols = ", ".join(f"CAST(mbx_synth({s}, i, {m}) + ({a}) AS {t}) AS k{j}" for j, (s, m, a, t) in enumerate(defs))
    q(c, f"CREATE TABLE mk AS SELECT {cols}, mbx_synth(9, i, 2000000) - 1000000 AS v FROM range({n}) tbl(i)")
    keys = [oracle.synth_i64(n, s, 0, m, a) for s, m, a, _ in defs]
    v = oracle.synth_i64(n, 9, 0, 2_000_000, -1_000_000)
    names = ", ".join(f"k{j}" for j in range(nk))
    got = q(c, f"SELECT {names}, COUNT(*), SUM(v), MAX(v) FROM mk GROUP BY {names}").rows
    ks = _kernels(c)
    assert kern in ks, ks
    want, _ = _np_group(keys, {"v": v}, [("count",), ("sum", "v"), ("max", "v")])
    if kern == "group_part":
        assert "hash_group_assign" not in ks, ks
        assert got == want
    else:
        assert "group_part" not in ks and "group_part_hashed" not in ks, ks
        assert sorted(got) == sorted(want)
    c.close()


def test_refusals_stay_exact(mbx, oracle):
    """No code plan: two sparse BIGINT keys each spanning about 2^40 (2^80
    codes), and one NULL-able key that holds INT64_MIN and INT64_MAX (a radix
    of 2^64 + 1).  The hash path answers both."""
    n = 100_003
    c = _conn(mbx)
    q(c, f"CREATE TABLE rf AS SELECT mbx_synth(7, i, 300) * 3665038759 AS a, mbx_synth(13, i, 200) * 5525731083 AS b, "
         f"mbx_synth(9, i, 2000000) - 1000000 AS v FROM range({n}) tbl(i)")
    a = oracle.synth_i64(n, 7, 0, 300, 0) * 3_665_038_759
    b = oracle.synth_i64(n, 13, 0, 200, 0) * 5_525_731_083
    v = oracle.synth_i64(n, 9, 0, 2_000_000, -1_000_000)
    got = q(c, "SELECT a, b, COUNT(*), SUM(v) FROM rf GROUP BY a, b").rows
    ks = _kernels(c)
    assert "hash_group_assign" in ks and "group_part" not in ks and "group_part_hashed" not in ks, ks
    want, _ = _np_group([a, b], {"v": v}, [("count",), ("sum", "v")])
    assert sorted(got) == sorted(want)
    q(c, f"CREATE TABLE re AS SELECT CASE WHEN i % 7 = 0 THEN NULL WHEN i % 7 = 1 THEN -9223372036854775807 - 1 "
         f"WHEN i % 7 = 2 THEN 9223372036854775807 ELSE (i % 5000) * 1000003 END AS k, i AS v FROM range({n}) tbl(i)")
    i = np.arange(n, dtype=np.int64)
    # (INT64_MAX is a key here: NULL is mapped to a value no row holds, and its cell blanked below)
    null = -12345
    k = np.where(i % 7 == 0, null, np.where(i % 7 == 1, I64.min, np.where(i % 7 == 2, I64.max, (i % 5000) * 1_000_003)))
    res = q(c, "SELECT k, COUNT(*), SUM(v) FROM re GROUP BY k")
    ks = _kernels(c)
    assert "hash_group_assign" in ks and "group_part" not in ks and "group_part_hashed" not in ks, ks
    want, wnulls = _np_group([k], {"v": i}, [("count",), ("sum", "v")], null=null)
    assert sorted(zip(res.rows, res.nulls)) == sorted(zip(want, wnulls))
    c.close()


@pytest.mark.parametrize("n", [65_536 + 1, 8 * 8192 + 8191])
@pytest.mark.parametrize("mult,kern", [(1, "group_part"), (1_000_003, "group_part_hashed")])
def test_skew_and_ragged_tiles(mbx, n, mult, kern):
    """90 % of the rows in one (a, b) group (one partition spans many reduce
    pieces), row counts just past a scatter tile and one row short of one."""
    c = _conn(mbx)
    q(c, f"CREATE TABLE sk AS SELECT CASE WHEN i % 10 = 0 THEN ((i * 7) % 3000) * {mult} "
         f"ELSE CAST(4242 AS BIGINT) * {mult} END AS a, "
         f"CAST(CASE WHEN i % 10 = 0 THEN i % 37 ELSE 5 END AS INTEGER) AS b, i % 1000 - 500 AS v "
         f"FROM range({n}) tbl(i)")
    i = np.arange(n, dtype=np.int64)
    a = np.where(i % 10 == 0, ((i * 7) % 3000) * mult, 4242 * mult)
    b = np.where(i % 10 == 0, i % 37, 5)
    v = i % 1000 - 500
    got = q(c, "SELECT a, b, COUNT(*), SUM(v), MIN(v), MAX(v) FROM sk GROUP BY a, b").rows
    ks = _kernels(c)
    assert kern in ks and "hash_group_assign" not in ks, ks
    want, _ = _np_group([a, b], {"v": v}, [("count",), ("sum", "v"), ("min", "v"), ("max", "v")])
    assert sorted(got) == sorted(want)
    if mult == 1:
        assert got == want
    c.close()


def test_floor_and_switch(mbx, oracle, monkeypatch):
    """Below 2^16 rows the shape keeps the earlier paths; MBX_PART_GROUP=0 turns
    the attempt off and the hash path gives the same groups."""
    c = _conn(mbx)
    _make_ab(c, 65_535)
    got = q(c, AB_SQL).rows
    ks = _kernels(c)
    assert "group_part" not in ks and "group_part_hashed" not in ks, ks
    assert sorted(got) == sorted(_expect_ab(oracle, 65_535)[0])
    _make_ab(c, 200_003)
    new = q(c, AB_SQL).rows
    assert "group_part" in _kernels(c)
    monkeypatch.setenv("MBX_PART_GROUP", "0")
    off = q(c, AB_SQL).rows
    ks = _kernels(c)
    monkeypatch.delenv("MBX_PART_GROUP")
    assert "hash_group_assign" in ks and "group_part" not in ks, ks
    assert sorted(off) == sorted(new)
    c.close()


def test_overflow_falls_back_to_hash_path(mbx):
    """4.5e6 distinct (a, b): more groups than the hashed tables hold."""
    n = 4_500_000
    c = _conn(mbx)
    q(c, f"CREATE TABLE ov AS SELECT i * 1000003 AS a, i % 3 AS b FROM range({n}) tbl(i)")
    r = c.query_raw("SELECT COUNT(*), SUM(c) FROM (SELECT a, b, COUNT(*) AS c FROM ov GROUP BY a, b) t")
    assert r.value(0, 0) == str(n) and r.value(1, 0) == str(n)
    r.close()
    assert "hash_group_assign" in _kernels(c), _kernels(c)
    c.close()


def test_sharded(mbx, oracle):
    n = 400_009
    c = _conn(mbx, "0,0")
    _make_ab(c, n)
    got = q(c, AB_SQL).rows
    ks = _kernels(c)
    assert ks.count("group_part") == 2 and "hash_group_assign" not in ks, ks  # each shard plans its own code
    assert sorted(got) == sorted(_expect_ab(oracle, n)[0])
    c.close()


def test_deferred_count_and_order_limit(mbx, oracle):
    """The top-level query leaves the group count on the device (query_raw reads
    it with the rows); under ORDER BY / LIMIT it is settled first."""
    n = 200_003
    c = _conn(mbx)
    _make_ab(c, n)
    want, _ = _expect_ab(oracle, n)
    rr = c.query_raw(AB_SQL)
    assert rr.row_count() == len(want)
    rows, _ = rr.cells()
    rr.close()
    assert "group_part" in _kernels(c)
    assert rows == want
    top = q(c, AB_SQL + " ORDER BY a, b LIMIT 5").rows
    assert top == want[:5]
    c.close()
