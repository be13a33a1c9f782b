"""Range aggregates answered on the host from a mirror of the code histogram
(mbx_scan_hist_host, csrc/aggregate.cpp): where the histogram would answer and the
row is the statement's own result, the host folds its copy of the counters, forms
the cells with the emit's own definition (csrc/emit_cell.h) and launches nothing.

Every floor is 0 here, the new one (mbx_scan_hist_host_min_rows) included.  Every
query runs on a connection with the switch on and on one with it off over the same
rows: the cells are equal as text (AVG too) and equal to Python integers over the
generated rows (generators, predicates and expected cells are those of
test_gpu_scan_hist.py and its neighbours).  Which path ran comes from
duckdb_mbx_scan_hist_host_stats and from the statement's profile, which has no
kernel on the host path."""
import numpy as np
import pytest

import test_gpu_scan_codes as base
import test_gpu_scan_hist as hist
import test_gpu_scan_planes as planes
from conftest import one, q

pytestmark = pytest.mark.gpu

I64_MIN, I64_MAX = base.I64_MIN, base.I64_MAX
S = 1 << 20
SIZES = [1, 33, 8193, S + 1]
C2 = "SELECT COUNT(*), SUM(x), MIN(x), MAX(x) FROM t WHERE x > 24"


def _conn(mbx, host=True, host_min_rows=0, **opts):
    cfg = mbx.Config.create()
    o = {"mbx_profile": "true", "mbx_scan_codes_min_rows": "0", "mbx_scan_codes_planes_min_rows": "0",
         "mbx_scan_codes_bits_min_rows": "0", "mbx_scan_hist_min_rows": "0",
         "mbx_scan_hist_host": "true" if host else "false", "mbx_scan_hist_host_min_rows": str(host_min_rows)}
    o.update(opts)
    for k, v in o.items():
        assert isinstance(cfg.set(k, v), mbx.Ok), k
    r = mbx.connect_with_config(cfg)
    assert isinstance(r, mbx.Ok), r.error.message
    return r.value


def _answered(c):
    return c.scan_hist_host_stats()["answered"]


def _both(on, off, sql):
    """the row of `sql`, answered on the host by `on` (one more answered, no kernel in
    its profile) and on the device by `off`, equal as text"""
    a0, b0 = _answered(on), _answered(off)
    got = one(on, sql)
    assert _answered(on) == a0 + 1, (sql, on.scan_hist_host_stats())
    assert on.last_profile()["kernels"] == [], (sql, on.last_profile())
    assert one(off, sql) == got, sql
    assert _answered(off) == b0 == 0, sql
    return got


KINDS = [(k, b) for k, b in hist.KINDS if k.name in ("bigint_b1", "bigint_b6", "bigint_b8", "integer_b8_neg",
                                                     "bigint_top_b8")]


@pytest.mark.parametrize("kind,b", KINDS, ids=[k.name for k, _ in KINDS])
def test_host_answer_agrees_with_the_device_and_the_rows(mbx, oracle, kind, b):
    on, off = _conn(mbx, True), _conn(mbx, False)
    for n in SIZES:
        x = kind.rows(n, oracle)
        hole = None
        if n >= 3 and kind.hi - kind.lo >= 2:  # no row keeps the value next to the smallest
            hole = kind.lo + 1
            x[x == hole] = kind.lo
        if n >= 2:
            assert planes._bits(x.min(), x.max()) == b
        for c in (on, off):
            base._load(mbx, c, kind, n, x)
        f0 = on.scan_hist_host_stats()["fetches"]
        for sql, lo, hi in hist._preds(kind, x, hole):
            cells, avg = base._expect(kind, x, lo, hi)
            want = {"COUNT(*)": cells[0], "COUNT(x)": cells[0], "SUM(x)": cells[1], "MIN(x)": cells[2],
                    "MAX(x)": cells[3]}
            for a in hist.AGGS:
                got = _both(on, off, f"SELECT {a} FROM t WHERE {sql}")
                if a != "AVG(x)":
                    assert got == [want[a]], (n, sql, a, got)
            got = _both(on, off, f"SELECT {hist.ALL} FROM t WHERE {sql}")
            assert got[:4] == cells and got[5] == cells[0], (n, sql, got, cells)
            if avg is None:
                assert got[1:5] == ["", "", "", ""], (n, sql, got)
            else:
                assert abs(float(got[4]) - avg) <= 2.0**-51 * abs(avg), (n, sql, got[4], avg)
        cells, _ = base._expect(kind, x, I64_MIN, I64_MAX)
        assert _both(on, off, "SELECT SUM(x), COUNT(*) FROM t") == [cells[1], cells[0]]
        assert _both(on, off, "SELECT COUNT(*) FROM t") == [cells[0]]  # no predicate: the row count
        assert on.scan_hist_host_stats()["fetches"] == f0 + 1, n  # one table, one fetch
        for c in (on, off):
            q(c, "DROP TABLE t")
    on.close()
    off.close()


def _cells(x, lo=25):
    sel = x[x >= lo].astype(object)
    return [str(len(sel)), str(int(sel.sum())), str(int(sel.min())), str(int(sel.max()))] if len(sel) else ["0", "", "", ""]


def test_mirror_follows_every_change_of_the_table(mbx, oracle):
    c = _conn(mbx)

    def fresh(x, fetched=1):
        """the answer over all rows after a change: `fetched` fetches, then none"""
        s0 = c.scan_hist_host_stats()
        assert one(c, C2) == _cells(x)
        assert one(c, "SELECT COUNT(*) FROM t WHERE x BETWEEN 9 AND 40") == [str(int(((x >= 9) & (x <= 40)).sum()))]
        s1 = c.scan_hist_host_stats()
        assert s1["fetches"] == s0["fetches"] + fetched and s1["answered"] == s0["answered"] + 2, (s0, s1)

    n = 70_001
    q(c, f"CREATE TABLE t AS SELECT mbx_synth(42, i, 50) + 1 AS x FROM range({n}) tbl(i)")
    x = base._synth(oracle, n)
    fresh(x)
    fresh(x, 0)
    x = hist._append(mbx, [c], x, 8192 + 20, oracle, False)  # INSERT ... SELECT extends
    fresh(x)
    x = hist._append(mbx, [c], x, 300, oracle, True)  # an appender commit, and the query at once
    fresh(x)
    for more, appender in ((33, True), (1, False), (31, True)):  # several flushes, one fetch
        x = hist._append(mbx, [c], x, more, oracle, appender)
    fresh(x)
    q(c, "INSERT INTO t VALUES (0)")  # lowers the minimum: the base moves
    x = np.append(x, np.int64(0))
    fresh(x)
    q(c, "INSERT INTO t VALUES (-100)")  # 6 bits become 8
    x = np.append(x, np.int64(-100))
    fresh(x)
    q(c, "INSERT INTO t VALUES (300)")  # past 8 bits: no histogram, the field scan answers
    x = np.append(x, np.int64(300))
    s0 = c.scan_hist_host_stats()
    assert one(c, C2) == _cells(x)
    assert [k["name"] for k in c.last_profile()["kernels"]].count("filter_agg") == 1
    s1 = c.scan_hist_host_stats()
    assert (s1["answered"], s1["fetches"]) == (s0["answered"], s0["fetches"]), (s0, s1)
    q(c, "INSERT INTO t VALUES (NULL)")  # a NULL frees the image
    assert one(c, C2) == _cells(x)
    assert one(c, "SELECT COUNT(*), COUNT(x) FROM t") == [str(len(x) + 1), str(len(x))]
    assert c.scan_hist_host_stats()["answered"] == s0["answered"]
    n = 3 * 8192 + 11  # other rows, another base and another width under the same name
    q(c, f"CREATE OR REPLACE TABLE t AS SELECT mbx_synth(7, i, 200) - 60 AS x FROM range({n}) tbl(i)")
    x = oracle.synth_i64(n, 7, 0, 200, -60).astype(np.int64)
    fresh(x)
    q(c, "DROP TABLE t")
    q(c, f"CREATE TABLE t AS SELECT mbx_synth(42, i, 50) + 1 AS x FROM range({n}) tbl(i)")  # the same row count
    fresh(base._synth(oracle, n))
    c.close()


def test_statements_that_keep_the_device_path(mbx, oracle):
    n = 50_003
    x = base._synth(oracle, n)
    cnt = int((x > 24).sum())
    create = f"CREATE TABLE t AS SELECT mbx_synth(42, i, 50) + 1 AS x FROM range({n}) tbl(i)"
    c = _conn(mbx)
    q(c, create)
    assert one(c, C2) == _cells(x)
    a0 = _answered(c)
    assert a0 == 1
    assert one(c, "SELECT COUNT(*) + 1 FROM t WHERE x > 24") == [str(cnt + 1)]
    assert one(c, "SELECT COUNT(*) FROM t WHERE x > 24 HAVING COUNT(*) > 0") == [str(cnt)]
    assert one(c, "SELECT COUNT(*) AS k FROM t WHERE x > 24 ORDER BY k") == [str(cnt)]
    assert one(c, "SELECT COUNT(*) FROM t WHERE x > 24 LIMIT 1") == [str(cnt)]
    got = q(c, "SELECT COUNT(*) FROM t WHERE x > 24 UNION ALL SELECT COUNT(*) FROM t WHERE x <= 24").rows
    assert got == [[str(cnt)], [str(n - cnt)]]
    assert one(c, "SELECT k FROM (SELECT COUNT(*) AS k FROM t WHERE x > 24) u") == [str(cnt)]
    q(c, "CREATE TABLE u AS SELECT COUNT(*) AS k FROM t WHERE x > 24")
    q(c, "INSERT INTO u SELECT COUNT(*) FROM t WHERE x <= 24")
    assert q(c, "SELECT k FROM u").rows == [[str(cnt)], [str(n - cnt)]]
    a = c.query_arrow("SELECT COUNT(*), MIN(x) FROM t WHERE x > 24").value
    assert a.row_count() == 1 and [a.raw_int64(j) for j in range(2)] == [[cnt], [25]]
    a.close()
    s = c.scan_hist_host_stats()
    assert s["answered"] == a0 and s["declined"] >= 9 and s["last_reason"], s
    assert one(c, C2) == _cells(x) and _answered(c) == a0 + 1  # and the plain statement still does
    c.close()
    for opts in ({"gpu_devices": "0,0"}, {"mbx_result_tail": "false"}, {"mbx_scan_hist": "false"}):
        c = _conn(mbx, **opts)
        q(c, create)
        assert one(c, C2) == _cells(x), opts
        assert one(c, "SELECT COUNT(*) FROM t WHERE x > 24") == [str(cnt)], opts
        assert _answered(c) == 0, (opts, c.scan_hist_host_stats())
        c.close()


def test_prepared_bounds_each_get_their_own_answer(mbx, oracle):
    c = _conn(mbx)
    n = 40_001
    x = base._synth(oracle, n)
    xo = x.astype(object)
    q(c, f"CREATE TABLE t AS SELECT mbx_synth(42, i, 50) + 1 AS x FROM range({n}) tbl(i)")
    st = c.prepare("SELECT COUNT(*), SUM(x) FROM t WHERE x > ?").value
    a0 = _answered(c)
    for k in range(50):
        st.bind_bigint(1, k)
        sel = xo[x > k]
        assert st.execute().value.rows == [[str(len(sel)), str(int(sel.sum())) if len(sel) else ""]], k
    st.close()
    s = c.scan_hist_host_stats()
    assert s["answered"] == a0 + 50 and s["fetches"] == 1, s
    c.close()


def test_profile_keeps_device_entries_in_order_around_a_host_statement(mbx, oracle):
    c = _conn(mbx, host_min_rows=20_000)
    q(c, "CREATE TABLE t AS SELECT mbx_synth(42, i, 50) + 1 AS x FROM range(30000) tbl(i)")
    q(c, "CREATE TABLE s AS SELECT mbx_synth(42, i, 50) + 1 AS x FROM range(10000) tbl(i)")  # below the floor
    xs = base._synth(oracle, 10000)
    c.profile_drain()
    a0 = _answered(c)
    assert one(c, "SELECT COUNT(*) FROM s WHERE x > 24") == [str(int((xs > 24).sum()))]  # device, on its ticket
    assert one(c, "SELECT COUNT(*) FROM t WHERE x > 24") == [str(int((base._synth(oracle, 30000) > 24).sum()))]
    assert c.last_profile()["kernels"] == []
    assert one(c, "SELECT MAX(x) FROM s WHERE x < 10") == ["9"]
    assert _answered(c) == a0 + 1
    d = c.profile_drain()
    assert [(k["name"], k["bytes"]) for k in d] == [("filter_agg", 512.0), ("filter_agg", 512.0)], d
    c.close()


def test_host_and_device_statements_share_the_mapped_buffer(mbx, oracle):
    """3000 statements back to back with changing bounds; every tenth is in turn a
    GROUP BY statement and a device-path tail statement on a table below the floor"""
    c = _conn(mbx, host_min_rows=20_000)
    n, m = 30_011, 10_007
    q(c, f"CREATE TABLE t AS SELECT mbx_synth(42, i, 50) + 1 AS x FROM range({n}) tbl(i)")
    q(c, f"CREATE TABLE s AS SELECT mbx_synth(7, i, 40) - 5 AS x FROM range({m}) tbl(i)")
    x = base._synth(oracle, n)
    y = oracle.synth_i64(m, 7, 0, 40, -5).astype(np.int64)
    # counts and sums of x > k and of y > k from the values' own histograms
    def above(v, lo, hi):
        cnt, tot, out = 0, 0, {}
        h = {int(k): int(cn) for k, cn in zip(*np.unique(v, return_counts=True))}
        for k in range(hi, lo - 2, -1):
            out[k] = (cnt, tot)
            cnt, tot = cnt + h.get(k, 0), tot + k * h.get(k, 0)
        return out
    ax, ay = above(x, 1, 50), above(y, -5, 34)
    groups = [[str(k), str(cn)] for k, cn in zip(*np.unique(y, return_counts=True))]
    a0, w0 = _answered(c), c.result_tail_stats()["tail"]
    host = dev = 0
    for i in range(3000):
        if i % 20 == 9:
            assert q(c, "SELECT x, COUNT(*) FROM s GROUP BY x ORDER BY x").rows == groups, i
        elif i % 20 == 19:
            k = (i // 20) % 39 - 5
            cnt, tot = ay[k]
            assert one(c, f"SELECT COUNT(*), SUM(x) FROM s WHERE x > {k}") == [str(cnt), str(tot) if cnt else ""], i
            dev += 1
        else:
            k = i % 50
            cnt, tot = ax[k]
            assert one(c, f"SELECT COUNT(*), SUM(x) FROM t WHERE x > {k}") == [str(cnt), str(tot) if cnt else ""], i
            host += 1
    assert _answered(c) == a0 + host
    assert c.result_tail_stats()["tail"] == w0 + dev
    c.close()
