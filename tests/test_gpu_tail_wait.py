"""The result tail's ticket (csrc/tail_wait.h): a statement that took the tail
returns when its row's ticket is in the mapped buffer, not when the stream has
drained, and with the profile on its kernel times are read later
(SettleProfile).

Tables of 100,000 rows, x = mbx_synth(42, i, 50) + 1, with the code, plane and
histogram floors at 0, so the histogram kernel of the 1e9-row step runs.  The
expected cells come from numpy over the oracle's copy of the same rows, computed
once.  How a statement waited comes from duckdb_mbx_tail_wait_stats, how its
result reached the host from duckdb_mbx_result_tail_stats."""
import numpy as np
import pytest

from conftest import q

pytestmark = pytest.mark.gpu

N = 100_000
WIDE = 1 << 33


def connect(mbx, **opts):
    cfg = mbx.Config.create()
    base = dict(mbx_profile="true", mbx_scan_codes_min_rows=0, mbx_scan_codes_planes_min_rows=0,
                mbx_scan_hist_min_rows=0)
    for k, v in dict(base, **opts).items():
        assert isinstance(cfg.set(k, str(v)), mbx.Ok), (k, v)
    r = mbx.connect_with_config(cfg)
    assert isinstance(r, mbx.Ok), r.error.message
    return r.value


def make_t(c, name="t", seed=42):
    q(c, f"CREATE TABLE {name} AS SELECT mbx_synth({seed}, i, 50) + 1 AS x, mbx_synth(7, i, 32) AS g "
         f"FROM range({N}) tbl(i)")


def load(mbx, c, name, decl, cols):
    q(c, f"CREATE TABLE {name} ({decl})")
    ap = c.create_appender("main", name).value
    for i, a in enumerate(cols):
        assert isinstance(ap.append_column(i, a), mbx.Ok)
    r = ap.commit(len(cols[0]))
    assert isinstance(r, mbx.Ok), r.error.message
    ap.close()


def cells(c, sql):
    res = q(c, sql)
    return [[None if res.nulls[i][j] else res.rows[i][j] for j in range(len(res.rows[i]))]
            for i in range(res.row_count())]


class Ref:
    """x and g as the oracle generates them, and COUNT(*), SUM(x), MIN(x) over x > k for k in 0..49"""
    def __init__(self, oracle, seed=42):
        self.x = oracle.synth_i64(N, seed, 0, 50, 1).astype(np.int64)
        self.g = oracle.synth_i64(N, 7, 0, 32, 0).astype(np.int64)
        self.above = []
        for k in range(50):
            s = self.x[self.x > k]
            self.above.append([str(len(s)), str(int(s.sum())), str(int(s.min()))] if len(s) else ["0", None, None])


@pytest.fixture(scope="module")
def ref(oracle):
    return Ref(oracle)


def delta(c, f):
    """f()'s value and what it added to the counters of both kinds"""
    w0, t0 = c.tail_wait_stats(), c.result_tail_stats()
    v = f()
    w1, t1 = c.tail_wait_stats(), c.result_tail_stats()
    d = {k: w1[k] - w0[k] for k in ("polled", "blocked", "wait_ns")}
    d.update({k: t1[k] - t0[k] for k in ("tail", "host_copy")})
    return v, d


@pytest.mark.parametrize("spin", [None, 0], ids=["spin_default", "spin_0"])
@pytest.mark.parametrize("profile", ["true", "false"], ids=["profile_on", "profile_off"])
def test_no_stale_row(mbx, ref, profile, spin):
    """3000 statements back to back whose answers differ from one to the next: every cell, and every
    statement polled (at mbx_tail_spin_us=0: every one through the blocking wait, the same cells)"""
    opts = dict(mbx_profile=profile)
    if spin is not None:
        opts["mbx_tail_spin_us"] = spin
    c = connect(mbx, **opts)
    make_t(c)
    steps = 3000

    def loop():
        bad = []
        for i in range(steps):
            k = i % 50
            got = cells(c, f"SELECT COUNT(*), SUM(x), MIN(x) FROM t WHERE x > {k}")
            if got != [ref.above[k]]:
                bad.append((i, k, got, ref.above[k]))
        return bad

    bad, d = delta(c, loop)
    assert not bad, bad[:5]
    assert d["tail"] == steps and d["host_copy"] == 0, d
    if spin == 0:
        assert (d["polled"], d["blocked"]) == (0, steps), d
    else:
        assert (d["polled"], d["blocked"]) == (steps, 0), d
    assert d["wait_ns"] > 0, d
    c.close()


def test_profile_deferred(mbx, ref):
    """the kernel times of statements that returned on their ticket, read later: none lost, none twice, in order"""
    c = connect(mbx)
    make_t(c)
    sql = "SELECT COUNT(*) FROM t WHERE x > 24"
    want = [[str(int((ref.x > 24).sum()))]]
    c.profile_drain()

    def entry_ok(k):
        # the histogram of a 6-bit code: 64 counters of 8 bytes; the rows the statement stands for
        return k["name"] == "filter_agg" and 0 < k["ms"] < 1 and k["bytes"] == 512 and k["rows"] == N

    # a single step: last_profile is exactly its kernel
    assert cells(c, sql) == want
    lp = c.last_profile()
    assert len(lp["kernels"]) == 1 and entry_ok(lp["kernels"][0]), lp
    assert lp["total_ms"] > 0
    assert len(c.profile_drain()) == 1
    # a statement answered on the host behind a pending one: its profile is empty, the pending one's kernel is kept
    assert cells(c, sql) == want and cells(c, "SELECT 1") == [["1"]]
    assert c.last_profile()["kernels"] == []
    assert [k["name"] for k in c.profile_drain()] == ["filter_agg"]
    # 500 steps, then one drain
    n = 500
    (_, d) = delta(c, lambda: [cells(c, sql) for _ in range(n)])
    assert (d["polled"], d["blocked"], d["tail"]) == (n, 0, n), d
    kern = c.profile_drain()
    assert len(kern) == n and all(entry_ok(k) for k in kern), (len(kern), [k for k in kern if not entry_ok(k)][:3])
    assert c.profile_drain() == []
    # a drain in the middle of a loop loses and duplicates nothing; other statements keep their place
    for _ in range(100):
        cells(c, sql)
    first = c.profile_drain()
    for _ in range(75):
        cells(c, sql)
    got = cells(c, "SELECT g, COUNT(*) FROM t GROUP BY g")  # (not a tail statement: settles at once)
    assert sorted((int(a), int(b)) for a, b in got) == [(k, int((ref.g == k).sum())) for k in range(32)]
    for _ in range(75):
        cells(c, sql)
    second = c.profile_drain()
    assert len(first) == 100 and all(entry_ok(k) for k in first)
    names = [k["name"] for k in second]
    assert names[:75] == ["filter_agg"] * 75 and names[-75:] == ["filter_agg"] * 75, names
    assert len(names) > 150 and "filter_agg" not in names[75:-75], names[75:-75]
    assert all(entry_ok(k) for k in second[:75] + second[-75:])
    # the event pool: one pair with the pending statement and one with the running one (or what
    # the largest statement so far took at once), however many steps run
    pairs = c.tail_wait_stats()["event_pairs"]
    for _ in range(10_000):
        r = c.query_raw(sql)
        r.close()
    assert c.tail_wait_stats()["event_pairs"] <= max(pairs, 2), (pairs, c.tail_wait_stats())
    assert len(c.profile_drain()) == 10_000
    c.close()


def test_shared_mapped_buffer(mbx, ref):
    """a tail statement, one whose result the copy kernel brings into the same buffer, and one that is sorted
    and cut on the way, by turns"""
    c = connect(mbx)
    make_t(c)
    groups = [[str(k), str(int((ref.g == k).sum())), str(int(ref.x[ref.g == k].sum()))] for k in range(32)]
    top = [[str(v)] for v in np.sort(ref.x)[::-1][:7]]
    for i in range(300):
        k = i % 50
        got, d = delta(c, lambda: cells(c, f"SELECT COUNT(*), SUM(x), MIN(x) FROM t WHERE x > {k}"))
        assert got == [ref.above[k]], (i, got)
        assert (d["tail"], d["host_copy"], d["polled"] + d["blocked"]) == (1, 0, 1), (i, d)
        got, d = delta(c, lambda: cells(c, "SELECT g, COUNT(*), SUM(x) FROM t GROUP BY g"))
        assert sorted(got, key=lambda r: int(r[0])) == groups, (i, got)
        assert (d["tail"], d["host_copy"], d["polled"] + d["blocked"]) == (0, 1, 0), (i, d)
        got, d = delta(c, lambda: cells(c, "SELECT x FROM t ORDER BY x DESC LIMIT 7"))
        assert got == top, (i, got)
        assert (d["tail"], d["polled"] + d["blocked"]) == (0, 0), (i, d)
    c.close()


def test_other_tail_sites(mbx, ref):
    c = connect(mbx)
    make_t(c)
    r = np.random.default_rng(5)
    f = r.integers(-4000, 4001, size=3001, dtype=np.int64).astype(np.float64) * 0.25  # sums exact in any order
    load(mbx, c, "tf", "f DOUBLE", [f])
    a = [(i % 7, i) for i in range(200)]
    b = [(i % 9, 1000 + i) for i in range(90)]
    load(mbx, c, "ja", "k BIGINT, v BIGINT", [np.array([r_[i] for r_ in a], dtype=np.int64) for i in range(2)])
    load(mbx, c, "jb", "k BIGINT, w BIGINT", [np.array([r_[i] for r_ in b], dtype=np.int64) for i in range(2)])

    def tail(sql):
        got, d = delta(c, lambda: cells(c, sql))
        assert (d["tail"], d["host_copy"], d["polled"] + d["blocked"]) == (1, 0, 1), (sql, d)
        assert len(got) == 1, (sql, got)
        return got[0]

    # GlobalReduce over a DOUBLE column
    sel = [float(v) for v in f if v > 3.0]
    got = tail("SELECT SUM(f), MIN(f), MAX(f), COUNT(f) FROM tf WHERE f > 3.0")
    assert [float(got[0]), float(got[1]), float(got[2])] == [sum(sel), min(sel), max(sel)] and got[3] == str(len(sel)), got
    # the join aggregate
    pairs = [(v, w) for k, v in a for kk, w in b if k == kk]
    assert tail("SELECT COUNT(*), SUM(ja.v + jb.w), MIN(jb.w), MAX(ja.v) FROM ja JOIN jb ON ja.k = jb.k") == [
        str(len(pairs)), str(sum(v + w for v, w in pairs)), str(min(w for _, w in pairs)),
        str(max(v for v, _ in pairs))]
    # a predicate every row passes: the known count, no scan
    assert tail("SELECT COUNT(*) FROM t WHERE x >= 1") == [str(N)]
    assert tail("SELECT COUNT(*), SUM(x) FROM t") == [str(N), str(int(ref.x.sum()))]
    # a predicate the zone map rules out
    assert tail("SELECT COUNT(*), SUM(x), MIN(x) FROM t WHERE x > 50") == ["0", None, None]
    # declined: the copy kernel brings the row, and nothing waits on a ticket
    got, d = delta(c, lambda: cells(c, "SELECT COUNT(*) + 1 FROM t WHERE x > 24"))
    assert got == [[str(int((ref.x > 24).sum()) + 1)]], got
    assert (d["tail"], d["host_copy"], d["polled"] + d["blocked"]) == (0, 1, 0), d
    c.close()


def test_work_in_front(mbx, oracle, ref):
    """an appender commit still in flight when a tail statement on another table begins; two connections on one
    device taking the tail by turns"""
    c = connect(mbx)
    make_t(c)
    q(c, "CREATE TABLE b (v BIGINT)")
    v = np.arange(1, 200_001, dtype=np.int64)
    ap = c.create_appender("main", "b").value
    assert isinstance(ap.append_column(0, v), mbx.Ok)
    r = ap.commit(len(v))
    assert isinstance(r, mbx.Ok), r.error.message
    assert cells(c, "SELECT COUNT(*), SUM(x), MIN(x) FROM t WHERE x > 24") == [ref.above[24]]
    ap.close()
    assert cells(c, "SELECT COUNT(*), SUM(v) FROM b") == [[str(len(v)), str(int(v.sum()))]]
    c2 = connect(mbx, mbx_profile="false")
    make_t(c2, "u", seed=43)
    ref2 = Ref(oracle, 43)
    w1, w2 = c.tail_wait_stats(), c2.tail_wait_stats()
    for i in range(200):
        k = (i * 7) % 50
        assert cells(c, f"SELECT COUNT(*), SUM(x), MIN(x) FROM t WHERE x > {k}") == [ref.above[k]], i
        assert cells(c2, f"SELECT COUNT(*), SUM(x), MIN(x) FROM u WHERE x > {k}") == [ref2.above[k]], i
    for cc, w in ((c, w1), (c2, w2)):
        s = cc.tail_wait_stats()
        assert s["polled"] + s["blocked"] - w["polled"] - w["blocked"] == 200, (w, s)
    c2.close()
    c.close()


def test_device_error(mbx, ref, monkeypatch):
    """the device error word comes back through the ticket's path as an error, and the next statement is clean
    (compiled at once, the statement is one jit_aggregate kernel with no error check of its own in front of the
    emit; interpreted, its projection raises the error before anything is emitted)"""
    monkeypatch.setenv("MBX_JIT", "sync")
    c = connect(mbx)
    make_t(c)
    r = np.random.default_rng(9)
    z = r.integers(-5, 6, size=8193, dtype=np.int64) * WIDE + r.integers(0, 1000, size=8193, dtype=np.int64)
    z[0], z[-1] = -5 * WIDE, 5 * WIDE + 999
    load(mbx, c, "tz", "z BIGINT", [z])
    res, d = delta(c, lambda: c.query("SELECT SUM(CAST(z AS INTEGER)), COUNT(*) FROM tz"))
    assert isinstance(res, mbx.Err), res
    assert "out of range" in res.error.message.lower(), res.error.message
    assert (d["polled"], d["blocked"]) == (1, 0), d
    got, d = delta(c, lambda: cells(c, "SELECT COUNT(*), SUM(x), MIN(x) FROM t WHERE x > 24"))
    assert got == [ref.above[24]] and (d["tail"], d["polled"], d["blocked"]) == (1, 1, 0), (got, d)
    assert cells(c, "SELECT COUNT(*), MIN(z), MAX(z) FROM tz") == [[str(len(z)), str(int(z.min())), str(int(z.max()))]]
    c.close()
