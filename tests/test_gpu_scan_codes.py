"""Scan code images (csrc/scan_codes.h): a narrow-range integer table column
keeps a 1- or 2-byte image of value - min, and the fused filter-aggregate
streams it instead of the 4- or 8-byte values.

Every answer is compared, exactly, with numpy over the same rows.  Which path
ran is read from the `filter_agg` profile entry: it reports the bytes actually
read, rows x code width where an image exists and rows x physical width where
none does (or the connection has mbx_scan_codes=false).  The expected width
comes from the rows' own min and max by the rule of the design (range <= 256:
1 byte; <= 65536 and an 8-byte column: 2 bytes; else none), not from the
engine.  A predicate that the zone map rules out entirely is answered without
a scan: its entry, when there is one, reports 0 bytes on the code path.

AVG is a double: sum and count are exact, so the engine's cell differs from
float(sum) / (float(count) * 10^scale) by at most the roundings of the int128
-> double conversion, the scaled divisor and the division, 3 x 2^-53 relative;
the bound below is 2^-51."""
import numpy as np
import pytest

from conftest import one, q

pytestmark = pytest.mark.gpu

I64_MIN, I64_MAX = -(2**63), 2**63 - 1
SIZES = [0, 1, 15, 16, 17, 511, 512, 513, 1023, 1024, 1025, 8_000_003]


def _conn(mbx, codes=True, devices=None, flush_rows=None):
    cfg = mbx.Config.create()
    assert isinstance(cfg.set("mbx_profile", "true"), mbx.Ok)
    assert isinstance(cfg.set("mbx_scan_codes_min_rows", "0"), mbx.Ok)
    assert isinstance(cfg.set("mbx_scan_codes", "true" if codes else "false"), mbx.Ok)
    if devices:
        assert isinstance(cfg.set("gpu_devices", devices), mbx.Ok)
    if flush_rows:
        assert isinstance(cfg.set("mbx_appender_flush_rows", str(flush_rows)), mbx.Ok)
    r = mbx.connect_with_config(cfg)
    assert isinstance(r, mbx.Ok), r.error.message
    return r.value


def _width(phys, lo, hi):
    rng = int(hi) - int(lo) + 1
    if rng <= 256:
        return 1
    if rng <= 65536 and phys == 8:
        return 2
    return 0


class Kind:
    def __init__(self, name, sqltype, lo, hi, dtype=np.int64, scale=0, ctas=False):
        self.name, self.sqltype, self.lo, self.hi, self.dtype, self.scale, self.ctas = name, sqltype, lo, hi, dtype, scale, ctas
        self.phys = np.dtype(dtype).itemsize

    def rows(self, n, oracle):
        if self.ctas:
            return oracle.synth_i64(n, 42, 0, 50, 1).astype(np.int64)
        r = np.random.default_rng(1234 + n)
        off = r.integers(0, self.hi - self.lo + 1, size=n, dtype=np.uint64)
        if n >= 2:  # both ends of the range present
            off[0], off[-1] = 0, self.hi - self.lo
        x = (off + np.uint64(self.lo % 2**64)).astype(np.uint64).view(np.int64)  # wraps: no int64 overflow
        return x.astype(self.dtype)

    def lit(self, v):
        v = min(max(int(v), I64_MIN), I64_MAX)
        if not self.scale:
            return str(v)
        assert v >= 0
        return f"{v // 10**self.scale}.{v % 10**self.scale:0{self.scale}d}"

    def cell(self, v):  # text of a SUM / MIN / MAX cell
        return str(v) if not self.scale else f"{v // 10**self.scale}.{v % 10**self.scale:0{self.scale}d}"


KINDS = [
    Kind("bigint_1_50", "BIGINT", 1, 50),
    Kind("integer_m100_100", "INTEGER", -100, 100, dtype=np.int32),
    Kind("decimal_100_5000", "DECIMAL(15,2)", 100, 5000, scale=2),
    Kind("bigint_0_65535", "BIGINT", 0, 65535),
    Kind("bigint_65537_wide", "BIGINT", 7, 7 + 65536),
    Kind("bigint_top", "BIGINT", I64_MAX - 49, I64_MAX),
    Kind("bigint_bottom", "BIGINT", I64_MIN, I64_MIN + 49),
    Kind("ctas_synth_1_50", "BIGINT", 1, 50, ctas=True),
]


def _load(mbx, c, kind, n, x):
    if kind.ctas:
        q(c, f"CREATE TABLE t AS SELECT mbx_synth(42, i, 50) + 1 AS x FROM range({n}) tbl(i)")
        return
    q(c, f"CREATE TABLE t (x {kind.sqltype})")
    if n:
        ap = c.create_appender("main", "t").value
        assert isinstance(ap.append_column(0, x), mbx.Ok)
        r = ap.commit(n)
        assert isinstance(r, mbx.Ok), r.error.message
        ap.close()


def _preds(kind, x):
    """(sql, lo, hi) with lo <= x <= hi the same predicate over the raw values"""
    if len(x):
        imin, imax = int(x.min()), int(x.max())
    else:
        imin, imax = kind.lo, kind.hi
    mid = (imin + imax) // 2
    L = kind.lit
    ps = [(f"x > {L(mid)}", mid + 1, I64_MAX),
          (f"x = {L(imin)}", imin, imin),
          (f"x = {L(imax)}", imax, imax),
          (f"x >= {L(imin)}", imin, I64_MAX),
          (f"x BETWEEN {L(max(imin - 5, 0 if kind.scale else I64_MIN))} AND {L(imin + 5)}", imin - 5, imin + 5),
          (f"x BETWEEN {L(imax - 5)} AND {L(imax + 5)}", imax - 5, min(imax + 5, I64_MAX))]
    if imin > I64_MIN:
        ps.append((f"x < {L(imin)}", I64_MIN, imin - 1))
    if imax < I64_MAX:
        ps.append((f"x > {L(imax)}", imax + 1, I64_MAX))
    return ps


def _expect(kind, x, lo, hi):
    """cells of COUNT(*), SUM, MIN, MAX and the AVG as a float (None: NULL)"""
    xi = x.astype(np.int64)
    m = (xi >= max(lo, I64_MIN)) & (xi <= min(hi, I64_MAX))
    cnt = int(m.sum())
    if cnt == 0:
        return ["0", "", "", ""], None
    sel = xi[m]
    base = int(sel.min())
    s = base * cnt + int((sel.view(np.uint64) - np.uint64(base % 2**64)).sum(dtype=np.uint64))
    return [str(cnt), kind.cell(s), kind.cell(base), kind.cell(int(sel.max()))], float(s) / (float(cnt) * 10**kind.scale)


def _fa_entries(c):
    return [k for k in c.last_profile()["kernels"] if k["name"] == "filter_agg"]


def _check_bytes(c, n, per_row, ruled_out, image, sql):
    fa = _fa_entries(c)
    if ruled_out:  # no row can pass: no scan is needed
        assert len(fa) <= 1, (sql, fa)
        if fa:
            assert fa[0]["bytes"] == (0 if image else n * per_row), (sql, fa)
        return
    assert len(fa) == 1, (sql, fa)
    assert fa[0]["bytes"] == n * per_row, (sql, fa, n, per_row)


def _run_queries(c, kind, n, x, per_row, image):
    if n == 0:
        assert one(c, "SELECT COUNT(*) FROM t WHERE x >= " + kind.lit(kind.lo)) == ["0"]
        assert one(c, "SELECT SUM(x) FROM t") == [""]
        return
    amin, amax = int(x.min()), int(x.max())
    for sql, lo, hi in _preds(kind, x):
        cells, avg = _expect(kind, x, lo, hi)
        ruled_out = hi < amin or lo > amax
        assert one(c, f"SELECT COUNT(*) FROM t WHERE {sql}") == cells[:1], sql
        _check_bytes(c, n, per_row, ruled_out, image, sql)
        got = one(c, f"SELECT COUNT(*), SUM(x), MIN(x), MAX(x), AVG(x) FROM t WHERE {sql}")
        assert got[:4] == cells, (sql, got, cells)
        _check_bytes(c, n, per_row, ruled_out, image, sql)
        if avg is None:
            assert got[4] == ""
        else:
            assert abs(float(got[4]) - avg) <= 2.0**-51 * abs(avg), (sql, got[4], avg)
    cells, _ = _expect(kind, x, I64_MIN, I64_MAX)
    assert one(c, "SELECT SUM(x) FROM t") == [cells[1]]
    _check_bytes(c, n, per_row, False, image, "SUM(x)")


@pytest.mark.parametrize("kind", KINDS, ids=[k.name for k in KINDS])
def test_scan_codes_edge_sizes(mbx, oracle, kind):
    on, off = _conn(mbx, True), _conn(mbx, False)
    for n in SIZES:
        x = kind.rows(n, oracle)
        w = _width(kind.phys, x.min(), x.max()) if n else 0
        for c, per_row, image in ((on, w or kind.phys, w > 0), (off, kind.phys, False)):
            _load(mbx, c, kind, n, x)
            _run_queries(c, kind, n, x, per_row, image)
            q(c, "DROP TABLE t")
    on.close()
    off.close()


def _synth(oracle, n, start=0):
    return oracle.synth_i64(n, 42, start, 50, 1).astype(np.int64)


def _check(c, x, n_bytes, where="x > 24", lo=25):
    sel = x[x >= lo]
    assert one(c, f"SELECT COUNT(*), SUM(x) FROM t WHERE {where}") == [str(len(sel)), str(int(sel.astype(object).sum()))]
    fa = _fa_entries(c)
    assert len(fa) == 1 and fa[0]["bytes"] == n_bytes, (fa, n_bytes)


def test_scan_codes_appends(mbx, oracle):
    c = _conn(mbx)
    n = 200_003
    q(c, f"CREATE TABLE t AS SELECT mbx_synth(42, i, 50) + 1 AS x FROM range({n}) tbl(i)")
    x = _synth(oracle, n)
    _check(c, x, n * 1)
    # an append inside the range extends the image
    q(c, f"INSERT INTO t SELECT mbx_synth(42, i, 50) + 1 FROM range({n}, {n + 70_001}) tbl(i)")
    x = _synth(oracle, n + 70_001)
    _check(c, x, len(x) * 1)
    # a value far outside drops it: the 8-byte values are read again
    q(c, "INSERT INTO t VALUES (1000000000000)")
    x = np.append(x, np.int64(10**12))
    _check(c, x, len(x) * 8)
    # a second table: an insert below the base that still fits one byte rebuilds the image
    q(c, f"CREATE TABLE u AS SELECT mbx_synth(42, i, 50) + 1 AS x FROM range({n}) tbl(i)")
    q(c, "INSERT INTO u VALUES (-100)")
    y = np.append(_synth(oracle, n), np.int64(-100))
    for where, lo in (("x > 24", 25), ("x >= -100", -100), ("x > -100", -99)):
        sel = y[y >= lo]
        assert one(c, f"SELECT COUNT(*), SUM(x) FROM u WHERE {where}") == [str(len(sel)), str(int(sel.sum()))]
        fa = _fa_entries(c)
        assert len(fa) == 1 and fa[0]["bytes"] == len(y) * 1, fa
    # ... and one that needs two bytes rebuilds it at that width
    q(c, "INSERT INTO u VALUES (300)")
    y = np.append(y, np.int64(300))
    sel = y[y >= 25]
    assert one(c, "SELECT COUNT(*), SUM(x) FROM u WHERE x > 24") == [str(len(sel)), str(int(sel.sum()))]
    fa = _fa_entries(c)
    assert len(fa) == 1 and fa[0]["bytes"] == len(y) * 2, fa
    # replaced and dropped tables leave nothing behind
    q(c, "CREATE OR REPLACE TABLE t AS SELECT mbx_synth(42, i, 50) + 1 AS x FROM range(1000) tbl(i)")
    _check(c, _synth(oracle, 1000), 1000)
    q(c, "DROP TABLE t")
    q(c, "DROP TABLE u")
    q(c, "CREATE TABLE t AS SELECT mbx_synth(42, i, 50) + 1 AS x FROM range(5000) tbl(i)")
    _check(c, _synth(oracle, 5000), 5000)
    c.close()


def test_scan_codes_async_appender_flushes(mbx):
    """three appender flushes of 70 001 rows each leave their DMA and zone map
    in flight; the query after them sees an image of all the rows"""
    per = 70_001
    c = _conn(mbx, flush_rows=per)
    q(c, "CREATE TABLE t (x BIGINT)")
    x = np.random.default_rng(7).integers(1, 51, size=3 * per, dtype=np.int64)
    ap = c.create_appender("main", "t").value
    for v in x.tolist():
        ap.begin_row()
        ap.append_bigint(v)
        ap.end_row()
    sel = x[x > 24]
    assert one(c, "SELECT COUNT(*), SUM(x), MIN(x), MAX(x) FROM t WHERE x > 24") == \
        [str(len(sel)), str(int(sel.sum())), str(sel.min()), str(sel.max())]
    fa = _fa_entries(c)
    assert len(fa) == 1 and fa[0]["bytes"] == 3 * per, fa
    ap.close()
    assert one(c, "SELECT COUNT(*) FROM t WHERE x > 24") == [str(len(sel))]
    c.close()


def test_scan_codes_shards_have_their_own_base(mbx, oracle):
    n = 3_000_017
    c = _conn(mbx, devices="0,0,0")
    q(c, f"CREATE TABLE t AS SELECT (i // 1000003) * 10 + mbx_synth(42, i, 50) AS x FROM range({n}) tbl(i)")
    x = np.arange(n, dtype=np.int64) // 1000003 * 10 + oracle.synth_i64(n, 42, 0, 50, 0).astype(np.int64)
    for where, m in (("x > 24", x > 24), ("x >= 0", x >= 0), ("x BETWEEN 45 AND 55", (x >= 45) & (x <= 55))):
        assert one(c, f"SELECT COUNT(*) FROM t WHERE {where}") == [str(int(m.sum()))]
        fa = _fa_entries(c)
        assert len(fa) == 3, fa  # one per shard
        assert sum(k["bytes"] for k in fa) == n, fa  # every part through its 1-byte image
        assert one(c, f"SELECT COUNT(*), SUM(x) FROM t WHERE {where}") == [str(int(m.sum())), str(int(x[m].sum()))]
        assert len(_fa_entries(c)) == 3
    c.close()
