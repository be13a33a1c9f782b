"""Code histograms of plane-image columns (csrc/scan_hist.h): with
mbx_scan_hist on (the default) and the table at mbx_scan_hist_min_rows rows or
more (lowered to 0 here, as the planes floor is), a column with a bit-plane
image also keeps 1 << b counters, counter c the rows whose code value - min is
c, counted while ingest builds the planes; a range aggregate the plane scan
would answer is answered from them by one workgroup.

Every answer is compared, exactly, with Python integers over the generated
rows (helpers, predicates, expected cells and the 2^-51 AVG bound are those of
test_gpu_scan_codes.py and test_gpu_scan_planes.py).  Every query also runs on
a second connection with mbx_scan_hist=false over the same rows, and the cells
of the two are compared.  Which path ran comes from the `filter_agg` profile
entry: (1 << b) x 8 bytes with the histogram, planes_read x 4 x ceil(n / 32)
without, b and planes_read from the rows' own min and max by the rule of the
design; 0 where the zone map rules every row out, or lets every row in and only
their number is asked."""
import numpy as np
import pytest

import test_gpu_scan_codes as base
import test_gpu_scan_codes_bits as bits
import test_gpu_scan_planes as planes
from conftest import one, q

pytestmark = pytest.mark.gpu

I64_MIN, I64_MAX = base.I64_MIN, base.I64_MAX
S = 1 << 20
SIZES = [1, 31, 32, 33, 8191, 8192, 8193, S - 1, S, S + 1, 3 * S + 77]
AGGS = ["COUNT(*)", "COUNT(x)", "SUM(x)", "AVG(x)", "MIN(x)", "MAX(x)"]
ALL = "COUNT(*), SUM(x), MIN(x), MAX(x), AVG(x), COUNT(x)"


def _conn(mbx, hist, planes_min_rows=0, hist_min_rows=0, bits_min_rows=None, devices=None, combine=None):
    cfg = mbx.Config.create()
    for k, v in (("mbx_profile", "true"), ("mbx_scan_codes_min_rows", "0"),
                 ("mbx_scan_codes_planes_min_rows", str(planes_min_rows)),
                 ("mbx_scan_hist", "true" if hist else "false"), ("mbx_scan_hist_min_rows", str(hist_min_rows))):
        assert isinstance(cfg.set(k, v), mbx.Ok), k
    if bits_min_rows is not None:
        assert isinstance(cfg.set("mbx_scan_codes_bits_min_rows", str(bits_min_rows)), mbx.Ok)
    if devices:
        assert isinstance(cfg.set("gpu_devices", devices), mbx.Ok)
    if combine:
        assert isinstance(cfg.set("mbx_combine", combine), mbx.Ok)
    r = mbx.connect_with_config(cfg)
    assert isinstance(r, mbx.Ok), r.error.message
    return r.value


def _pair(mbx, **kw):
    return _conn(mbx, True, **kw), _conn(mbx, False, **kw)


def _hist_bytes(amin, amax):
    return (1 << planes._bits(amin, amax)) * 8


def _want_bytes(n, amin, amax, lo, hi, values, hist):
    p = planes._planes_read(amin, amax, lo, hi, values)
    if p is None or p == 0:  # ruled out, or every row passes and only their number is asked: no launch
        return 0
    return _hist_bytes(amin, amax) if hist else planes._scan_bytes(n, p)


def _check_bytes(c, want, sql):
    fa = base._fa_entries(c)
    assert len(fa) <= 1 if want == 0 else len(fa) == 1, (sql, want, fa)
    assert not fa or fa[0]["bytes"] == want, (sql, want, fa)


def _both(on, off, sql, n, amin, amax, lo, hi, values):
    """the row of `sql` on the histogram connection, equal to the other's; each ran its own path"""
    got = one(on, sql)
    _check_bytes(on, _want_bytes(n, amin, amax, lo, hi, values, True), sql)
    assert one(off, sql) == got, sql
    _check_bytes(off, _want_bytes(n, amin, amax, lo, hi, values, False), sql)
    return got


def _preds(kind, x, hole):
    amin, amax = int(x.min()), int(x.max())
    mid = (amin + amax) // 2
    L = kind.lit
    ps = planes._preds(kind, x) + [(f"x <= {L(mid)}", I64_MIN, mid), (f"x >= {L(mid)}", mid, I64_MAX)]
    if mid > I64_MIN:
        ps.append((f"x < {L(mid)}", I64_MIN, mid - 1))
    if hole is not None:  # inside the zone map, and no row has it
        ps.append((f"x = {L(hole)}", hole, hole))
    return ps


def _check_all(on, off, kind, x, hole=None):
    n, amin, amax = len(x), int(x.min()), int(x.max())
    for sql, lo, hi in _preds(kind, x, hole):
        cells, avg = base._expect(kind, x, lo, hi)
        want = {"COUNT(*)": cells[0], "COUNT(x)": cells[0], "SUM(x)": cells[1], "MIN(x)": cells[2], "MAX(x)": cells[3]}
        for a in AGGS:
            got = _both(on, off, f"SELECT {a} FROM t WHERE {sql}", n, amin, amax, lo, hi, a != "COUNT(*)")
            if a != "AVG(x)":
                assert got == [want[a]], (n, sql, a, got)
        got = _both(on, off, f"SELECT {ALL} FROM t WHERE {sql}", n, amin, amax, lo, hi, True)
        assert got[:4] == cells and got[5] == cells[0], (n, sql, got, cells)
        if avg is None:
            assert got[1:5] == ["", "", "", ""], (n, sql, got)  # SUM, MIN, MAX and AVG of no row are NULL
        else:
            assert abs(float(got[4]) - avg) <= 2.0**-51 * abs(avg), (n, sql, got[4], avg)
    cells, _ = base._expect(kind, x, I64_MIN, I64_MAX)
    assert _both(on, off, "SELECT SUM(x), COUNT(*) FROM t", n, amin, amax, I64_MIN, I64_MAX, True) == [cells[1], cells[0]]


KINDS = planes.KINDS + [
    (planes._kind("bigint_const", "BIGINT", -7, 1), 1),
    (planes._kind("integer_b8_neg", "INTEGER", -(2**31) + 1000, 256, dtype=np.int32), 8),
    (planes._kind("bigint_top_b8", "BIGINT", I64_MAX - 255, 256), 8),
]


@pytest.mark.parametrize("kind,b", KINDS, ids=[k.name for k, _ in KINDS])
def test_scan_hist_widths(mbx, oracle, kind, b):
    on, off = _pair(mbx)
    for n in SIZES:
        x = kind.rows(n, oracle)
        hole = None
        if n >= 3 and kind.hi - kind.lo >= 2:  # no row keeps the value next to the smallest
            hole = kind.lo + 1
            x[x == hole] = kind.lo
        if n >= 2:
            assert planes._bits(x.min(), x.max()) == b, (n, x.min(), x.max())
        for c in (on, off):
            base._load(mbx, c, kind, n, x)
        _check_all(on, off, kind, x, hole)
        for c in (on, off):
            q(c, "DROP TABLE t")
    on.close()
    off.close()


def _simple(on, off, x, wheres=(("x > 24", 25, I64_MAX), ("x BETWEEN 9 AND 40", 9, 40), ("x <= 3", I64_MIN, 3))):
    """COUNT(*) alone and COUNT, SUM, MIN, MAX together over the rows x, each connection on its own path"""
    n, amin, amax = len(x), int(x.min()), int(x.max())
    xo = x.astype(object)
    for where, lo, hi in wheres:
        sel = xo[(x >= max(lo, I64_MIN)) & (x <= min(hi, I64_MAX))]
        assert _both(on, off, f"SELECT COUNT(*) FROM t WHERE {where}", n, amin, amax, lo, hi, False) == [str(len(sel))]
        want = [str(len(sel)), str(int(sel.sum())), str(int(sel.min())), str(int(sel.max()))] if len(sel) else ["0", "", "", ""]
        got = _both(on, off, f"SELECT COUNT(*), SUM(x), MIN(x), MAX(x) FROM t WHERE {where}", n, amin, amax, lo, hi, True)
        assert got == want, (where, got, want)


def _append(mbx, cs, x, more, oracle, appender):
    """appends the next `more` rows of the generator to t on every connection; the rows after it"""
    y = base._synth(oracle, more, start=len(x))
    if appender:
        for c in cs:
            ap = c.create_appender("main", "t").value
            assert isinstance(ap.append_column(0, y), mbx.Ok)
            assert isinstance(ap.commit(more), mbx.Ok)
            ap.close()
    else:
        for c in cs:
            q(c, f"INSERT INTO t SELECT mbx_synth(42, i, 50) + 1 FROM range({len(x)}, {len(x) + more}) tbl(i)")
    return np.concatenate([x, y])


def test_scan_hist_appends(mbx, oracle):
    on, off = cs = _pair(mbx, bits_min_rows=0)
    n = S - 8192 - 50  # ends in the middle of a word, a piece short of the segment's end
    assert n % 32
    for c in cs:
        q(c, f"CREATE TABLE t AS SELECT mbx_synth(42, i, 50) + 1 AS x FROM range({n}) tbl(i)")
    x = base._synth(oracle, n)
    _simple(on, off, x)
    # from the middle of a word across a piece boundary, then across the segment's end,
    # through INSERT ... SELECT and through the appender
    for more, appender in ((8192 + 20, False), (300, True)):
        x = _append(mbx, cs, x, more, oracle, appender)
        _simple(on, off, x)
    assert len(x) > S
    # several in a row before the next query, each starting inside a word
    for more, appender in ((33, True), (1, False), (31, True), (8192, False)):
        x = _append(mbx, cs, x, more, oracle, appender)
    _simple(on, off, x)
    # past the column's capacity: the image moves to a larger buffer, the histogram stays
    x = _append(mbx, cs, x, 2 * S + 77, oracle, False)
    _simple(on, off, x)
    # a row below the base moves imin: image and histogram are rebuilt (codes 0..50)
    for c in cs:
        q(c, "INSERT INTO t VALUES (0)")
    x = np.append(x, np.int64(0))
    _simple(on, off, x)
    # one that takes the codes from 6 to 8 bits rebuilds both with 256 counters
    for c in cs:
        q(c, "INSERT INTO t VALUES (-100)")
    x = np.append(x, np.int64(-100))
    assert _hist_bytes(x.min(), x.max()) == 2048
    _simple(on, off, x)
    x = _append(mbx, cs, x, 100, oracle, True)  # and is extended again
    _simple(on, off, x)
    # one that needs 9 bits: planes and histogram are gone, three 10-bit fields to a word answer
    for c in cs:
        q(c, "INSERT INTO t VALUES (300)")
    x = np.append(x, np.int64(300))
    for c in cs:
        base._check(c, x, bits._image_bytes(len(x), 3, 8))
    # one far outside frees the image: the 8-byte values are read again
    for c in cs:
        q(c, "INSERT INTO t VALUES (1000000000000)")
    x = np.append(x, np.int64(10**12))
    for c in cs:
        base._check(c, x, len(x) * 8)
    on.close()
    off.close()


def test_scan_hist_planes_floor(mbx, oracle):
    """a table growing across the planes floor gets its planes and its histogram in one rebuild"""
    on, off = cs = _pair(mbx, planes_min_rows=100_000, bits_min_rows=0)
    n = 60_000
    for c in cs:
        q(c, f"CREATE TABLE t AS SELECT mbx_synth(42, i, 50) + 1 AS x FROM range({n}) tbl(i)")
        base._check(c, base._synth(oracle, n), bits._image_bytes(n, 5, 8))  # below the floor: 6-bit fields
    x = _append(mbx, cs, base._synth(oracle, n), 50_001, oracle, False)
    _simple(on, off, x)
    x = _append(mbx, cs, x, 10, oracle, True)
    _simple(on, off, x)
    on.close()
    off.close()


def test_scan_hist_own_floor(mbx, oracle):
    """below mbx_scan_hist_min_rows the planes answer; the append that crosses it counts every row"""
    c, off = _pair(mbx, hist_min_rows=100_000)
    n = 60_000
    for k in (c, off):
        q(k, f"CREATE TABLE t AS SELECT mbx_synth(42, i, 50) + 1 AS x FROM range({n}) tbl(i)")
    x = base._synth(oracle, n)
    cnt = str(int((x > 24).sum()))
    assert one(c, "SELECT COUNT(*) FROM t WHERE x > 24") == [cnt]
    _check_bytes(c, planes._scan_bytes(n, 3), "below the floor")
    x = _append(mbx, (c, off), x, 50_001, oracle, False)
    _simple(c, off, x)
    c.close()
    off.close()


def test_scan_hist_create_or_replace(mbx, oracle):
    on, off = cs = _pair(mbx)
    for c in cs:
        q(c, f"CREATE TABLE t AS SELECT mbx_synth(42, i, 50) + 1 AS x FROM range({S + 5}) tbl(i)")
    _simple(on, off, base._synth(oracle, S + 5))
    n = 3 * 8192 + 11  # other rows, another base and another width under the same name
    for c in cs:
        q(c, f"CREATE OR REPLACE TABLE t AS SELECT mbx_synth(7, i, 200) - 60 AS x FROM range({n}) tbl(i)")
    x = oracle.synth_i64(n, 7, 0, 200, -60).astype(np.int64)
    assert planes._bits(x.min(), x.max()) == 8
    _simple(on, off, x, wheres=(("x > 24", 25, I64_MAX), ("x BETWEEN -9 AND 40", -9, 40), ("x < -58", I64_MIN, -59)))
    for c in cs:  # and the same width and base again, fewer rows
        q(c, f"CREATE OR REPLACE TABLE t AS SELECT mbx_synth(7, i, 200) - 60 AS x FROM range({n - 8192}) tbl(i)")
    _simple(on, off, x[:n - 8192], wheres=(("x > 24", 25, I64_MAX), ("x = 0", 0, 0)))
    on.close()
    off.close()


def test_scan_hist_sharded(mbx, oracle):
    """two shards on one device: each answers from the histogram of its own rows"""
    n = 2 * S + 4001
    x = base._synth(oracle, n)
    for combine in (None, "rccl_loopback"):
        on, off = _pair(mbx, devices="0,0", combine=combine)
        for c in (on, off):
            q(c, f"CREATE TABLE t AS SELECT mbx_synth(42, i, 50) + 1 AS x FROM range({n}) tbl(i)")
        parts = [x[n * i // 2:n * (i + 1) // 2] for i in range(2)]
        for where, lo, hi in (("x > 24", 25, I64_MAX), ("x BETWEEN 9 AND 40", 9, 40), ("x = 50", 50, 50)):
            sel = x[(x >= lo) & (x <= hi)].astype(object)
            want = [str(len(sel)), str(int(sel.sum())), str(int(sel.min())), str(int(sel.max()))]
            for c, hist in ((on, True), (off, False)):
                assert one(c, f"SELECT COUNT(*), SUM(x), MIN(x), MAX(x) FROM t WHERE {where}") == want, (combine, where)
                fa = base._fa_entries(c)  # one per shard
                assert sorted((k["rows"], k["bytes"]) for k in fa) == sorted(
                    (len(p), _want_bytes(len(p), p.min(), p.max(), lo, hi, True, hist)) for p in parts), (where, fa)
                assert one(c, f"SELECT COUNT(*) FROM t WHERE {where}") == want[:1]
                fa = base._fa_entries(c)
                assert sorted((k["rows"], k["bytes"]) for k in fa) == sorted(
                    (len(p), _want_bytes(len(p), p.min(), p.max(), lo, hi, False, hist)) for p in parts), (where, fa)
        if combine:  # the shards' partials as the combine got them
            for c in (on, off):
                one(c, "SELECT COUNT(*), SUM(x) FROM t WHERE x > 24")
                for i, p in enumerate(parts):
                    sp = c.shard_partial(i)
                    sel = p[p > 24].astype(object)
                    assert sp.value(0, 0) == str(len(sel)) and sp.value(1, 0) == str(int(sel.sum())), (i, sp.cells())
                    sp.close()
        on.close()
        off.close()


def test_scan_hist_one_row_inside_a_query_and_other_entry_points(mbx, oracle):
    on, off = cs = _pair(mbx)
    n = S + 8192 + 3
    x = base._synth(oracle, n)
    xo = x.astype(object)
    hi, lo = xo[x > 24], xo[x < 10]
    for c in cs:
        q(c, f"CREATE TABLE t AS SELECT mbx_synth(42, i, 50) + 1 AS x FROM range({n}) tbl(i)")
        # the one-row aggregate under a subquery, and two of them under UNION ALL
        assert one(c, "SELECT c + 1, m FROM (SELECT COUNT(*) AS c, MAX(x) AS m FROM t WHERE x > 24) u") == \
            [str(len(hi) + 1), "50"]
        got = q(c, "SELECT COUNT(*), MAX(x) FROM t WHERE x > 24 UNION ALL SELECT COUNT(*), MAX(x) FROM t WHERE x < 10").rows
        assert got == [[str(len(hi)), "50"], [str(len(lo)), "9"]], got
        # prepared, with the bound patched between runs
        st = c.prepare("SELECT COUNT(*), SUM(x) FROM t WHERE x > ?").value
        for k in (24, 40, 50):
            st.bind_bigint(1, k)
            sel = xo[x > k]
            assert st.execute().value.rows == [[str(len(sel)), str(int(sel.sum())) if len(sel) else ""]], k
        st.close()
        # stream
        s = c.query_stream("SELECT COUNT(*), SUM(x), MIN(x) FROM t WHERE x > 24").value
        ch = s.next().value
        assert ch.rows == [[str(len(hi)), str(int(hi.sum())), "25"]], ch.rows
        assert s.next().value is None
        s.close()
        # Arrow
        a = c.query_arrow("SELECT COUNT(*), MIN(x), MAX(x) FROM t WHERE x < 10").value
        assert a.row_count() == 1 and [a.raw_int64(j) for j in range(3)] == [[len(lo)], [1], [9]]
        a.close()
    # the plain query last, so that the profile read is its own: both paths ran
    for c, hist in ((on, True), (off, False)):
        assert one(c, "SELECT COUNT(*) FROM t WHERE x > 24") == [str(len(hi))]
        _check_bytes(c, _want_bytes(n, 1, 50, 25, I64_MAX, False, hist), "x > 24")
    on.close()
    off.close()
