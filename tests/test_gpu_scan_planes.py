"""Bit-plane scan code images (csrc/scan_planes.h): with
mbx_scan_codes_planes_min_rows at 0 a narrow-range integer column whose codes
value - min have b <= 8 bits keeps one bit plane per code bit, in segments of
S = 2^20 rows, and the fused filter-aggregate streams only the planes the
predicate needs.

Every answer is compared, exactly, with numpy over the same rows; the helpers,
the base predicates, the expected cells and the AVG bound (2^-51 relative) are
those of test_gpu_scan_codes.py.  Which planes were read comes from the
`filter_agg` profile entry, planes_read x 4 x ceil(n / 32) bytes, and the
expected planes_read follows from the rows' own min and max by the rule of the
design, not from the engine: b = bit length of max - min (at least 1); the
predicate clamped to [min, max] is clo <= code <= chi; the lower side is tested
iff clo > 0, the upper iff chi < max - min; t is the least of ctz(clo) and
ctz(chi + 1) over the tested sides (b when none is); COUNT(*) alone reads
b - t planes, anything with SUM, MIN, MAX or AVG reads all b.  A predicate that
the zone map rules out reports 0 bytes, as does a COUNT(*) whose predicate
lets every row in."""
import numpy as np
import pytest

import test_gpu_scan_codes as base
import test_gpu_scan_codes_bits as bits
from conftest import one, q

pytestmark = pytest.mark.gpu

I64_MIN, I64_MAX = base.I64_MIN, base.I64_MAX
S = 1 << 20
SIZES = [1, 31, 32, 33, 8191, 8192, 8193, 24 * 8192 + 7, S - 1, S, S + 1, 2 * S + 8192 + 33]


def _conn(mbx, planes_min_rows=0, bits_min_rows=None, devices=None):
    cfg = mbx.Config.create()
    assert isinstance(cfg.set("mbx_profile", "true"), mbx.Ok)
    assert isinstance(cfg.set("mbx_scan_codes_min_rows", "0"), mbx.Ok)
    assert isinstance(cfg.set("mbx_scan_codes_planes_min_rows", str(planes_min_rows)), mbx.Ok)
    if bits_min_rows is not None:
        assert isinstance(cfg.set("mbx_scan_codes_bits_min_rows", str(bits_min_rows)), mbx.Ok)
    if devices:
        assert isinstance(cfg.set("gpu_devices", devices), mbx.Ok)
    r = mbx.connect_with_config(cfg)
    assert isinstance(r, mbx.Ok), r.error.message
    return r.value


def _ctz(v):
    return (v & -v).bit_length() - 1


def _bits(amin, amax):
    return max((int(amax) - int(amin)).bit_length(), 1)


def _planes_read(amin, amax, lo, hi, values):
    """planes a scan of lo <= x <= hi reads over rows with the given min and max; None: ruled out"""
    amin, amax = int(amin), int(amax)
    if lo > hi or hi < amin or lo > amax:
        return None
    b, top = _bits(amin, amax), amax - amin
    clo, chi = max(lo, amin) - amin, min(hi, amax) - amin
    t = b
    if clo > 0:
        t = min(t, _ctz(clo))
    if chi < top:
        t = min(t, _ctz(chi + 1))
    return b if values else b - t


def _scan_bytes(n, planes):
    return planes * 4 * ((n + 31) // 32)


def _check_bytes(c, n, planes, sql):
    fa = base._fa_entries(c)
    if planes is None:  # no row can pass: no scan is needed
        assert len(fa) <= 1, (sql, fa)
        assert not fa or fa[0]["bytes"] == 0, (sql, fa)
        return
    assert len(fa) == 1, (sql, fa)
    assert fa[0]["bytes"] == _scan_bytes(n, planes), (sql, n, planes, fa)


def _kind(name, sqltype, lo, count, dtype=np.int64):
    return base.Kind(name, sqltype, lo, lo + count - 1, dtype=dtype)


# kind, bits per code of the full range
KINDS = [
    (_kind("bigint_b1", "BIGINT", 7, 2), 1),
    (_kind("bigint_b2", "BIGINT", -2, 4), 2),
    (_kind("bigint_b3", "BIGINT", 100, 7), 3),
    (_kind("bigint_b4", "BIGINT", -16, 16), 4),
    (_kind("bigint_b5", "BIGINT", 1, 21), 5),
    (_kind("bigint_b6", "BIGINT", 1, 50), 6),
    (_kind("bigint_b7", "BIGINT", -1, 100), 7),
    (_kind("bigint_b8", "BIGINT", -100, 256), 8),
    (_kind("integer_b6", "INTEGER", -5, 50, dtype=np.int32), 6),
    (_kind("bigint_bottom", "BIGINT", I64_MIN, 50), 6),
    (_kind("bigint_top", "BIGINT", I64_MAX - 49, 50), 6),
]


def _preds(kind, x):
    """base._preds plus a lower bound whose code has trailing zeros and an upper
    bound whose code has trailing ones (both 2^(b-1), the latter less one)"""
    amin, amax = int(x.min()), int(x.max())
    half = 1 << (_bits(amin, amax) - 1)
    L = kind.lit
    more = [(f"x >= {L(amin + half)}", amin + half, I64_MAX),
            (f"x <= {L(amin + half - 1)}", I64_MIN, amin + half - 1),
            (f"x BETWEEN {L(amin + half // 2)} AND {L(amin + half + half // 2 - 1)}", amin + half // 2, amin + half + half // 2 - 1)]
    # (a single row at the very top of int64 has no literal above it)
    return base._preds(kind, x) + [p for p in more if p[1] <= I64_MAX and p[2] <= I64_MAX]


@pytest.mark.parametrize("kind,b", KINDS, ids=[k.name for k, _ in KINDS])
def test_scan_planes_widths(mbx, oracle, kind, b):
    c = _conn(mbx)
    for n in SIZES:
        x = kind.rows(n, oracle)
        amin, amax = int(x.min()), int(x.max())
        if n >= 2:
            assert _bits(amin, amax) == b, (n, amin, amax)  # both ends of the range are present
        base._load(mbx, c, kind, n, x)
        for sql, lo, hi in _preds(kind, x):
            cells, avg = base._expect(kind, x, lo, hi)
            assert one(c, f"SELECT COUNT(*) FROM t WHERE {sql}") == cells[:1], (n, sql)
            _check_bytes(c, n, _planes_read(amin, amax, lo, hi, False), sql)
            assert one(c, f"SELECT COUNT(*), SUM(x) FROM t WHERE {sql}") == cells[:2], (n, sql)
            _check_bytes(c, n, _planes_read(amin, amax, lo, hi, True), sql)
            got = one(c, f"SELECT COUNT(*), SUM(x), MIN(x), MAX(x), AVG(x) FROM t WHERE {sql}")
            assert got[:4] == cells, (n, sql, got, cells)
            _check_bytes(c, n, _planes_read(amin, amax, lo, hi, True), sql)
            if avg is None:
                assert got[4] == ""
            else:
                assert abs(float(got[4]) - avg) <= 2.0**-51 * abs(avg), (n, sql, got[4], avg)
        cells, _ = base._expect(kind, x, I64_MIN, I64_MAX)
        assert one(c, "SELECT SUM(x) FROM t") == [cells[1]]
        _check_bytes(c, n, _bits(amin, amax), "SUM(x)")
        q(c, "DROP TABLE t")
    c.close()


def test_scan_planes_every_range_of_1_50(mbx, oracle):
    c = _conn(mbx)
    n = 24 * 8192 + 7
    q(c, f"CREATE TABLE t AS SELECT mbx_synth(42, i, 50) + 1 AS x FROM range({n}) tbl(i)")
    x = base._synth(oracle, n)
    assert x.min() == 1 and x.max() == 50
    hist = np.bincount(x, minlength=51).astype(object)
    for a in range(1, 51):
        for b in range(a, 51):
            cnt = int(sum(hist[a:b + 1]))
            tot = int(sum(v * hist[v] for v in range(a, b + 1)))
            sql = f"x BETWEEN {a} AND {b}"
            assert one(c, f"SELECT COUNT(*) FROM t WHERE {sql}") == [str(cnt)], sql
            _check_bytes(c, n, _planes_read(1, 50, a, b, False), sql)
            present = [v for v in range(a, b + 1) if hist[v]]
            want = [str(tot), str(present[0]), str(present[-1])] if cnt else ["", "", ""]
            assert one(c, f"SELECT SUM(x), MIN(x), MAX(x) FROM t WHERE {sql}") == want, sql
            _check_bytes(c, n, 6, sql)
    c.close()


def _check(c, x, planes_count, planes_values=None, where="x > 24", lo=25):
    """COUNT(*) alone and COUNT(*), SUM(x) of x >= lo, with the planes each reads"""
    sel = x[x >= lo]
    assert one(c, f"SELECT COUNT(*) FROM t WHERE {where}") == [str(len(sel))]
    _check_bytes(c, len(x), planes_count, where)
    assert one(c, f"SELECT COUNT(*), SUM(x) FROM t WHERE {where}") == [str(len(sel)), str(int(sel.astype(object).sum()))]
    _check_bytes(c, len(x), planes_values, where)


def test_scan_planes_appends(mbx, oracle):
    c = _conn(mbx, bits_min_rows=0)
    n = S - 8192 - 50  # ends in the middle of a word, a piece short of the segment's end
    assert n % 32
    q(c, f"CREATE TABLE t AS SELECT mbx_synth(42, i, 50) + 1 AS x FROM range({n}) tbl(i)")
    x = base._synth(oracle, n)
    _check(c, x, 3, 6)
    # an append inside the range extends the planes from the middle of a word, across a piece ...
    for more in (8192 + 20, 300):  # ... and then across the segment's end
        q(c, f"INSERT INTO t SELECT mbx_synth(42, i, 50) + 1 FROM range({len(x)}, {len(x) + more}) tbl(i)")
        x = base._synth(oracle, len(x) + more)
        _check(c, x, 3, 6)
    assert len(x) > S
    sel = x[(x >= 9) & (x <= 40)]
    assert one(c, "SELECT COUNT(*), SUM(x), MIN(x), MAX(x) FROM t WHERE x BETWEEN 9 AND 40") == \
        [str(len(sel)), str(int(sel.sum())), "9", "40"]
    # past the column's capacity: the image moves to a larger buffer
    more = 2 * S + 77
    q(c, f"INSERT INTO t SELECT mbx_synth(42, i, 50) + 1 FROM range({len(x)}, {len(x) + more}) tbl(i)")
    x = base._synth(oracle, len(x) + more)
    _check(c, x, 3, 6)
    # a row below the base rebuilds the image: codes 0..50, x > 24 is code >= 25
    q(c, "INSERT INTO t VALUES (0)")
    x = np.append(x, np.int64(0))
    _check(c, x, 6, 6)
    _check(c, x, 3, 6, where="x > 23", lo=24)
    # a row that takes the codes from 6 to 8 bits rebuilds it as 8 planes: x > 24 is code >= 125
    q(c, "INSERT INTO t VALUES (-100)")
    x = np.append(x, np.int64(-100))
    _check(c, x, 8, 8)
    _check(c, x, 1, 8, where="x > 27", lo=28)  # code >= 128: the top plane alone
    # one that needs 9 bits leaves three 10-bit fields to a word
    q(c, "INSERT INTO t VALUES (300)")
    x = np.append(x, np.int64(300))
    sel = x[x > 24]
    assert one(c, "SELECT COUNT(*) FROM t WHERE x > 24") == [str(len(sel))]
    fa = base._fa_entries(c)
    assert len(fa) == 1 and fa[0]["bytes"] == bits._image_bytes(len(x), 3, 8), fa
    base._check(c, x, bits._image_bytes(len(x), 3, 8))
    # one far outside frees the image: the 8-byte values are read again
    q(c, "INSERT INTO t VALUES (1000000000000)")
    x = np.append(x, np.int64(10**12))
    base._check(c, x, len(x) * 8)
    c.close()


def test_scan_planes_floor(mbx, oracle):
    c = _conn(mbx, planes_min_rows=100_000, bits_min_rows=0)
    n = 60_000
    q(c, f"CREATE TABLE t AS SELECT mbx_synth(42, i, 50) + 1 AS x FROM range({n}) tbl(i)")
    base._check(c, base._synth(oracle, n), bits._image_bytes(n, 5, 8))  # below the floor: 6-bit fields
    q(c, f"INSERT INTO t SELECT mbx_synth(42, i, 50) + 1 FROM range({n}, {n + 50_001}) tbl(i)")
    x = base._synth(oracle, n + 50_001)
    _check(c, x, 3, 6)  # past it: rebuilt once as planes
    q(c, f"INSERT INTO t SELECT mbx_synth(42, i, 50) + 1 FROM range({len(x)}, {len(x) + 10}) tbl(i)")
    x = base._synth(oracle, len(x) + 10)
    _check(c, x, 3, 6)
    c.close()


def test_scan_planes_floor_default_keeps_fields(mbx, oracle):
    """at the default floor (2^24 rows) a small table keeps today's image"""
    c = bits._conn(mbx)
    n = 200_003
    q(c, f"CREATE TABLE t AS SELECT mbx_synth(42, i, 50) + 1 AS x FROM range({n}) tbl(i)")
    base._check(c, base._synth(oracle, n), bits._image_bytes(n, 5, 8))
    c.close()


def test_scan_planes_shards_have_their_own_planes(mbx, oracle):
    n = 3_000_017
    c = _conn(mbx, devices="0,0,0")
    q(c, f"CREATE TABLE t AS SELECT (i // 1000003 + 1) * mbx_synth(42, i, 50) AS x FROM range({n}) tbl(i)")
    x = (np.arange(n, dtype=np.int64) // 1000003 + 1) * oracle.synth_i64(n, 42, 0, 50, 0).astype(np.int64)
    widths = set()
    for where, lo, hi in (("x > 23", 24, I64_MAX), ("x >= 0", 0, I64_MAX), ("x BETWEEN 48 AND 63", 48, 63),
                          ("x > 120", 121, I64_MAX)):
        m = (x >= lo) & (x <= hi)
        for values in (False, True):
            if values:
                assert one(c, f"SELECT COUNT(*), SUM(x) FROM t WHERE {where}") == [str(int(m.sum())), str(int(x[m].sum()))]
            else:
                assert one(c, f"SELECT COUNT(*) FROM t WHERE {where}") == [str(int(m.sum()))]
            fa = base._fa_entries(c)  # one per shard, in the order the shards finished
            want = []
            for i in range(3):  # part i holds rows [n i / 3, n (i + 1) / 3); each has the planes of its own range
                part = x[n * i // 3:n * (i + 1) // 3]
                widths.add(_bits(part.min(), part.max()))
                planes = _planes_read(part.min(), part.max(), lo, hi, values)
                want.append((len(part), 0 if planes is None else _scan_bytes(len(part), planes)))
            assert sorted((k["rows"], k["bytes"]) for k in fa) == sorted(want), (where, values, fa)
    assert len(widths) > 1, widths
    c.close()
