"""Bit-packed scan code images (csrc/scan_codes.h): with
mbx_scan_codes_bits_min_rows at 0 a narrow-range integer column keeps F codes
of value - min per 32-bit word, in fields of 32 // F bits, and the fused
filter-aggregate streams those words.

Every answer is compared, exactly, with numpy over the same rows; the
predicates, the expected cells and the AVG bound (2^-51 relative) are those of
test_gpu_scan_codes.py.  Which image was read comes from the `filter_agg`
profile entry.  The expected field count follows from the rows' own min and max
by the rule of the design, not from the engine: b = bit length of max - min
gives 32, 16, 10, 8, 6, 5 fields for b = 1..6, 4 for b = 7..8, 3 for b = 9..10
(8-byte columns only), 2 for b = 11..16 (8-byte columns only), else no image.
An image of F fields reports its words, 4 * ceil(n / F) bytes; the plain 1- and
2-byte images (F = 4, F = 2) keep reporting their codes, n and 2 n bytes, as
test_gpu_scan_codes.py pins them at sizes that are no multiple of 4.  A
predicate that the zone map rules out reports 0 bytes."""
import numpy as np
import pytest

import test_gpu_scan_codes as base
from conftest import one, q

pytestmark = pytest.mark.gpu

I64_MIN, I64_MAX = base.I64_MIN, base.I64_MAX


def _conn(mbx, bits_min_rows=0, devices=None):
    cfg = mbx.Config.create()
    assert isinstance(cfg.set("mbx_profile", "true"), mbx.Ok)
    assert isinstance(cfg.set("mbx_scan_codes_min_rows", "0"), mbx.Ok)
    assert isinstance(cfg.set("mbx_scan_codes_bits_min_rows", str(bits_min_rows)), mbx.Ok)
    if devices:
        assert isinstance(cfg.set("gpu_devices", devices), mbx.Ok)
    r = mbx.connect_with_config(cfg)
    assert isinstance(r, mbx.Ok), r.error.message
    return r.value


def _fields(phys, lo, hi):
    b = max((int(hi) - int(lo)).bit_length(), 1)
    if b <= 6:
        return {1: 32, 2: 16, 3: 10, 4: 8, 5: 6, 6: 5}[b]
    if b <= 8:
        return 4
    if phys == 8 and b <= 10:
        return 3
    if phys == 8 and b <= 16:
        return 2
    return 0


def _image_bytes(n, f, phys):
    if f == 0:
        return n * phys
    if f in (4, 2):
        return n * (4 // f)
    return 4 * ((n + f - 1) // f)


def _kind(name, sqltype, lo, count, dtype=np.int64):
    return base.Kind(name, sqltype, lo, lo + count - 1, dtype=dtype)


# name, kind, fields per word of the full range
KINDS = [
    (_kind("bigint_2", "BIGINT", 7, 2), 32),
    (_kind("bigint_4", "BIGINT", -2, 4), 16),
    (_kind("bigint_8", "BIGINT", 100, 8), 10),
    (_kind("bigint_16", "BIGINT", -16, 16), 8),
    (_kind("bigint_32", "BIGINT", 1, 32), 6),
    (_kind("bigint_50", "BIGINT", 1, 50), 5),
    (_kind("bigint_64", "BIGINT", -1, 64), 5),
    (_kind("bigint_200", "BIGINT", -100, 200), 4),
    (_kind("bigint_1000", "BIGINT", 1, 1000), 3),
    (_kind("integer_32", "INTEGER", -5, 32, dtype=np.int32), 6),
    (_kind("integer_1000", "INTEGER", 1, 1000, dtype=np.int32), 0),
    (_kind("bigint_bottom", "BIGINT", I64_MIN, 50), 5),
    (_kind("bigint_top", "BIGINT", I64_MAX - 49, 50), 5),
]


def _sizes(f):
    f = f or 4
    return [1, f, f + 1, 4 * f + 1, 256 * f - 1, 256 * f, 256 * f + 1, 24 * 256 * f + 7, 2_000_003]


def _check_bytes(c, want, ruled_out, image, sql):
    fa = base._fa_entries(c)
    if ruled_out:
        assert len(fa) <= 1, (sql, fa)
        if fa:
            assert fa[0]["bytes"] == (0 if image else want), (sql, fa)
        return
    assert len(fa) == 1, (sql, fa)
    assert fa[0]["bytes"] == want, (sql, fa, want)


@pytest.mark.parametrize("kind,fields", KINDS, ids=[k.name for k, _ in KINDS])
def test_scan_codes_bits_field_widths(mbx, oracle, kind, fields):
    c = _conn(mbx)
    for n in _sizes(fields):
        x = kind.rows(n, oracle)
        f = _fields(kind.phys, x.min(), x.max())
        if n >= 2:
            assert f == fields, (n, f, fields)  # both ends of the range are present
        want = _image_bytes(n, f, kind.phys)
        base._load(mbx, c, kind, n, x)
        amin, amax = int(x.min()), int(x.max())
        for sql, lo, hi in base._preds(kind, x):
            cells, avg = base._expect(kind, x, lo, hi)
            ruled_out = hi < amin or lo > amax
            assert one(c, f"SELECT COUNT(*) FROM t WHERE {sql}") == cells[:1], (n, sql)
            _check_bytes(c, want, ruled_out, f > 0, sql)
            assert one(c, f"SELECT COUNT(*), SUM(x) FROM t WHERE {sql}") == cells[:2], (n, sql)
            _check_bytes(c, want, ruled_out, f > 0, sql)
            got = one(c, f"SELECT COUNT(*), SUM(x), MIN(x), MAX(x), AVG(x) FROM t WHERE {sql}")
            assert got[:4] == cells, (n, sql, got, cells)
            _check_bytes(c, want, ruled_out, f > 0, sql)
            if avg is None:
                assert got[4] == ""
            else:
                assert abs(float(got[4]) - avg) <= 2.0**-51 * abs(avg), (n, sql, got[4], avg)
        cells, _ = base._expect(kind, x, I64_MIN, I64_MAX)
        assert one(c, "SELECT SUM(x) FROM t") == [cells[1]]
        _check_bytes(c, want, False, f > 0, "SUM(x)")
        q(c, "DROP TABLE t")
    c.close()


def test_scan_codes_bits_appends(mbx, oracle):
    c = _conn(mbx)
    n = 200_003  # 3 codes in the last word
    q(c, f"CREATE TABLE t AS SELECT mbx_synth(42, i, 50) + 1 AS x FROM range({n}) tbl(i)")
    x = base._synth(oracle, n)
    base._check(c, x, _image_bytes(n, 5, 8))
    # an append inside the range extends the 6-bit image from the middle of a word
    q(c, f"INSERT INTO t SELECT mbx_synth(42, i, 50) + 1 FROM range({n}, {n + 70_001}) tbl(i)")
    x = base._synth(oracle, n + 70_001)
    base._check(c, x, _image_bytes(len(x), 5, 8))
    sel = x[(x >= 10) & (x <= 40)]
    assert one(c, "SELECT COUNT(*), SUM(x), MIN(x), MAX(x) FROM t WHERE x BETWEEN 10 AND 40") == \
        [str(len(sel)), str(int(sel.sum())), "10", "40"]
    # one row that needs 8 bits rebuilds the image at a byte a row
    q(c, "INSERT INTO t VALUES (-100)")
    x = np.append(x, np.int64(-100))
    base._check(c, x, len(x) * 1)
    base._check(c, x, len(x) * 1, where="x >= -100", lo=-100)
    # one row far outside frees it: the 8-byte values are read again
    q(c, "INSERT INTO t VALUES (1000000000000)")
    x = np.append(x, np.int64(10**12))
    base._check(c, x, len(x) * 8)
    c.close()


def test_scan_codes_bits_floor(mbx, oracle):
    c = _conn(mbx, bits_min_rows=100_000)
    n = 60_000
    q(c, f"CREATE TABLE t AS SELECT mbx_synth(42, i, 50) + 1 AS x FROM range({n}) tbl(i)")
    base._check(c, base._synth(oracle, n), n * 1)  # below the floor: the byte image
    q(c, f"INSERT INTO t SELECT mbx_synth(42, i, 50) + 1 FROM range({n}, {n + 50_001}) tbl(i)")
    x = base._synth(oracle, n + 50_001)
    base._check(c, x, _image_bytes(len(x), 5, 8))  # past it: rebuilt once in 6-bit fields
    c.close()


def test_scan_codes_bits_shards_have_their_own_width(mbx, oracle):
    n = 3_000_017
    c = _conn(mbx, devices="0,0,0")
    q(c, f"CREATE TABLE t AS SELECT (i // 1000003) * 10 + mbx_synth(42, i, 50) AS x FROM range({n}) tbl(i)")
    x = np.arange(n, dtype=np.int64) // 1000003 * 10 + oracle.synth_i64(n, 42, 0, 50, 0).astype(np.int64)
    for where, m in (("x > 24", x > 24), ("x >= 0", x >= 0), ("x BETWEEN 45 AND 55", (x >= 45) & (x <= 55))):
        assert one(c, f"SELECT COUNT(*) FROM t WHERE {where}") == [str(int(m.sum()))]
        fa = base._fa_entries(c)  # in shard order
        assert len(fa) == 3, fa  # one per shard
        assert sum(k["rows"] for k in fa) == n, fa
        at = 0
        for k in fa:  # the parts hold consecutive rows; each has the width of its own range
            part = x[at:at + k["rows"]]
            at += k["rows"]
            f = _fields(8, part.min(), part.max())
            assert f in (4, 5), (f, fa)  # 50 to 70 distinct values
            lo, hi = {"x > 24": (25, I64_MAX), "x >= 0": (0, I64_MAX), "x BETWEEN 45 AND 55": (45, 55)}[where]
            ruled_out = hi < part.min() or lo > part.max()
            assert k["bytes"] == (0 if ruled_out else _image_bytes(len(part), f, 8)), (where, k, f)
        assert one(c, f"SELECT COUNT(*), SUM(x) FROM t WHERE {where}") == [str(int(m.sum())), str(int(x[m].sum()))]
        assert len(base._fa_entries(c)) == 3
    c.close()
