"""Table loading shared by the GPU suites: the columnar appender with an exact
read-back for the numeric tables of vm_cases, the row appender for tables with
VARCHAR columns (fill), and the edge tables at other sizes (retable: tiled or
permuted rows under a fresh id)."""
import struct

import numpy as np

import vm_cases as V
import vm_reference as R
from conftest import q


def _f64(raw):
    return struct.unpack("<d", raw)[0] if len(raw) == 8 else struct.unpack("<f", raw)[0]


def profiled(mbx):
    """a connection whose last_profile() names the kernels of the last statement"""
    cfg = mbx.Config.create()
    assert isinstance(cfg.set("mbx_profile", "true"), mbx.Ok)
    r = mbx.connect_with_config(cfg)
    assert isinstance(r, mbx.Ok), r.error.message
    return r.value


def kernels(conn):
    return [k["name"] for k in conn.last_profile()["kernels"]]


def tile(n, base=V.N):
    """row indices that repeat a base-row table up to n rows"""
    return [r % base for r in range(n)]


def retable(table, rows, cols, name=None):
    """a vm_cases.Table holding rows `rows` (an index array: tiled, permuted,
    repeated) of the named columns of `table`, with `id` renumbered 0..len-1 so
    that it stays unique"""
    out = [V.Col("id", "BIGINT", range(len(rows)))]
    for k in cols:
        if k == "id":
            continue
        c = table.cols[k]
        out.append(V.Col(k, c.sqltype, [c.values[r] for r in rows], [c.valid[r] for r in rows]))
    return V.Table(name or table.name, out)


def check_cell(c, v, text, raw, where):
    """one non-NULL result cell against the column's value v: floats by bit
    pattern (any NaN matches NaN), everything else as text"""
    if c.sqltype in ("DATE", "TIMESTAMP"):  # the stored days / microseconds, not their spelling
        assert int.from_bytes(raw(), "little", signed=True) == v, (where, raw())
    elif c.kind in ("f64", "f32"):
        got = _f64(raw())
        assert (got != got) if v != v else R.bits(got) == R.bits(v), (where, got, v)
    elif c.kind == "dec":
        assert text == V.dec_text(v, c.scale), (where, text)
    elif c.kind == "bool":
        assert text == ("true" if v else "false"), (where, text)
    else:
        assert text == str(v), (where, text)


def load(mbx, conn, table, name, rows, cols):
    """table `name` with the given rows of the given columns, through the
    columnar appender; then read back: the load itself must be exact"""
    cols = [table.cols[k] for k in cols]
    q(conn, f"CREATE TABLE {name} (" + ", ".join(f"{c.name} {c.sqltype}" for c in cols) + ")")
    ap = conn.create_appender("main", name).value
    idx = np.array(rows, dtype=np.int64)
    for j, c in enumerate(cols):
        valid = np.array(c.valid, dtype=np.uint8)[idx]
        r = ap.append_column(j, c.numpy()[idx], None if valid.all() else valid)
        assert isinstance(r, mbx.Ok), r.error.message
    r = ap.commit(len(rows))
    assert isinstance(r, mbx.Ok), r.error.message
    ap.close()
    res = conn.query_raw(f"SELECT * FROM {name}")
    assert res.row_count() == len(rows)
    text, nulls = res.cells()
    for j, c in enumerate(cols):
        for k, r in enumerate(rows):
            v = c.get(r)
            assert nulls[k][j] == (v is None), (name, c.name, r)
            if v is not None:
                check_cell(c, v, text[k][j], lambda: res.raw(j, k), (name, c.name, r))
    res.close()


def fill(c, name, cols, rows):
    """table `name` (`cols`: the column definitions) from Python rows through
    the row appender: None, str, float and int cells"""
    q(c, f"CREATE TABLE {name} ({cols})")
    ap = c.create_appender("main", name).value
    for row in rows:
        ap.begin_row()
        for k, v in enumerate(row):
            if v is None:
                ap.append_null()
            elif isinstance(v, str):
                ap.append_varchar(v)
            elif isinstance(v, float):
                ap.append_double(v)
            else:
                ap.append_int(v)
        ap.end_row()
    ap.flush()
    ap.close()
