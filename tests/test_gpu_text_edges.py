"""Result cells spelled on the device (csrc/text_kernels.hip) against str(v),
vm_cases.dec_text and true / false, at the values where the spelling takes
another path: INT64_MIN, UBIGINT above 2^63, HUGEINT min / max, 2^64 - 1 and
2^64, the 10^19 chunks and their zero padding (10^19, 10^19 - 1, 2 * 10^19,
10^38 - 1, 10^38), decimals with no more digits than their scale (0.05, -0.05,
DECIMAL(18,18), DECIMAL(38,38)), and the 1- and 2-byte types.

The Arrow string getters always format on the device.  Cell-by-cell results
(duckdb_mb_query) switch from the host formatter to the text kernels at
65,536 rows (kTextRows, executor.cpp): both sides of the switch must give the
same text."""
import pytest

import vm_cases as V
import vm_reference as R
from gpu_tables import kernels, load, profiled, retable, tile
from oracle import wire

pytestmark = pytest.mark.gpu

I128 = R.INT_RANGE["HUGEINT"]
HX = [10 ** 19, 10 ** 19 - 1, 10 ** 38, 2 * 10 ** 19, -(10 ** 19), -(10 ** 38), 10 ** 19 + 1, I128[0], I128[1], 2 ** 64, 2 ** 64 - 1,
      2 ** 64 + 1, -(2 ** 64), 0, -1]
DX = [5, -5, 50, -99, 100, 0, -100, 1, -1, 99, 10 ** 9 - 1, -(10 ** 9 - 1), 101, -101, 10]
assert len(HX) == len(DX)
_ok = [k % 4 != 1 for k in range(len(HX))]
EXTRA = V.Table("tx", [V.Col("id", "BIGINT", range(len(HX))), V.Col("hx", "HUGEINT", HX), V.Col("hxn", "HUGEINT", HX, _ok),
                       V.Col("dx", "DECIMAL(9,2)", DX), V.Col("dxn", "DECIMAL(9,2)", DX, _ok)])
TABLES = {"ti": V.TABLES["ti"], "tu": V.TABLES["tu"], "th": V.TABLES["th"], "td": V.TABLES["td"], "tl": V.TABLES["tl"],
          "tx": EXTRA}
# the columns pulled through the row-count switch: every type and width once, with its NULL-able twin
SWITCH = {"ti": ["ta", "tan", "sa", "san", "ia", "ian", "ba", "ban"], "tu": ["uta", "utan", "usa", "usan", "uia", "uian", "ula", "ulan"],
          "th": ["ha", "han"], "td": ["da", "dan", "ea", "ean", "ga", "gan", "ka", "kan", "wa", "va"], "tl": ["pn", "qn"]}


def spell(c, v):
    if v is None:
        return None
    return V.dec_text(v, c.scale) if c.kind == "dec" else ("true" if v else "false") if c.kind == "bool" else str(v)


def test_the_edge_values_are_in_the_tables():
    have = lambda t, c, v: v in V.TABLES[t].cols[c].values
    assert have("ti", "ba", R.INT_RANGE["BIGINT"][0]) and have("tu", "ula", 2 ** 64 - 1) and have("tu", "ula", 2 ** 64 - 2)
    assert have("th", "ha", I128[0]) and have("th", "ha", I128[1]) and have("th", "ha", 2 ** 64) and have("th", "ha", 2 ** 64 - 1)
    assert have("td", "ka", 10 ** 38 - 1) and have("td", "va", 1) and have("td", "wa", -1)
    assert spell(EXTRA.cols["dx"], 5) == "0.05" and spell(EXTRA.cols["dx"], -5) == "-0.05" and spell(EXTRA.cols["dx"], -99) == "-0.99"


@pytest.mark.parametrize("tname", list(TABLES))
def test_arrow_string_getters(mbx, tname):
    t = TABLES[tname]
    n = len(t.cols["id"].values)
    conn = profiled(mbx)
    cols = list(t.cols)
    load(mbx, conn, t, tname, list(range(n)), cols)
    for name in cols:
        c = t.cols[name]
        vals = [spell(c, c.get(r)) for r in range(n)]
        a = conn.query_arrow(f"SELECT {name} FROM {tname}").value
        conn.profile_drain()
        for nullable in (False, True):
            got = mbx._take((mbx.lib.duckdb_mb_arrow_get_column_string_nullable if nullable else
                             mbx.lib.duckdb_mb_arrow_get_column_string)(a._h, 0))
            want = wire.string(vals, nullable)
            if got != want:
                i = next((j for j in range(min(len(got), len(want))) if got[j] != want[j]), min(len(got), len(want)))
                raise AssertionError(f"{tname}.{name} nullable={nullable} len {len(got)} vs {len(want)}, first difference at "
                                     f"byte {i}: got {got[max(0, i - 40):i + 40]!r} want {want[max(0, i - 40):i + 40]!r}")
            ran = [x["name"] for x in conn.profile_drain()]
            assert "text_lengths" in ran and "text_write" in ran, (tname, name, ran)
        a.close()
    conn.close()


@pytest.mark.parametrize("n", [65535, 66000])
@pytest.mark.parametrize("tname", list(SWITCH))
def test_row_count_switch(mbx, tname, n):
    """load()'s read-back is SELECT * pulled cell by cell: every cell against the model, on either side of kTextRows"""
    conn = profiled(mbx)
    t = retable(V.TABLES[tname], tile(n), SWITCH[tname])
    load(mbx, conn, t, "big", list(range(n)), list(t.cols))
    ran = kernels(conn)
    if n >= 65536:
        assert "text_lengths" in ran and "text_write" in ran, (tname, n, ran)
    else:
        assert "text_lengths" not in ran and "text_write" not in ran, (tname, n, ran)
    conn.close()


def test_text_after_limit_offset(mbx):
    """a result that begins in the middle of a validity word (the gather) or on a later word (the slice):
    whichever formatter takes it, the text is the same"""
    n = 66000 + 128
    conn = profiled(mbx)
    cols = ["ban", "han"]
    src = V.Table("m", list(V.TABLES["ti"].cols.values()) + [V.TABLES["th"].cols["han"]])
    t = retable(src, tile(n), cols)
    load(mbx, conn, t, "big", list(range(n)), list(t.cols))
    for off in (37, 64):
        res = conn.query_raw(f"SELECT ban, han FROM big LIMIT 66000 OFFSET {off}")
        assert res.row_count() == 66000
        text, nulls = res.cells()
        for j, name in enumerate(cols):
            c = t.cols[name]
            for k in range(66000):
                v = c.get(off + k)
                assert nulls[k][j] == (v is None) and (v is None or text[k][j] == str(v)), (off, name, k, text[k][j], v)
        res.close()
    conn.close()
