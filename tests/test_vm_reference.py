"""The expression-VM case table (vm_cases.py) against engine 1, the host
constant folder (EvalConst / CastValue in binder.cpp), and against itself:
every row of the model is reproduced by the folder when the row's inputs are
written as typed literals; every case plans onto the device; the cases reach
every VmOpc; and at least 90 % of each case's rows are usable on the device."""
import os
import re
import struct

import pytest

import vm_cases as V
import vm_reference as R
from conftest import ROOT

HOST_ROWS = list(range(300)) + list(range(300, V.N, 50))  # all edge rows, and a sample of the random ones


def _typename(mbx, res, c=0):
    return mbx.column_type_from_id(res.column_type(c))


def cell_matches(case, res, text, null, r, want):
    """one result cell (row r of column 0 of `res`) against the model's value"""
    if want is None:
        return null
    if null:
        return False
    if case.out in ("f64", "f32"):
        raw = res.raw(0, r)
        got = struct.unpack("<d", raw)[0] if len(raw) == 8 else struct.unpack("<f", raw)[0]
        if want != want:
            return got != got
        return R.bits(got) == R.bits(want)
    return text == case.text(want)


def _host_check(mbx, hostconn, case, with_literals, expect):
    ok_rows = [r for r in HOST_ROWS if expect(r)[0] == "ok"]
    bad = []
    for lo in range(0, len(ok_rows), 100):
        rows = ok_rows[lo:lo + 100]
        sql = " UNION ALL ".join(f"SELECT {with_literals(r)}" for r in rows)
        res = hostconn.query_raw(sql)
        assert res.row_count() == len(rows), sql[:200]
        assert _typename(mbx, res) == case.rtype, (case.sql, _typename(mbx, res))
        text, nulls = res.cells()
        for k, r in enumerate(rows):
            if not cell_matches(case, res, text[k][0], nulls[k][0], k, expect(r)[1]):
                bad.append((r, with_literals(r), text[k][0], nulls[k][0], expect(r)[1]))
        res.close()
    assert not bad, (case.sql, len(bad), bad[:5])
    for r in HOST_ROWS:
        st, kind = expect(r)
        if st == "err":
            got = hostconn.query(f"SELECT {with_literals(r)}")
            assert isinstance(got, mbx.Err) and got.error.message.startswith(kind + " Error"), \
                (case.sql, with_literals(r), kind, got)


@pytest.mark.parametrize("fam", V.FAMILIES)
def test_host_folder_matches_model(mbx, hostconn, fam):
    for case in V.family(fam):
        _host_check(mbx, hostconn, case, case.with_literals, case.expect)


def test_host_folder_error_cases(mbx, hostconn):
    """each error case: in range with 0, the model's error kind with 1, NULL with NULL"""
    for e in V.ERR_CASES:
        r = hostconn.query(f"SELECT {e.with_literals(0)}")
        assert isinstance(r, mbx.Ok) and r.value.nulls == [[False]], (e.name, r)
        r = hostconn.query(f"SELECT {e.with_literals(1)}")
        assert isinstance(r, mbx.Err) and r.error.message.startswith(e.kind + " Error"), (e.name, r)
        r = hostconn.query(f"SELECT {e.with_literals(None)}")
        assert isinstance(r, mbx.Ok) and r.value.nulls == [[True]], (e.name, r)


def test_defects_of_the_host_folder(mbx, hostconn):
    """the host rows of the defect table this suite was written against"""
    one = lambda sql: hostconn.query(sql)
    assert one("SELECT CAST(CAST(0.9 AS DECIMAL(38,38)) AS BIGINT)").value.rows == [["1"]]
    r = one("SELECT ABS(CAST(-170141183460469231731687303715884105728 AS HUGEINT))")
    assert isinstance(r, mbx.Err) and r.error.message.startswith("Out of Range Error")
    r = one("SELECT CAST(-170141183460469231731687303715884105728 AS HUGEINT) // -1")
    assert isinstance(r, mbx.Err) and r.error.message.startswith("Out of Range Error")
    assert one("SELECT CAST(-170141183460469231731687303715884105728 AS HUGEINT) % -1").value.rows == [["0"]]
    r = one("SELECT CAST(18446744073709551615 AS UBIGINT) + CAST(1 AS UBIGINT)")
    assert isinstance(r, mbx.Err) and r.error.message.startswith("Out of Range Error")
    # decimal -> double is double(unscaled) / 10^scale: ...326.0, not the correctly rounded ...327.0
    res = hostconn.query_raw("SELECT CAST(CAST('8176441668080326.8' AS DECIMAL(18,1)) AS DOUBLE), "
                             "CAST(CAST(27670116110564329473 AS HUGEINT) AS DOUBLE)")
    assert struct.unpack("<d", res.raw(0, 0))[0] == float(81764416680803268) / 10.0 == 8176441668080326.0
    assert struct.unpack("<d", res.raw(1, 0))[0] == float(27670116110564329473) == 27670116110564331520.0


def _tables(hostconn):
    from conftest import q
    for t in V.TABLES.values():
        if t.source == t.name:
            q(hostconn, t.ddl())


def test_every_case_plans_onto_the_device(hostconn):
    _tables(hostconn)
    for c in V.CASES + V.ERR_CASES:
        src = c.table.source if isinstance(c, V.Case) else "te"
        plan = hostconn.explain(f"SELECT {c.sql} FROM {src}")
        assert plan.rstrip().endswith("[device]"), (c.sql, plan)
        # the operators and cast targets the case is about are in the bound plan
        for sym in re.findall(r" (//|[-+*/%]|<>|<=|>=|=|<|>|AND|OR|IS NOT DISTINCT FROM|IS DISTINCT FROM) ", c.sql):
            assert f" {'!=' if sym == '<>' else sym} " in plan, (c.sql, sym, plan)  # the plan spells <> as !=
        for t in re.findall(r" AS ([A-Z]+(?:\(\d+,\d+\))?)\)", c.sql):
            assert f"AS {t}" in plan, (c.sql, t, plan)
        if isinstance(c, V.Case) and c.is_bool:
            plan = hostconn.explain(f"SELECT id FROM {src} WHERE {c.sql}" if "id" in c.table.cols
                                    else f"SELECT i FROM {src} WHERE {c.sql}")
            assert plan.rstrip().endswith("[device]"), (c.sql, plan)


def test_cases_reach_every_opcode():
    src = open(os.path.join(ROOT, "duckdb.mbt_amd", "csrc", "vm.h")).read()
    body = re.search(r"enum VmOpc : uint8_t \{(.*?)\};", src, re.S).group(1)
    body = re.sub(r"//[^\n]*", "", body)
    opcodes = set(re.findall(r"\b(V_[A-Z0-9_]+)\b", body))
    assert len(opcodes) > 50
    declared = {o for c in V.CASES + V.ERR_CASES for o in c.ops}
    assert declared - opcodes == set(), declared - opcodes
    assert opcodes - declared == {"V_NOP", "V_MOV"}, sorted(opcodes - declared)  # the compiler never emits these two


def test_nine_tenths_of_every_case_are_usable():
    for c in V.CASES:
        ok = sum(1 for r in range(V.N) if c.expect(r)[0] == "ok")
        assert ok >= 0.9 * V.N, (c.sql, ok)
    for e in V.ERR_CASES:  # exactly one raising row, inside a tile
        assert 256 < V.ERR_ROW < 512 and V.ERR_ROW % 256 not in (0, 255)


def test_model_primitives():
    assert (R.div(-7, 2), R.mod(-7, 2), R.div(7, -2), R.mod(7, -2)) == (-3, -1, -3, 1)
    assert [R.round_half_away_div(v, 10) for v in (5, -5, 4, -4, 15, -15, 14)] == [1, -1, 0, 0, 2, -2, 1]
    assert R.round_half_away_div(9 * 10 ** 37, 10 ** 38) == 1
    assert [R.f_to_int(x, "BIGINT") for x in (0.5, 1.5, 2.5, -2.5, -0.5)] == [0, 2, 2, -2, 0]
    assert R.cmp3(float("nan"), float("inf")) == 1 and R.cmp3(float("nan"), float("nan")) == 0 and R.cmp3(-0.0, 0.0) == 0
    assert (R.and3(None, False), R.and3(None, True), R.or3(None, True), R.or3(None, False)) == (False, None, True, None)
    assert R.distinct(None, None) is False and R.distinct(None, 1) is True
    assert R.dec_to_f64(81764416680803268, 1) == 8176441668080326.0
    with pytest.raises(R.VmError):
        R.abs_("HUGEINT", -2 ** 127)
    with pytest.raises(R.VmError):
        R.add("UBIGINT", 2 ** 64 - 1, 1)
