"""Aggregates of DOUBLE, FLOAT, HUGEINT, DECIMAL(38,2) and UBIGINT values on every
path that takes them: the generic kernels (reduce_column with reduce_minmax128,
group_assign / hash_group_assign with group_reduce and group_minmax128), the
float and 128-bit branches of jit_aggregate, the join's fused aggregate and its
materialised fall-back, COUNT(DISTINCT) and the shard combine.  The fast paths
take only BIGINT and INTEGER arguments, which the other aggregate suites feed.

Every statement computes COUNT(*), COUNT(v), SUM(v), MIN(v), MAX(v) and AVG(v)
and is compared with agg_model (exact integers, Fractions, math.fsum) over the
same Python values, never with another connection of the engine:
  * counts, and SUM / MIN / MAX of the integer classes, exactly, as text;
  * MIN / MAX of DOUBLE and FLOAT by bit pattern: one of the tying inputs
    (either zero where -0.0 and 0.0 tie, any NaN where NaN wins);
  * SUM of DOUBLE and FLOAT exactly where the model says NaN or +-inf, else
    within 1e-9 * sum|x| of fsum ("Floating-point sums"), AVG
    within that over the count; AVG of the integer classes within 1e-9 relative
    of the Fraction ("Aggregate types").
The sum|x| of a group is below 1e300 in every column but dx (asserted on the
inputs), so no partial sum can overflow in any order; dx adds a handful of
+-1e300 for MIN / MAX, its sum|x| stays below 1e305, which still cannot overflow.

Tables load through the columnar appender (gpu_tables.load reads every cell
back), float cells are read as raw bytes, and every statement's kernel list is
pinned (KERNELS), so no case can move to another path unnoticed.  Sizes: 1, 63,
64, 65 and 257 rows for the wave and validity-word edges, 4 099 for several
workgroups with a ragged last wave; the hashed, join and sharded cases run at
4 099 only."""
import functools
import math
import struct
from fractions import Fraction

import pytest

import agg_model as M
import vm_cases as V
import vm_reference as R
from conftest import q
from gpu_tables import kernels, load

pytestmark = pytest.mark.gpu

N = 4_099
SIZES = [1, 63, 64, 65, 257, N]
INF, NAN, NEG_NAN = math.inf, math.nan, R.from_bits(0xFFF8000000000001)
SUB = 5e-324
U63 = 2 ** 63


# ---- the table --------------------------------------------------------------------------------
def key7(r):
    """the INTEGER key of range 7: runs of three rows, so that a NULL mask (one residue of r mod 7)
    takes rows out of every group"""
    return (r // 3) % 7


def ordinary(r):
    """mixed sign, 1e-3 .. 2e12"""
    return (-1.0 if r % 3 == 1 else 1.0) * (1 + (r * 37 % 1000) / 1000) * 10.0 ** ((r * 13) % 16 - 3)


def d_val(r):
    return [SUB, -SUB, 0.0, -0.0][(r // 5) % 4] if r % 5 == 0 else ordinary(r)


def dx_val(r):
    if r % 5 == 1 and (r // 5) % 50 == 0:
        return 1e300 if (r // 250) % 2 == 0 else -1e300
    return d_val(r)


def dn_val(r):
    """NaNs in groups 1, 5 and 6 only: the other groups' sums are finite.  Groups 1 and 5 hold both the
    positive quiet NaN and the negative one with a payload, group 6 only the negative one (whose bits, read
    as a number, would sort below -inf)"""
    g = key7(r)
    if r % 5 == 0 and g in (1, 5, 6):
        return NEG_NAN if g == 6 or (r // 5) % 2 else NAN
    return d_val(r)


def dni_val(r):
    """as dn, with +inf in group 2, -inf in group 3, both in group 4 and beside the NaNs of group 5"""
    g = key7(r)
    if r % 5 == 0 and g in (2, 3, 4):
        return INF if g == 2 or (g == 4 and (r // 5) % 2 == 0) else -INF
    if r % 5 == 0 and g == 5 and (r // 5) % 3 == 0:
        return INF
    return dn_val(r)


def dc_col(n):
    """1e16 in the first third, 1.0 in the second, -1e16 in the last: the three that cancel sit in
    different waves and, from 4 099 rows on, in different workgroups"""
    t = n // 3
    return [1e16 if r < t else 1.0 if r < 2 * t else -1e16 if r < 3 * t else 0.5 for r in range(n)]


F32_EDGES = [16777216.0, 16777218.0, 16777215.0, -0.0, 0.0, R.f32(1e-45), -16777216.0, R.f32(0.1)]


def ff_val(r):
    return F32_EDGES[(r // 5) % len(F32_EDGES)] if r % 5 == 0 else R.f32(ordinary(r))


def f_val(r):
    x = dni_val(r)
    return x if x != x or math.isinf(x) else ff_val(r)


H_EDGES = [2 ** 64 - 1, -2 ** 64, 0, -1, 2 ** 64, -2 ** 64 - 1,
           # the same low word under seven high words, and one high word over low words on both sides of 2^63
           (-3 << 64) + 77, (-2 << 64) + 77, (-1 << 64) + 77, 77, (1 << 64) + 77, (2 << 64) + 77, (3 << 64) + 77,
           (5 << 64) + 1, (5 << 64) + U63 - 1, (5 << 64) + U63, (5 << 64) + 2 ** 64 - 1,
           (-5 << 64) + 1, (-5 << 64) + U63 - 1, (-5 << 64) + U63, (-5 << 64) + 2 ** 64 - 1]


def h_val(r):
    """one +(2^126 - 0) and one -(2^126 - 1) in the whole column, so that no subset's sum leaves HUGEINT"""
    if r == 0:
        return 2 ** 126
    if r == 8:
        return -(2 ** 126 - 1)
    s = -1 if (r // 4) % 2 else 1
    return [s * (2 ** 100 + r), s * (2 ** 64 + r), H_EDGES[(r // 4) % len(H_EDGES)], s * r][r % 4]


def m_val(r):
    """DECIMAL(38,2), unscaled: the HUGEINT values in another phase (|v| <= 2^126 < 10^38), small ones for r % 4 = 3"""
    if r in (0, 8):
        return h_val(r)
    return [-1, 1, 250, -99][(r // 4) % 4] if r % 4 == 3 else h_val(r + 1)


U_EDGES = [0, 1, U63 - 1, U63, U63 + 1, 2 ** 64 - 1]


def u_val(r):
    return U_EDGES[(r * 7 + r // 7) % 6] if r % 4 else (r * 2654435761) % 2 ** 64


KD = [0.0, -0.0, NAN, NEG_NAN, INF, -INF, SUB, 1.5, -2.5]  # the DOUBLE key: seven groups (one zero, one NaN)
VALUE_COLS = {"d": "DOUBLE", "dx": "DOUBLE", "dn": "DOUBLE", "dni": "DOUBLE", "dc": "DOUBLE", "f": "FLOAT",
              "ff": "FLOAT", "h": "HUGEINT", "m": "DECIMAL(38,2)", "u": "UBIGINT"}
GEN = {"d": d_val, "dx": dx_val, "dn": dn_val, "dni": dni_val, "f": f_val, "ff": ff_val, "h": h_val, "m": m_val,
       "u": u_val}
SUM_LIMIT = {"dx": 1e305}  # sum|x| of any set of rows stays below this; 1e300 for every other column
ALL_COLS = [v + sfx for v in VALUE_COLS for sfx in ("", "_n")]


def _mask(j, n):
    m = V.null_mask(j)
    return [m[r % V.N] for r in range(n)]


@functools.lru_cache(maxsize=None)
def table(n):
    """n rows: id, the keys, w (the WHERE column) and every value column with its NULL-able twin, whose
    rows of group 3 are all NULL"""
    rows = range(n)
    cols = [V.Col("id", "BIGINT", rows),
            V.Col("k", "INTEGER", [key7(r) for r in rows]),
            V.Col("kn", "INTEGER", [key7(r) for r in rows], _mask(11, n)),
            V.Col("w", "BIGINT", [(r * 17) % 1000 for r in rows]),
            V.Col("kd", "DOUBLE", [KD[(r * 5 + r // 9) % len(KD)] for r in rows]),
            V.Col("ka", "BIGINT", [r % 3 - 1 for r in rows]),
            V.Col("kb", "BIGINT", [((r // 3) % 5) * 10 ** 10 for r in rows]),
            V.Col("kw", "BIGINT", [((r * 7) % 2000) * 1000003 for r in rows]),
            V.Col("hw", "HUGEINT", [((r % 9 - 4) << 64) + 77 for r in rows])]
    for j, (name, t) in enumerate(VALUE_COLS.items()):
        vals = dc_col(n) if name == "dc" else [GEN[name](r) for r in rows]
        cols.append(V.Col(name, t, vals))
        cols.append(V.Col(name + "_n", t, vals, [ok and key7(r) != 3 for r, ok in zip(rows, _mask(j, n))]))
    return V.Table("t", cols)


def kind_of(col):
    return "f64" if col.kind in ("f64", "f32") else "int"


def cls(col):
    return {"DOUBLE": "f64", "FLOAT": "f32", "HUGEINT": "i128", "UBIGINT": "u64"}.get(col.sqltype, "dec128")


def ident(col):
    """what the kernel lists depend on: the value class and whether the column has a validity bitmap"""
    return cls(col) + ("?" if not all(col.valid) else "")


# ---- the kernel lists, as the build before the grouped 128-bit MIN / MAX fix reported them ---------
# One entry per aggregate with an argument: the second pass of a 128-bit MIN / MAX runs inside its
# reduce_column entry (and, since the fix, inside its group_reduce entry), so it adds no name.
RC5, GR5 = 5 * ["reduce_column"], 5 * ["group_reduce"]
JOIN = ["join_keys", "radix_sort", "join_build"]
PAIRS = JOIN + ["join_probe_count", "join_expand", "join_gather"]
CLASSES = ("f64", "f32", "i128", "dec128", "u64")


def _kernel_lists():
    K = {}
    for k in CLASSES:
        for nl in ("", "?"):
            f32 = k == "f32"  # a FLOAT argument is widened by a projection, which also does the filtering
            compact = ["compact"] * (3 if k in ("i128", "dec128") else 2) + (["compact_validity"] * 5 if nl else [])
            K[f"global:{k}{nl}:all"] = (["vm_project"] if f32 else []) + RC5
            K[f"global:{k}{nl}:where"] = (["vm_filter", "vm_project"] if f32 else ["filter_bits"] + compact) + RC5
            K[f"global:{k}{nl}:none"] = (["vm_filter"] if f32 else ["filter_bits"]) + RC5
            project = ["vm_project"] if f32 else []
            K[f"slot:{k}{nl}"] = project + ["group_assign"] + GR5
            for path in ("hash_varchar", "hash_double", "hash_two_keys", "hash_wide"):
                K[f"{path}:{k}{nl}"] = project + ["hash_group_assign"] + GR5
            # the fused probe takes DOUBLE arguments and declines a 128-bit MIN / MAX
            K[f"join_fused:{k}{nl}"] = JOIN + ["join_probe_agg", "join_agg_fold"] if k == "f64" else PAIRS + RC5
            K[f"join_plain:{k}{nl}"] = PAIRS + RC5
            # a GROUP BY over a join reduces the materialised pairs on either connection
            K[f"join_grouped:{k}{nl}"] = PAIRS + project + ["group_assign"] + GR5
            # two shards: AVG travels as SUM and COUNT, so six states per column and shard
            K[f"sharded:{k}{nl}"] = 2 * (["group_assign"] + 6 * ["group_reduce"])
            K[f"sharded_global:{k}{nl}"] = 12 * ["reduce_column"]
    K["sharded:three"] = 2 * (["group_assign"] + 12 * ["group_reduce"])
    K["join_fused:repeat"] = JOIN + ["join_probe_agg", "join_agg_fold"]
    # COUNT(DISTINCT v), COUNT(v): the distinct values by the hash table, counted in LDS where they are few
    for v, few in (("kd", True), ("hw", True), ("dn", False), ("dni_n", False), ("h_n", False)):
        K[f"distinct:{v}"] = 2 * ["reduce_column"] + ["hash_group_assign"] + few * ["group_direct"] + ["reduce_column"]
    K["distinct:grouped"] = ["group_assign", "group_reduce", "hash_group_assign", "group_assign", "group_reduce",
                             "radix_sort"]
    for k in ("jit:f64:all", "jit:f64:where", "jit:f32:all", "jit:wide_sums:where"):
        K[k] = ["jit_aggregate"]
    K["jit:i128:declined"] = RC5  # (a statement the compiler declines leaves no entry of its own)
    return K


KERNELS = _kernel_lists()


def pin(c, name):
    assert kernels(c) == KERNELS[name], (name, kernels(c))


# ---- statements and their check ---------------------------------------------------------------------
def aggs(names, avg=True):
    return "COUNT(*), " + ", ".join(f"COUNT({v}), SUM({v}), MIN({v}), MAX({v})" + (f", AVG({v})" if avg else "")
                                    for v in names)


def _float(raw):
    return struct.unpack("<d", raw)[0] if len(raw) == 8 else struct.unpack("<f", raw)[0]


def _near(got, want, tol, where):
    """got against the model's double `want` (a Fraction where finite): exact for NaN / inf, else within tol"""
    if isinstance(want, float) and want != want:
        assert got != got, where + (got,)
    elif isinstance(want, float) and math.isinf(want):
        assert got == want, where + (got, want)
    else:
        assert math.isfinite(got), where + (got, want)
        assert abs(Fraction(got) - Fraction(want)) <= tol, where + (got, float(want), float(tol))


def check_block(col, st, text, nulls, raw, j, where, avg=True):
    """COUNT(v), SUM, MIN, MAX [, AVG] at result columns j .. j + 4 against the group's Stats"""
    w = 5 if avg else 4
    assert not nulls[j] and text[j] == str(st.count), where + ("count", text[j], st.count)
    if st.count == 0:
        assert nulls[j + 1:j + w] == [True] * (w - 1), where + ("not NULL", text[j + 1:j + w])
        return
    assert not any(nulls[j + 1:j + w]), where + ("NULL", nulls[j + 1:j + w])
    if kind_of(col) == "int":
        fmt = (lambda v: V.dec_text(v, col.scale)) if col.kind == "dec" else str
        for o, (what, want) in enumerate((("sum", st.sum), ("min", st.min), ("max", st.max)), 1):
            assert text[j + o] == fmt(want), where + (what, text[j + o], fmt(want))
        if avg:
            assert len(raw(j + 4)) == 8, where
            _near(_float(raw(j + 4)), st.avg, abs(st.avg) / 10 ** 9, where + ("avg",))
        return
    tol = Fraction(st.abs_sum) / 10 ** 9
    _near(_float(raw(j + 1)), st.sum if st.sum != st.sum or math.isinf(st.sum) else Fraction(st.sum), tol, where + ("sum",))
    if avg:
        want = st.avg if st.sum != st.sum or math.isinf(st.sum) else Fraction(st.sum) / st.count
        _near(_float(raw(j + 4)), want, tol / st.count, where + ("avg",))
    for o, what, want in ((2, "min", st.min), (3, "max", st.max)):
        b = raw(j + o)
        assert len(b) == (4 if col.kind == "f32" else 8), where + (what, b)  # MIN / MAX keep the input type
        got = _float(b)
        assert (M.NAN in want) if got != got else (R.bits(got) in want), where + (what, got, R.bits(got), want)


def check_sums_cannot_overflow(col, groups):
    for st in groups.values():
        if st.abs_sum is not None:
            assert st.abs_sum < SUM_LIMIT.get(col.name.replace("_n", ""), 1e300), (col.name, st.abs_sum)


def run(c, t, n, names, keys=(), where=None, keep=None, source="t", mult=None, avg=True):
    """SELECT keys, COUNT(*), the five aggregates of each named column (four with avg=False) FROM source
    [WHERE where] [GROUP BY keys] against the model over rows 0 .. n-1 of table t (keep: the WHERE as a row
    predicate; mult: how many times the source repeats a row, for a join).  Returns the result's key set."""
    cols = [t.cols[v] for v in names]
    kcols = [t.cols[k.split(".")[-1]] for k in keys]
    sql = "SELECT " + ", ".join(list(keys) + [aggs(names, avg)]) + f" FROM {source}" + (f" WHERE {where}" if where else "") + \
        (" GROUP BY " + ", ".join(keys) if keys else "")
    rows = [r for r in range(n) if keep is None or keep(r) for _ in range(1 if mult is None else mult(r))]
    model = []
    for col in cols:
        pairs = [(tuple(kc.get(r) for kc in kcols), col.get(r)) for r in rows]
        groups = M.aggregate(pairs, kind_of(col), col.scale)
        if not keys and not groups:  # no GROUP BY: one row, even over no rows
            groups = {(): M.stats([], kind_of(col))}
        check_sums_cannot_overflow(col, groups)
        model.append(groups)
    res = c.query_raw(sql)
    try:
        text, nulls = res.cells()
        nk = len(keys)
        got = {}
        for i in range(res.row_count()):
            key = []
            for g, kc in enumerate(kcols):
                if nulls[i][g]:
                    key.append(None)
                elif kc.kind == "f64":
                    assert len(res.raw(g, i)) == 8
                    key.append(M.key_of(_float(res.raw(g, i))))
                else:
                    key.append(int(text[i][g]) if kc.kind == "int" else text[i][g])
            assert tuple(key) not in got, (sql, "group twice", key)
            got[tuple(key)] = i
        assert set(got) == set(model[0]), (sql, sorted(map(str, got)), sorted(map(str, model[0])))
        for key, i in got.items():
            where_ = (sql, n, key)
            assert not nulls[i][nk] and text[i][nk] == str(model[0][key].count_star), where_ + ("count(*)", text[i][nk])
            for b, col in enumerate(cols):
                check_block(col, model[b][key], text[i], nulls[i], lambda j, i=i: res.raw(j, i),
                            nk + 1 + (5 if avg else 4) * b, where_, avg)
        return set(got)
    finally:
        res.close()


def connect(mbx, **opts):
    cfg = mbx.Config.create()
    for k, v in dict(mbx_profile="true", **opts).items():
        assert isinstance(cfg.set(k, str(v)), mbx.Ok), (k, v)
    r = mbx.connect_with_config(cfg)
    assert isinstance(r, mbx.Ok), r.error.message
    return r.value


def loaded(mbx, n, cols, **opts):
    c = connect(mbx, **opts)
    t = table(n)
    load(mbx, c, t, "t", list(range(n)), cols)
    return c, t


W_HALF = ("w < 500", lambda r: (r * 17) % 1000 < 500)
W_NONE = ("w < 0", lambda r: False)


# ---- global: reduce_column ---------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
def test_global_reduce_column(mbx, monkeypatch, n):
    monkeypatch.setenv("MBX_JIT", "0")
    c, t = loaded(mbx, n, ["w"] + ALL_COLS)
    for v in ALL_COLS:
        run(c, t, n, [v])
        pin(c, f"global:{ident(t.cols[v])}:all")
        run(c, t, n, [v], where=W_HALF[0], keep=W_HALF[1])
        pin(c, f"global:{ident(t.cols[v])}:where")
        run(c, t, n, [v], where=W_NONE[0], keep=W_NONE[1])
        pin(c, f"global:{ident(t.cols[v])}:none")
    c.close()


# ---- global: jit_aggregate -----------------------------------------------------------------------------
def test_global_jit_aggregate(mbx, monkeypatch):
    monkeypatch.setenv("MBX_JIT", "sync")
    c, t = loaded(mbx, N, ["w", "d", "dni_n", "f_n", "h", "h_n", "u_n"])
    run(c, t, N, ["d"])
    pin(c, "jit:f64:all")
    run(c, t, N, ["dni_n"], where=W_HALF[0], keep=W_HALF[1])
    pin(c, "jit:f64:where")
    run(c, t, N, ["f_n"])
    pin(c, "jit:f32:all")
    # SUM, AVG and COUNT of 128-bit values are compiled ...
    rows = [r for r in range(N) if W_HALF[1](r)]
    h, u = M.stats([t.cols["h_n"].get(r) for r in rows], "int"), M.stats([t.cols["u_n"].get(r) for r in rows], "int")
    res = c.query_raw("SELECT COUNT(*), COUNT(h_n), SUM(h_n), AVG(h_n), COUNT(u_n), SUM(u_n), AVG(u_n) FROM t WHERE w < 500")
    pin(c, "jit:wide_sums:where")
    text, nulls = res.cells()
    assert text[0][:3] == [str(len(rows)), str(h.count), str(h.sum)] and not any(nulls[0]), text
    assert [text[0][4], text[0][5]] == [str(u.count), str(u.sum)], text
    _near(_float(res.raw(3, 0)), h.avg, abs(h.avg) / 10 ** 9, ("avg(h_n)",))
    _near(_float(res.raw(6, 0)), u.avg, abs(u.avg) / 10 ** 9, ("avg(u_n)",))
    res.close()
    # ... a 128-bit MIN is not: the statement declines to reduce_column and is still right
    run(c, t, N, ["h"])
    pin(c, "jit:i128:declined")
    c.close()


# ---- grouped: group_assign + group_reduce -----------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
def test_group_assign_reduce(mbx, monkeypatch, n):
    monkeypatch.setenv("MBX_JIT", "0")
    c, t = loaded(mbx, n, ["k", "kn"] + ALL_COLS)
    for v in ALL_COLS:
        for key in ("k", "kn"):
            seen = run(c, t, n, [v], keys=[key])
            pin(c, f"slot:{ident(t.cols[v])}")
            if n == N:
                assert len(seen) == (7 if key == "k" else 8)  # the NULL group
    c.close()


def test_group_whose_values_are_all_null(mbx, monkeypatch):
    """group 3 of every NULL-able column: the counts, and NULL for the rest (run() requires it of every
    statement; here it is said aloud, on the inputs)"""
    monkeypatch.setenv("MBX_JIT", "0")
    t = table(N)
    for v in ("dn_n", "h_n", "u_n"):
        assert all(t.cols[v].get(r) is None for r in range(N) if key7(r) == 3)
        assert M.aggregate([(key7(r), t.cols[v].get(r)) for r in range(N)], kind_of(t.cols[v]))[3].count == 0
    c, t = loaded(mbx, N, ["k", "dn_n", "h_n", "u_n"])
    for v in ("dn_n", "h_n", "u_n"):
        res = c.query_raw(f"SELECT k, {aggs([v])} FROM t WHERE k = 3 GROUP BY k")
        text, nulls = res.cells()
        assert text == [["3", str(sum(1 for r in range(N) if key7(r) == 3)), "0", "", "", "", ""]], text
        assert nulls == [[False, False, False, True, True, True, True]], nulls
        res.close()
    c.close()


# ---- grouped: hash_group_assign + group_reduce -----------------------------------------------------------
def test_hash_varchar_key(mbx, monkeypatch):
    monkeypatch.setenv("MBX_JIT", "0")
    c, t = loaded(mbx, N, ["id"] + ALL_COLS)
    names = ["ash", "birch", "cedar", "date", "elm"]
    case = "CASE " + " ".join(f"WHEN (id // 7) % 5 = {i} THEN '{s}'" for i, s in enumerate(names)) + " END"
    q(c, f"CREATE TABLE ts AS SELECT {case} AS s, " + ", ".join(ALL_COLS) + " FROM t")
    ts = V.Table("ts", [V.Col("s", "VARCHAR", [names[(r // 7) % 5] for r in range(N)])] + [t.cols[v] for v in ALL_COLS])
    ts.cols["s"].kind = "str"
    for v in ALL_COLS:
        assert len(run(c, ts, N, [v], keys=["s"], source="ts")) == 5
        pin(c, f"hash_varchar:{ident(t.cols[v])}")
    c.close()


def test_hash_double_key_and_two_bigint_keys(mbx, monkeypatch):
    monkeypatch.setenv("MBX_JIT", "0")
    c, t = loaded(mbx, N, ["kd", "ka", "kb", "dn", "dni_n", "h", "h_n", "m_n", "u", "u_n"])
    for v in ("dn", "dni_n", "h", "m_n", "u_n"):
        # -0.0 and 0.0 are one group, and so are the two NaNs
        assert run(c, t, N, [v], keys=["kd"]) == {(0.0,), (M.NAN,), (INF,), (-INF,), (SUB,), (1.5,), (-2.5,)}
        pin(c, f"hash_double:{ident(t.cols[v])}")
    # the group-code path refuses a DOUBLE (and a 128-bit) argument: the hash path answers
    for v in ("dn", "dni_n", "h_n", "u"):
        assert len(run(c, t, N, [v], keys=["ka", "kb"])) == 15
        pin(c, f"hash_two_keys:{ident(t.cols[v])}")
    c.close()


def test_hash_2000_groups(mbx, monkeypatch):
    monkeypatch.setenv("MBX_JIT", "0")
    c, t = loaded(mbx, N, ["kw"] + ALL_COLS)
    for v in ALL_COLS:
        assert len(run(c, t, N, [v], keys=["kw"])) == 2000
        pin(c, f"hash_wide:{ident(t.cols[v])}")
    c.close()


# ---- DOUBLE and HUGEINT under COUNT(DISTINCT) --------------------------------------------------------------
def test_count_distinct(mbx, monkeypatch):
    monkeypatch.setenv("MBX_JIT", "0")
    c, t = loaded(mbx, N, ["k", "kd", "dn", "dni_n", "hw", "h_n"])
    assert M.count_distinct(t.cols["kd"].values) == 7 and M.count_distinct(t.cols["hw"].values) == 9
    for v in ("kd", "dn", "dni_n", "hw", "h_n"):
        vals = [t.cols[v].get(r) for r in range(N)]
        assert q(c, f"SELECT COUNT(DISTINCT {v}), COUNT({v}) FROM t").rows == \
            [[str(M.count_distinct(vals)), str(sum(x is not None for x in vals))]], v
        pin(c, f"distinct:{v}")
    want = {}
    for r in range(N):
        want.setdefault(key7(r), []).append(t.cols["dni_n"].get(r))
    got = q(c, "SELECT k, COUNT(DISTINCT dni_n) FROM t GROUP BY k ORDER BY k").rows
    assert got == [[str(g), str(M.count_distinct(want[g]))] for g in range(7)]
    pin(c, "distinct:grouped")
    c.close()


# ---- aggregates over an inner join ----------------------------------------------------------------------------
# dim: keys 0 .. 4 (groups 5 and 6 find no partner), key 1 twice.  Not key 0 or 2: the rows of +-2^126 are
# in those groups, and twice 2^126 is one more than HUGEINT holds.
DIM = "CREATE TABLE dim AS SELECT CAST(CASE WHEN i = 5 THEN 1 ELSE i END AS INTEGER) AS k, i AS x FROM range(6) tbl(i)"
JOIN_COLS = ["dn", "dni_n", "dc", "h", "h_n", "m_n", "u", "u_n"]


def dim_mult(t, key):
    return lambda r: {0: 1, 1: 2, 2: 1, 3: 1, 4: 1}.get(t.cols[key].get(r), 0)  # (a NULL key meets nothing)


def joined(mbx, cols):
    """the two connections of test_gpu_join_agg.py, fused and materialising, with t and dim"""
    out = []
    for opts in (dict(mbx_join_agg="true", mbx_join_agg_max_run=8), dict(mbx_join_agg="false")):
        c, t = loaded(mbx, N, cols, **opts)
        q(c, DIM)
        out.append(c)
    return out[0], out[1], t


@pytest.mark.parametrize("v", JOIN_COLS)
def test_join_global(mbx, monkeypatch, v):
    monkeypatch.setenv("MBX_JIT", "0")
    fused, plain, t = joined(mbx, ["kn", v])
    for c, name in ((fused, "fused"), (plain, "plain")):
        run(c, t, N, [v], source="t JOIN dim ON t.kn = dim.k", mult=dim_mult(t, "kn"))
        pin(c, f"join_{name}:{ident(t.cols[v])}")
        c.close()


def test_join_fused_double_sums_repeat(mbx, monkeypatch):
    """the fused probe merges its partials in a fixed order; the atomic paths promise no such thing"""
    monkeypatch.setenv("MBX_JIT", "0")
    fused, plain, t = joined(mbx, ["k", "dn", "dc", "dni_n"])
    for v in ("dn", "dc", "dni_n"):
        bits = []
        for _ in range(3):
            res = fused.query_raw(f"SELECT SUM({v}) FROM t JOIN dim ON t.k = dim.k WHERE t.k <> 1")
            bits.append(res.raw(0, 0))
            res.close()
            pin(fused, "join_fused:repeat")
        assert len(bits[0]) == 8 and bits[0] == bits[1] == bits[2], (v, bits)
    fused.close()
    plain.close()


def test_join_grouped_wide_min_max(mbx, monkeypatch):
    """a GROUP BY over a join reduces the materialised pairs on both connections"""
    monkeypatch.setenv("MBX_JIT", "0")
    cols = ["h", "h_n", "m_n", "u", "u_n", "dni_n"]
    fused, plain, t = joined(mbx, ["k"] + cols)
    for c in (fused, plain):
        for v in cols:
            seen = run(c, t, N, [v], keys=["t.k"], source="t JOIN dim ON t.k = dim.k", mult=dim_mult(t, "k"))
            assert seen == {(g,) for g in range(5)}
            pin(c, f"join_grouped:{ident(t.cols[v])}")
        c.close()


# ---- sharded ---------------------------------------------------------------------------------------------------
def test_sharded_group_by(mbx, monkeypatch):
    """two shards of 2 048 and 2 051 rows on one device, combined on the host: one statement over dn, h and u
    (without the AVGs: with them it has more aggregates than a shard takes), then each column with its AVG,
    against the model"""
    monkeypatch.setenv("MBX_JIT", "0")
    c, t = loaded(mbx, N, ["kn", "dni_n", "h_n", "u"], gpu_devices="0,0", mbx_shard_rows=2048)
    assert len(run(c, t, N, ["dni_n", "h_n", "u"], keys=["kn"], avg=False)) == 8
    pin(c, "sharded:three")
    for v in ("dni_n", "h_n", "u"):
        run(c, t, N, [v], keys=["kn"])
        pin(c, f"sharded:{ident(t.cols[v])}")
        run(c, t, N, [v])
        pin(c, f"sharded_global:{ident(t.cols[v])}")
    c.close()
