"""The case table of the expression-VM tests: input tables, one Case per SQL
expression with its exact model (vm_reference) and the VmOpc names it is meant
to reach, and the error cases.  Used by test_vm_reference.py (host folder) and
test_gpu_vm_ops.py (tile interpreter and run-time compiled kernels)."""
import itertools
import math
import re

import numpy as np

import vm_reference as R

N = 1000  # three full 256-row tiles and a 232-row tail
I64 = R.INT_RANGE["BIGINT"]
I128 = R.INT_RANGE["HUGEINT"]


class Col:
    """name, SQL type, values (Python ints / floats; DECIMAL: unscaled), valid flags"""

    def __init__(self, name, sqltype, values, valid=None):
        self.name, self.sqltype, self.values = name, sqltype, list(values)
        self.valid = list(valid) if valid is not None else [True] * len(self.values)
        m = re.match(r"DECIMAL\((\d+),(\d+)\)", sqltype)
        self.width, self.scale = (int(m.group(1)), int(m.group(2))) if m else (0, 0)
        self.kind = "dec" if m else "f64" if sqltype == "DOUBLE" else "f32" if sqltype == "FLOAT" else \
            "bool" if sqltype == "BOOLEAN" else "int"

    def get(self, r):
        return self.values[r] if self.valid[r] else None

    def numpy(self):
        """the column in its physical layout (what append_column takes)"""
        t = self.sqltype
        if self.kind == "f64":
            return np.array([R.bits(v) for v in self.values], dtype=np.uint64)
        if self.kind == "f32":
            return np.array(self.values, dtype=np.float32)
        if self.kind == "bool":
            return np.array(self.values, dtype=np.uint8)
        if self.kind == "dec":
            dt = np.int16 if self.width <= 4 else np.int32 if self.width <= 9 else np.int64 if self.width <= 18 else None
        else:
            dt = {"TINYINT": np.int8, "SMALLINT": np.int16, "INTEGER": np.int32, "BIGINT": np.int64,
                  "UTINYINT": np.uint8, "USMALLINT": np.uint16, "UINTEGER": np.uint32, "UBIGINT": np.uint64,
                  "HUGEINT": None, "DATE": np.int32, "TIMESTAMP": np.int64}[t]  # days / microseconds
        if dt is None:  # 128 bits: low word, high word
            return np.array([[v & (2 ** 64 - 1), (v >> 64) & (2 ** 64 - 1)] for v in self.values], dtype=np.uint64)
        return np.array(self.values, dtype=dt)

    def literal(self, r):
        """row r as a typed SQL literal (the host folder's input)"""
        v = self.get(r)
        if v is None:
            return f"CAST(NULL AS {self.sqltype})"
        if self.kind in ("f64", "f32"):
            s = "nan" if v != v else ("inf" if v > 0 else "-inf") if math.isinf(v) else repr(v)
            return f"CAST('{s}' AS {self.sqltype})"
        if self.kind == "dec":
            return f"CAST('{dec_text(v, self.scale)}' AS {self.sqltype})"
        if self.kind == "bool":
            return "true" if v else "false"
        return f"CAST({v} AS {self.sqltype})"


def dec_text(raw, scale):
    if scale == 0:
        return str(raw)
    a = abs(raw)
    return ("-" if raw < 0 else "") + f"{a // 10 ** scale}.{a % 10 ** scale:0{scale}d}"


class Table:
    def __init__(self, name, cols, source=None):
        self.name, self.cols = name, {c.name: c for c in cols}
        self.source = source or name  # FROM clause

    def ddl(self):
        return f"CREATE TABLE {self.name} (" + ", ".join(f"{c.name} {c.sqltype}" for c in self.cols.values()) + ")"

    def row(self, r):
        return {k: c.get(r) for k, c in self.cols.items()}


def pairs(core, extras=()):
    """every pair of the core edge values, and each extra against 1, -1, 0 and itself"""
    p = list(itertools.product(core, core))
    for x in extras:
        p += [(x, 1), (x, -1), (x, 0), (x, x), (1, x), (-1, x)]
    return p


def null_mask(k):
    """about one row in seven NULL, a different seventh for every column"""
    return [(r * 5 + 3 * k + 1) % 7 != 0 for r in range(N)]


def column_pair(rng, na, nb, t, edge_pairs, draw_a, draw_b, k, poison=None):
    """two columns whose first rows are the edge pairs and the rest random draws,
    and their NULL-able twins.  `poison` is the value stored under a NULL slot: a
    kernel that evaluates the row anyway (unconditional loads) would raise."""
    a = [p[0] for p in edge_pairs] + [int(draw_a(rng)) for _ in range(N - len(edge_pairs))]
    b = [p[1] for p in edge_pairs] + [int(draw_b(rng)) for _ in range(N - len(edge_pairs))]
    out = [Col(na, t, a), Col(nb, t, b)]
    for j, (nm, v) in enumerate(((na, a), (nb, b))):
        m = null_mask(k + j)
        pv = poison[j] if poison else None
        out.append(Col(nm + "n", t, [x if ok or pv is None else pv for x, ok in zip(v, m)], m))
    return out


def core(t):
    lo, hi = R.INT_RANGE[t]
    return [lo, lo + 1, -1, 0, 1, hi - 1, hi] if lo < 0 else [0, 1, 2, hi - 1, hi]


def ints(lo, hi):
    return lambda g: g.integers(lo, hi, endpoint=True)


def _id():
    return Col("id", "BIGINT", range(N))


def make_tables():
    g = np.random.default_rng(20241019)
    T = {}
    # ---- 64-bit class: signed and unsigned integers
    c = [_id()]
    c += column_pair(g, "ba", "bb", "BIGINT", pairs(core("BIGINT"), [10 ** 18, -10 ** 18]),
                     ints(-2 ** 40, 2 ** 40), ints(-2 ** 20, 2 ** 20), 0, (I64[1], 0))
    c += column_pair(g, "ia", "ib", "INTEGER", pairs(core("INTEGER")), ints(-2 ** 15, 2 ** 15), ints(-2 ** 14, 2 ** 14), 2,
                     (2 ** 31 - 1, 0))
    c += column_pair(g, "sa", "sb", "SMALLINT", pairs(core("SMALLINT")), ints(-150, 150), ints(-150, 150), 4, (2 ** 15 - 1, 0))
    c += column_pair(g, "ta", "tb", "TINYINT", pairs(core("TINYINT")), ints(-10, 10), ints(-10, 10), 6, (127, 0))
    T["ti"] = Table("ti", c)
    c = [_id()]
    c += column_pair(g, "uta", "utb", "UTINYINT", pairs(core("UTINYINT")), ints(8, 15), ints(0, 7), 0, (255, 0))
    c += column_pair(g, "usa", "usb", "USMALLINT", pairs(core("USMALLINT")), ints(300, 400), ints(0, 100), 2, (65535, 0))
    c += column_pair(g, "uia", "uib", "UINTEGER", pairs(core("UINTEGER")), ints(70000, 130000), ints(0, 30000), 4,
                     (2 ** 32 - 1, 0))
    c += column_pair(g, "ula", "ulb", "UBIGINT", pairs(core("UBIGINT")), ints(2 ** 33, 2 ** 34), ints(0, 2 ** 29), 6,
                     (2 ** 64 - 1, 0))
    c += [Col("ta", "TINYINT", T["ti"].cols["ta"].values), Col("ia", "INTEGER", T["ti"].cols["ia"].values),
          Col("ba", "BIGINT", T["ti"].cols["ba"].values)]
    T["tu"] = Table("tu", c)
    # ---- 128-bit class
    hx = [10 ** 18, -10 ** 18, 10 ** 38 - 1, 2 ** 64 - 1, 2 ** 64, 2 ** 64 + 2 ** 63 + 2049]
    big = lambda bits_: (lambda g_: int(g_.integers(-2 ** 62, 2 ** 62)) * int(g_.integers(0, 2 ** (bits_ - 62))) // 1)
    c = [_id()]
    c += column_pair(g, "ha", "hb", "HUGEINT", pairs(core("HUGEINT"), hx), big(100), ints(-2 ** 26, 2 ** 26), 0,
                     (I128[1], 0))
    hq = [p[1] if I64[0] <= p[1] <= I64[1] else 3 for p in pairs(core("HUGEINT"), hx)]
    hq += [int(g.integers(-2 ** 20, 2 ** 20)) for _ in range(N - len(hq))]
    c += [Col("hq", "BIGINT", hq), Col("hqn", "BIGINT", hq, null_mask(3))]
    T["th"] = Table("th", c)
    # ---- decimals
    c = [_id()]
    half = [5, -5, 15, -15, 25, -25, 49, 50, 51, -49, -50, -51, 149, 150, -150]
    d9 = [10 ** 9 - 1, -(10 ** 9 - 1), 0, 1, -1] + half
    c += column_pair(g, "da", "db", "DECIMAL(9,2)", pairs(d9[:8]) + [(x, 100) for x in d9[8:]],
                     ints(-10 ** 6, 10 ** 6), ints(-10 ** 4, 10 ** 4), 0, (10 ** 9 - 1, 0))
    e18 = [10 ** 18 - 1, -(10 ** 18 - 1), 0, 1, -1, 81764416680803268, 5, -5, 15, 25]
    c += column_pair(g, "ea", "eb", "DECIMAL(18,1)", pairs(e18[:6]) + [(x, 10) for x in e18[6:]],
                     ints(-10 ** 12, 10 ** 12), ints(-10 ** 5, 10 ** 5), 2, (10 ** 18 - 1, 0))
    g38 = [10 ** 38 - 1, -(10 ** 38 - 1), 0, 1, -1, 10 ** 18, 5 * 10 ** 9, -5 * 10 ** 9, 15 * 10 ** 9 - 1]
    c += column_pair(g, "ga", "gb", "DECIMAL(38,10)", pairs(g38[:6]) + [(x, 1) for x in g38[6:]],
                     big(98), lambda g_: int(g_.integers(-2 ** 62, 2 ** 62)) * 16, 4, (10 ** 38 - 1, 0))
    k38 = [9 * 10 ** 37, -9 * 10 ** 37, 5 * 10 ** 37, -5 * 10 ** 37, 5 * 10 ** 37 - 1, 10 ** 38 - 1, -(10 ** 38 - 1), 0, 1,
           10 ** 37, 15 * 10 ** 36]
    k38 += [int(g.integers(-10 ** 18, 10 ** 18)) * int(g.integers(0, 10 ** 18)) * 99 for _ in range(N - len(k38))]
    w20 = [5 * 10 ** 17, -5 * 10 ** 17, 5 * 10 ** 17 - 1, 15 * 10 ** 17, 10 ** 38 - 1, -(10 ** 38 - 1), 0, 1, -1]
    w20 += [int(g.integers(-10 ** 18, 10 ** 18)) * int(g.integers(0, 10 ** 12)) for _ in range(N - len(w20))]
    v18 = [5 * 10 ** 17, -5 * 10 ** 17, 5 * 10 ** 17 - 1, 10 ** 18 - 1, -(10 ** 18 - 1), 0, 1, -1]
    v18 += [int(g.integers(-10 ** 18 + 1, 10 ** 18 - 1)) for _ in range(N - len(v18))]
    zz = [0, 1, -1, 0] + [0 if g.integers(0, 40) else int(g.integers(-1, 1, endpoint=True)) for _ in range(N - 4)]
    dq = [0, 1, -1, 10 ** 18, -10 ** 18, I64[1], I64[0]] + [int(g.integers(-10 ** 6, 10 ** 6)) for _ in range(N - 7)]
    c += [Col("ka", "DECIMAL(38,38)", k38), Col("kan", "DECIMAL(38,38)", k38, null_mask(6)),
          Col("wa", "DECIMAL(38,20)", w20), Col("va", "DECIMAL(18,18)", v18), Col("zz", "TINYINT", zz),
          Col("dq", "BIGINT", dq), Col("dqn", "BIGINT", dq, null_mask(7))]
    T["td"] = Table("td", c)
    # ---- doubles and floats
    sub = 5e-324
    fe = [0.0, -0.0, math.inf, -math.inf, math.nan, R.from_bits(0xFFF8000000000001), 0.5, 1.5, 2.5, -2.5,
          9007199254740993.0, 1e19, 1.7e38, sub, 1.0, -1.0]
    fp = list(itertools.product(fe, fe))

    def fdraw(scale):
        def f(g_):
            x = g_.standard_normal() * scale
            k = g_.integers(0, 4)
            return float(round(x)) + 0.5 if k == 0 else float(round(x)) if k == 1 else float(x)
        return f

    def fcol(name, t, edge, draw, k, conv=float):
        v = [conv(x) for x in edge] + [conv(draw(g)) for _ in range(N - len(edge))]
        return [Col(name, t, v), Col(name + "n", t, v, null_mask(k))]

    c = [_id()]
    c += fcol("fa", "DOUBLE", [p[0] for p in fp], fdraw(1e3), 0)
    c += fcol("fb", "DOUBLE", [p[1] for p in fp], fdraw(10), 1)
    c += fcol("fc", "DOUBLE", fe + [9.223372036854775e18, -9.223372036854775808e18, 2147483647.5, 2147483647.49,
                                    -2147483648.5, 1e-300, 1e300, 4.5e15 + 0.5], fdraw(1e6), 2)
    c += fcol("fs", "DOUBLE", [0.5, 1.5, 2.5, -2.5, -0.5, 126.5, 127.49, 127.5, -128.5, -128.51, 255.49, -0.49, 0.0, -0.0],
              fdraw(30), 3)
    fe32 = [R.f32(x) for x in fe[:13]] + [1e-45, 1.0, 16777217.0, 3.4028234663852886e38, 0.1]
    c += fcol("ra", "FLOAT", fe32 + fe32[::-1], fdraw(100), 4, R.f32)
    c += fcol("rb", "FLOAT", fe32 + fe32[3:] + fe32[:3], fdraw(7), 5, R.f32)
    T["tf"] = Table("tf", c)
    # ---- logic: NULL-able booleans in all nine pairs, small NULL-able integers
    tfn = [True, False, None]
    pv = [tfn[r % 3] for r in range(N)]
    qv = [tfn[(r // 3) % 3] for r in range(N)]
    lv = [int(g.integers(-5, 5, endpoint=True)) for _ in range(N)]
    mv = [int(g.integers(0, 4)) for _ in range(N)]
    T["tl"] = Table("tl", [_id(), Col("pn", "BOOLEAN", [bool(x) for x in pv], [x is not None for x in pv]),
                           Col("qn", "BOOLEAN", [bool(x) for x in qv], [x is not None for x in qv]),
                           Col("ln", "BIGINT", lv, null_mask(0)), Col("mn", "BIGINT", mv, null_mask(1)),
                           Col("on", "BIGINT", lv[::-1], null_mask(2))])
    # ---- range(): the virtual column
    T["tr"] = Table("tr", [Col("i", "BIGINT", range(N))], source=f"range({N}) tbl(i)")
    return T


TABLES = make_tables()


class Case:
    """sql over the columns of `table`; rtype as column_types reports it; fn maps
    one row (dict) to the expected value; out: 'int', 'bool', 'f64', 'f32' or
    ('dec', scale); ops: the VmOpc names the expression is meant to reach"""

    def __init__(self, fam, table, sql, rtype, out, fn, ops):
        self.fam, self.table, self.sql, self.rtype, self.out, self.fn = fam, TABLES[table], sql, rtype, out, fn
        self.ops = ["V_" + o for o in ops.split()]
        self.cols = [k for k in self.table.cols if re.search(rf"\b{k}\b", sql)]
        self.is_bool = rtype == "Boolean"

    def expect(self, r):
        """('ok', value) or ('err', kind) for row r"""
        try:
            return "ok", self.fn(self.table.row(r))
        except R.VmError as e:
            return "err", e.kind

    def text(self, v):
        if self.out == "bool":
            return "true" if v else "false"
        if self.out == "int":
            return str(v)
        return dec_text(v, self.out[1])

    def with_literals(self, r):
        s = self.sql
        for k in self.cols:
            s = re.sub(rf"\b{k}\b", self.table.cols[k].literal(r), s)
        return s


CASES = []


def C(fam, table, sql, rtype, out, fn, ops):
    CASES.append(Case(fam, table, sql, rtype, out, fn, ops))


SQLT = {"TINYINT": "TinyInt", "SMALLINT": "SmallInt", "INTEGER": "Integer", "BIGINT": "BigInt", "HUGEINT": "HugeInt",
        "UTINYINT": "UTinyInt", "USMALLINT": "USmallInt", "UINTEGER": "UInteger", "UBIGINT": "UBigInt"}


def int_family(fam, table, a, b, t, sfx, chk, unsigned=False):
    """+ - * // % (and -x, ABS for signed types) on one integer type"""
    L = "L" if t in ("HUGEINT", "UBIGINT") else "I"
    chk = (" " + chk) if chk else ""
    rt = SQLT[t]
    C(fam, table, f"{a} + {b}", rt, "int", lambda r: R.add(t, r[a], r[b]), f"LOADCOL ADD_{L}{chk}")
    C(fam, table, f"{a} - {b}", rt, "int", lambda r: R.sub(t, r[a], r[b]), f"SUB_{L}{chk}")
    C(fam, table, f"{a} * {b}", rt, "int", lambda r: R.mul(t, r[a], r[b]), f"MUL_{L}{chk}")
    C(fam, table, f"{a} // {b}", rt, "int", lambda r: R.idiv(t, r[a], r[b]), f"DIV_{L}{chk}")
    C(fam, table, f"{a} % {b}", rt, "int", lambda r: R.imod(t, r[a], r[b]), f"MOD_{L}{chk}")
    if not unsigned:
        C(fam, table, f"-{a}", rt, "int", lambda r: R.neg(t, r[a]), f"NEG_{L}{chk}")
        C(fam, table, f"ABS({a})", rt, "int", lambda r: R.abs_(t, r[a]), f"ABS_{L}{chk}")
    # the NULL-able twins: a NULL operand gives NULL, whatever lies under it
    an, bn = a + "n", b + "n"
    C(fam, table, f"{an} + {bn}", rt, "int", lambda r: R.add(t, r[an], r[bn]), f"ADD_{L}")
    C(fam, table, f"{an} // {bn}", rt, "int", lambda r: R.idiv(t, r[an], r[bn]), f"DIV_{L}")


def fdivi(x, y):
    return R.fop("/", R.int_to_f64(x), R.int_to_f64(y))


# ---- int64 ------------------------------------------------------------------------
int_family("int64", "ti", "ba", "bb", "BIGINT", "", "")
C("int64", "ti", "ba / bb", "Double", "f64", lambda r: fdivi(r["ba"], r["bb"]), "I2F DIV_F")
C("int64", "ti", "ban * 3 + 1", "BigInt", "int", lambda r: R.add("BIGINT", R.mul("BIGINT", r["ban"], 3), 1), "CONST MUL_I ADD_I")
int_family("int32", "ti", "ia", "ib", "INTEGER", "", "CHECK_I")
C("int32", "ti", "ia / ib", "Double", "f64", lambda r: fdivi(r["ia"], r["ib"]), "I2F DIV_F")
int_family("int16", "ti", "sa", "sb", "SMALLINT", "", "CHECK_I")
int_family("int8", "ti", "ta", "tb", "TINYINT", "", "CHECK_I")

# ---- unsigned -----------------------------------------------------------------------
int_family("uint8", "tu", "uta", "utb", "UTINYINT", "", "CHECK_I", True)
int_family("uint16", "tu", "usa", "usb", "USMALLINT", "", "CHECK_I", True)
int_family("uint32", "tu", "uia", "uib", "UINTEGER", "", "CHECK_I", True)
int_family("uint64", "tu", "ula", "ulb", "UBIGINT", "", "CHECK_L", True)
C("umixed", "tu", "ta + uta", "SmallInt", "int", lambda r: R.add("SMALLINT", r["ta"], r["uta"]), "ADD_I CHECK_I")
C("umixed", "tu", "ia * usa", "Integer", "int", lambda r: R.mul("INTEGER", r["ia"], r["usa"]), "MUL_I CHECK_I")
C("umixed", "tu", "ia - uia", "BigInt", "int", lambda r: R.sub("BIGINT", r["ia"], r["uia"]), "SUB_I")
C("umixed", "tu", "ba + ula", "HugeInt", "int", lambda r: R.add("HUGEINT", r["ba"], r["ula"]), "I2L ADD_L")
C("umixed", "tu", "ula / ulb", "Double", "f64", lambda r: fdivi(r["ula"], r["ulb"]), "L2F DIV_F")
C("umixed", "tu", "CAST(ula AS HUGEINT)", "HugeInt", "int", lambda r: r["ula"], "LOADCOL")
C("umixed", "tu", "CAST(ABS(ba) AS UBIGINT)", "UBigInt", "int",
  lambda r: R.cast_int(R.abs_("BIGINT", r["ba"]), "UBIGINT"), "ABS_I I2L CHECK_L")
C("umixed", "tu", "CAST(ulan AS BIGINT)", "BigInt", "int", lambda r: R.cast_int(r["ulan"], "BIGINT"), "L2I")
C("umixed", "tu", "CAST(uia AS INTEGER)", "Integer", "int", lambda r: R.cast_int(r["uia"], "INTEGER"), "CHECK_I")
C("umixed", "tu", "CAST(ABS(ta) AS UTINYINT)", "UTinyInt", "int",
  lambda r: R.cast_int(R.abs_("TINYINT", r["ta"]), "UTINYINT"), "ABS_I CHECK_I")
C("umixed", "tu", "ula > ulb", "Boolean", "bool", lambda r: R.compare(">", r["ula"], r["ulb"]), "CMP_L")
C("umixed", "tu", "uta = utb", "Boolean", "bool", lambda r: R.compare("=", r["uta"], r["utb"]), "CMP_I")

# ---- int128 -------------------------------------------------------------------------
int_family("int128", "th", "ha", "hb", "HUGEINT", "", "")
C("int128x", "th", "hq * ha", "HugeInt", "int", lambda r: R.mul("HUGEINT", r["hq"], r["ha"]), "I2L MUL_L")
C("int128x", "th", "hqn + han", "HugeInt", "int", lambda r: R.add("HUGEINT", r["hqn"], r["han"]), "I2L ADD_L")
C("int128x", "th", "CAST(hb AS BIGINT)", "BigInt", "int", lambda r: R.cast_int(r["hb"], "BIGINT"), "L2I")
C("int128x", "th", "CAST(hb AS INTEGER)", "Integer", "int", lambda r: R.cast_int(r["hb"], "INTEGER"), "L2I")
C("int128x", "th", "CAST(hq AS HUGEINT)", "HugeInt", "int", lambda r: r["hq"], "I2L")
C("int128x", "th", "CAST(ha AS DOUBLE)", "Double", "f64", lambda r: R.int_to_f64(r["ha"]), "L2F")
C("int128x", "th", "CAST(han AS FLOAT)", "Float", "f32", lambda r: R.to_f32(R.int_to_f64(r["han"])), "L2F MUL_F")
C("int128x", "th", "ha / hb", "Double", "f64", lambda r: fdivi(r["ha"], r["hb"]), "L2F DIV_F")
C("int128x", "th", "CAST(ha AS BOOLEAN)", "Boolean", "bool", lambda r: R.to_bool(r["ha"]), "TOBOOL_I")

# ---- decimal ------------------------------------------------------------------------
D = "Decimal"


def dec2(w, op, a, b):
    return lambda r: R.dec_arith(w, op, r[a], r[b])


def up(v, k):
    return None if v is None else v * 10 ** k


_add, _sub, _mul = (lambda x, y: x + y), (lambda x, y: x - y), (lambda x, y: x * y)
C("dec64", "td", "da + db", D, ("dec", 2), dec2(10, _add, "da", "db"), "ADD_I")
C("dec64", "td", "da - db", D, ("dec", 2), dec2(10, _sub, "da", "db"), "SUB_I")
C("dec64", "td", "da * db", D, ("dec", 4), dec2(18, _mul, "da", "db"), "MUL_I")
C("dec64", "td", "da % db", D, ("dec", 2), lambda r: R.imod("BIGINT", r["da"], r["db"]), "MOD_I")
C("dec64", "td", "dan + dbn", D, ("dec", 2), dec2(10, _add, "dan", "dbn"), "ADD_I")
C("dec64", "td", "da // db", "BigInt", "int",
  lambda r: R.f_to_int(R.fop("//", R.dec_to_f64(r["da"], 2), R.dec_to_f64(r["db"], 2)), "BIGINT"), "DEC2F_I IDIV_F F2I")
C("dec64", "td", "da + dq", D, ("dec", 2),
  lambda r: R.dec_arith(22, _add, R.cast_dec(r["da"], 2, 22, 2), R.cast_dec(r["dq"], 0, 22, 2)), "SCALEUP_L ADD_L CHECK_L")
C("dec128", "td", "ea + eb", D, ("dec", 1), dec2(19, _add, "ea", "eb"), "I2L ADD_L")
C("dec128", "td", "ea * eb", D, ("dec", 2), dec2(36, _mul, "ea", "eb"), "MUL_L")
C("dec128", "td", "ga + gb", D, ("dec", 10), dec2(38, _add, "ga", "gb"), "ADD_L")
C("dec128", "td", "ga - gb", D, ("dec", 10), dec2(38, _sub, "ga", "gb"), "SUB_L")
C("dec128", "td", "ga % gb", D, ("dec", 10), lambda r: R.imod("HUGEINT", r["ga"], r["gb"]), "MOD_L")
C("dec128", "td", "gan * dbn", D, ("dec", 12), dec2(38, _mul, "gan", "dbn"), "MUL_L")
C("dec128", "td", "-ga", D, ("dec", 10), lambda r: R.neg("HUGEINT", r["ga"]), "NEG_L")
C("dec128", "td", "ga > gb", "Boolean", "bool", lambda r: R.compare(">", r["ga"], r["gb"]), "CMP_L")
C("dec128", "td", "ea > da", "Boolean", "bool", lambda r: R.compare(">", up(r["ea"], 1), r["da"]), "SCALEUP_L CMP_L")
# rescale by 1, 18, 38, up and down
C("decscale", "td", "CAST(da AS DECIMAL(12,3))", D, ("dec", 3), lambda r: R.cast_dec(r["da"], 2, 12, 3), "SCALEUP_I CHECK_I")
C("decscale", "td", "CAST(zz AS DECIMAL(18,18))", D, ("dec", 18), lambda r: R.cast_dec(r["zz"], 0, 18, 18), "SCALEUP_I")
C("decscale", "td", "CAST(dqn AS DECIMAL(38,18))", D, ("dec", 18), lambda r: R.cast_dec(r["dqn"], 0, 38, 18), "SCALEUP_L")
C("decscale", "td", "CAST(zz AS DECIMAL(38,38))", D, ("dec", 38), lambda r: R.cast_dec(r["zz"], 0, 38, 38), "SCALEUP_L")
C("decscale", "td", "CAST(da AS DECIMAL(9,1))", D, ("dec", 1), lambda r: R.cast_dec(r["da"], 2, 9, 1), "SCALEDN_I")
C("decscale", "td", "CAST(va AS DECIMAL(18,0))", D, ("dec", 0), lambda r: R.cast_dec(r["va"], 18, 18, 0), "SCALEDN_I")
C("decscale", "td", "CAST(wa AS DECIMAL(38,2))", D, ("dec", 2), lambda r: R.cast_dec(r["wa"], 20, 38, 2), "SCALEDN_L")
C("decscale", "td", "CAST(ka AS DECIMAL(38,0))", D, ("dec", 0), lambda r: R.cast_dec(r["ka"], 38, 38, 0), "SCALEDN_L")
# 128-bit source, 64-bit target: the value fits only once it is scaled down
C("decscale", "td", "CAST(wa AS DECIMAL(18,2))", D, ("dec", 2), lambda r: R.cast_dec(r["wa"], 20, 18, 2), "SCALEDN_L L2I")
C("decscale", "td", "CAST(db AS DECIMAL(6,2))", D, ("dec", 2), lambda r: R.cast_dec(r["db"], 2, 6, 2), "CHECK_I")
# decimal <-> integer, double, float
C("deccast", "td", "CAST(ka AS BIGINT)", "BigInt", "int", lambda r: R.dec_to_int(r["ka"], 38, "BIGINT"), "SCALEDN_L L2I")
C("deccast", "td", "CAST(kan AS TINYINT)", "TinyInt", "int", lambda r: R.dec_to_int(r["kan"], 38, "TINYINT"), "SCALEDN_L L2I")
C("deccast", "td", "CAST(da AS INTEGER)", "Integer", "int", lambda r: R.dec_to_int(r["da"], 2, "INTEGER"), "SCALEDN_I CHECK_I")
C("deccast", "td", "CAST(ga AS HUGEINT)", "HugeInt", "int", lambda r: R.dec_to_int(r["ga"], 10, "HUGEINT"), "SCALEDN_L CHECK_L")
C("deccast", "td", "CAST(ea AS DOUBLE)", "Double", "f64", lambda r: R.dec_to_f64(r["ea"], 1), "DEC2F_I")
C("deccast", "td", "CAST(ea AS FLOAT)", "Float", "f32", lambda r: R.to_f32(R.dec_to_f64(r["ea"], 1)), "DEC2F_I MUL_F")
C("deccast", "td", "CAST(ka AS DOUBLE)", "Double", "f64", lambda r: R.dec_to_f64(r["ka"], 38), "DEC2F_L")
C("deccast", "td", "CAST(gan AS DOUBLE)", "Double", "f64", lambda r: R.dec_to_f64(r["gan"], 10), "DEC2F_L")
C("deccast", "td", "CAST(da AS BOOLEAN)", "Boolean", "bool", lambda r: R.to_bool(r["da"]), "TOBOOL_I")

# ---- double and float -----------------------------------------------------------------
for _op, _o in (("+", "ADD_F"), ("-", "SUB_F"), ("*", "MUL_F"), ("/", "DIV_F"), ("%", "MOD_F"), ("//", "IDIV_F")):
    C("double", "tf", f"fa {_op} fb", "Double", "f64", (lambda o: lambda r: R.fop(o, r["fa"], r["fb"]))(_op), _o)
    C("float", "tf", f"ra {_op} rb", "Double" if _op == "/" else "Float", "f64" if _op == "/" else "f32",
      (lambda o: lambda r: R.fop(o, r["ra"], r["rb"], o != "/"))(_op), _o)
C("double", "tf", "-fa", "Double", "f64", lambda r: R.fneg(r["fa"]), "NEG_F")
C("double", "tf", "ABS(fan)", "Double", "f64", lambda r: R.fabs_(r["fan"]), "ABS_F")
C("double", "tf", "fan + fbn", "Double", "f64", lambda r: R.fop("+", r["fan"], r["fbn"]), "ADD_F")
C("float", "tf", "-ra", "Float", "f32", lambda r: R.fneg(r["ra"]), "NEG_F")
C("float", "tf", "ABS(ra)", "Float", "f32", lambda r: R.fabs_(r["ra"]), "ABS_F")
C("float", "tf", "ra + fb", "Double", "f64", lambda r: R.fop("+", r["ra"], r["fb"]), "ADD_F")
C("float", "tf", "CAST(fa AS FLOAT)", "Float", "f32", lambda r: R.to_f32(r["fa"]), "MUL_F")
# the fused-multiply-add probe: a product rounded before the sum
C("fma", "tf", "fa * fb + fc", "Double", "f64", lambda r: R.fop("+", R.fop("*", r["fa"], r["fb"]), r["fc"]), "MUL_F ADD_F")
C("fma", "tf", "fa * fb - fc", "Double", "f64", lambda r: R.fop("-", R.fop("*", r["fa"], r["fb"]), r["fc"]), "MUL_F SUB_F")
C("fma", "tf", "fc * fc - fs * fs", "Double", "f64",
  lambda r: R.fop("-", R.fop("*", r["fc"], r["fc"]), R.fop("*", r["fs"], r["fs"])), "MUL_F SUB_F")
C("fma", "tf", "ra * rb + ra", "Float", "f32",
  lambda r: R.fop("+", R.fop("*", r["ra"], r["rb"], True), r["ra"], True), "MUL_F ADD_F")
for _t, _col in (("TINYINT", "fs"), ("UTINYINT", "fs"), ("SMALLINT", "fs"), ("USMALLINT", "fsn"), ("INTEGER", "fs"),
                 ("UINTEGER", "fs"), ("BIGINT", "fc"), ("UBIGINT", "fc"), ("HUGEINT", "fc")):
    if _t[0] == "U":  # the random rows of an unsigned target must not be negative
        C("fcast", "tf", f"CAST(ABS({_col}) AS {_t})", SQLT[_t], "int",
          (lambda t, c: lambda r: R.f_to_int(R.fabs_(r[c]), t))(_t, _col), "ABS_F " + ("F2L" if _t == "UBIGINT" else "F2I"))
    else:
        C("fcast", "tf", f"CAST({_col} AS {_t})", SQLT[_t], "int", (lambda t, c: lambda r: R.f_to_int(r[c], t))(_t, _col),
          "F2L" if _t == "HUGEINT" else "F2I")
C("fcast", "tf", "CAST(fs AS DECIMAL(9,2))", D, ("dec", 2), lambda r: R.f_to_dec(r["fs"], 9, 2), "F2DEC_I")
C("fcast", "tf", "CAST(fcn AS DECIMAL(38,10))", D, ("dec", 10), lambda r: R.f_to_dec(r["fcn"], 38, 10), "F2DEC_L")
C("fcast", "tf", "CAST(fc AS BOOLEAN)", "Boolean", "bool", lambda r: R.to_bool(r["fc"]), "TOBOOL_F")
C("fcast", "tf", "CAST(ra AS INTEGER)", "Integer", "int", lambda r: R.f_to_int(r["ra"], "INTEGER"), "F2I")

# ---- compare and logic ------------------------------------------------------------------
for _k, (_tb, _a, _b, _cl) in {"cmp_i": ("ti", "ba", "bb", "I"), "cmp_l": ("th", "ha", "hb", "L"),
                               "cmp_f": ("tf", "fa", "fb", "F")}.items():
    for _op in ("=", "<>", "<", "<=", ">", ">="):
        C(_k, _tb, f"{_a} {_op} {_b}", "Boolean", "bool",
          (lambda o, a, b: lambda r: R.compare(o, r[a], r[b]))(_op, _a, _b), f"CMP_{_cl}")
    _an, _bn = _a + "n", _b + "n"
    C(_k, _tb, f"{_an} < {_bn}", "Boolean", "bool", (lambda a, b: lambda r: R.compare("<", r[a], r[b]))(_an, _bn), f"CMP_{_cl}")
    C(_k, _tb, f"{_an} IS DISTINCT FROM {_bn}", "Boolean", "bool",
      (lambda a, b: lambda r: R.distinct(r[a], r[b]))(_an, _bn), f"DISTINCT_{_cl}")
    C(_k, _tb, f"{_an} IS NOT DISTINCT FROM {_bn}", "Boolean", "bool",
      (lambda a, b: lambda r: R.not_distinct(r[a], r[b]))(_an, _bn), f"DISTINCT_{_cl}")
    C(_k, _tb, f"{_a} IS DISTINCT FROM {_b}", "Boolean", "bool",
      (lambda a, b: lambda r: R.distinct(r[a], r[b]))(_a, _b), f"DISTINCT_{_cl}")
C("cmp_f", "tf", "ra >= rb", "Boolean", "bool", lambda r: R.compare(">=", r["ra"], r["rb"]), "CMP_F")
C("cmp_f", "tf", "fa = fa", "Boolean", "bool", lambda r: R.compare("=", r["fa"], r["fa"]), "CMP_F")

C("logic", "tl", "pn AND qn", "Boolean", "bool", lambda r: R.and3(r["pn"], r["qn"]), "AND")
C("logic", "tl", "pn OR qn", "Boolean", "bool", lambda r: R.or3(r["pn"], r["qn"]), "OR")
C("logic", "tl", "NOT pn", "Boolean", "bool", lambda r: R.not3(r["pn"]), "NOT")
C("logic", "tl", "pn IS NULL", "Boolean", "bool", lambda r: r["pn"] is None, "ISNULL")
C("logic", "tl", "ln IS NOT NULL", "Boolean", "bool", lambda r: r["ln"] is not None, "ISNOTNULL")
C("logic", "tl", "ln > 0 AND (mn = 1 OR on < 0)", "Boolean", "bool",
  lambda r: R.and3(R.compare(">", r["ln"], 0), R.or3(R.compare("=", r["mn"], 1), R.compare("<", r["on"], 0))),
  "CMP_I AND OR")
C("logic", "tl", "NOT (ln > mn)", "Boolean", "bool", lambda r: R.not3(R.compare(">", r["ln"], r["mn"])), "NOT CMP_I")
C("select", "tl", "COALESCE(ln, mn)", "BigInt", "int", lambda r: R.coalesce(r["ln"], r["mn"]), "COALESCE")
C("select", "tl", "COALESCE(ln, mn, 7)", "BigInt", "int", lambda r: R.coalesce(r["ln"], r["mn"], 7), "COALESCE CONST")
C("select", "tl", "CASE WHEN ln > 0 THEN mn END", "BigInt", "int",
  lambda r: R.case([(R.compare(">", r["ln"], 0), r["mn"])]), "SELECT")
C("select", "tl", "CASE WHEN ln > 0 THEN mn WHEN ln < 0 THEN -on ELSE 0 END", "BigInt", "int",
  lambda r: R.case([(R.compare(">", r["ln"], 0), r["mn"]), (R.compare("<", r["ln"], 0), R.neg("BIGINT", r["on"]))], 0),
  "SELECT NEG_I")
C("select", "tl", "CASE WHEN pn THEN ln ELSE on END", "BigInt", "int", lambda r: r["ln"] if r["pn"] else r["on"], "SELECT")
C("select", "tl", "mbx_synth(42, ln, mn)", "BigInt", "int", lambda r: R.synth(42, r["ln"], r["mn"]), "SYNTH")
C("select", "tl", "mbx_synth(42, id, 50) + 1", "BigInt", "int", lambda r: R.add("BIGINT", R.synth(42, r["id"], 50), 1), "SYNTH")
C("range", "tr", "i * 3 + 1", "BigInt", "int", lambda r: r["i"] * 3 + 1, "LOADRANGE MUL_I ADD_I")
C("range", "tr", "mbx_synth(7, i, 50)", "BigInt", "int", lambda r: R.synth(7, r["i"], 50), "LOADRANGE SYNTH")
C("range", "tr", "i % 7 = 3", "Boolean", "bool", lambda r: r["i"] % 7 == 3, "LOADRANGE MOD_I CMP_I")

FAMILIES = []
for _c in CASES:
    if _c.fam not in FAMILIES:
        FAMILIES.append(_c.fam)


def family(f):
    return [c for c in CASES if c.fam == f]


# ---- error cases ----------------------------------------------------------------------
# Table te: `one`, `hone` and `fone` are 0 everywhere and 1 at row 300, so every
# expression below is in range on 999 rows and raises at exactly one row inside
# a tile.  The twins are NULL at row 300 with the 1 still stored under the NULL.
ERR_ROW = 300
_one = [1 if r == ERR_ROW else 0 for r in range(N)]
_v300 = [r != ERR_ROW for r in range(N)]
TABLES["te"] = Table("te", [_id(), Col("one", "BIGINT", _one), Col("onen", "BIGINT", _one, _v300),
                            Col("hone", "HUGEINT", _one), Col("honen", "HUGEINT", _one, _v300),
                            Col("fone", "DOUBLE", [float(x) for x in _one]),
                            Col("fonen", "DOUBLE", [float(x) for x in _one], _v300)])
ERR_KEEP_OTHERS = f"id % {N} <> {ERR_ROW}"  # evaluated by the VM (not a bare range compare)
I64MAX, I64MIN, I128MAX, I128MIN = I64[1], I64[0], I128[1], I128[0]


class ErrCase:
    """sql over `one` / `hone` / `fone`; the NULL form replaces the column by its twin"""

    def __init__(self, name, sql, kind, ops, col):
        self.name, self.sql, self.kind, self.col = name, sql, kind, col
        self.ops = ["V_" + o for o in ops.split()]
        self.sql_null = re.sub(rf"\b{col}\b", col + "n", sql)

    def with_literals(self, one):
        c = TABLES["te"].cols[self.col]
        lit = f"CAST({'NULL' if one is None else one} AS {c.sqltype})"
        return re.sub(rf"\b{self.col}\b", lit, self.sql)


ERR_CASES = []


def E(name, sql, kind, ops, col="one"):
    ERR_CASES.append(ErrCase(name, sql, kind, ops, col))


E("add64", f"one + {I64MAX}", R.OOR, "ADD_I")
E("sub64", f"({I64MIN}) - one", R.OOR, "SUB_I")
E("mul64", "(one + 1) * 4611686018427387904", R.OOR, "MUL_I")
E("neg64", f"-(({I64MIN + 1}) - one)", R.OOR, "NEG_I")
E("idiv64", f"(({I64MIN + 1}) - one) // (-1)", R.OOR, "DIV_I")
E("abs64", f"ABS(({I64MIN + 1}) - one)", R.OOR, "ABS_I")
E("add128", f"hone + {I128MAX}", R.OOR, "ADD_L", "hone")
E("sub128", f"({I128MIN + 1}) - hone - hone", R.OOR, "SUB_L", "hone")
E("mul128", f"(hone + 1) * {2 ** 126}", R.OOR, "MUL_L", "hone")
E("neg128", f"-(({I128MIN + 1}) - hone)", R.OOR, "NEG_L", "hone")
E("idiv128", f"(({I128MIN + 1}) - hone) // (-1)", R.OOR, "DIV_L", "hone")
E("abs128", f"ABS(({I128MIN + 1}) - hone)", R.OOR, "ABS_L", "hone")
E("add32", "CAST(one AS INTEGER) + 2147483647", R.OOR, "ADD_I CHECK_I")
E("mul8", "CAST(one + 1 AS TINYINT) * CAST(64 AS TINYINT)", R.OOR, "MUL_I CHECK_I")
E("neg8", "-CAST(-127 - one AS TINYINT)", R.OOR, "NEG_I CHECK_I")
E("uadd64", "CAST(one AS UBIGINT) + CAST(18446744073709551615 AS UBIGINT)", R.OOR, "ADD_L CHECK_L")
E("usub64", "CAST(0 AS UBIGINT) - CAST(one AS UBIGINT)", R.OOR, "SUB_L CHECK_L")
E("umul64", "CAST(one + 1 AS UBIGINT) * CAST(9223372036854775808 AS UBIGINT)", R.OOR, "MUL_L CHECK_L")
E("usub8", "CAST(0 AS UTINYINT) - CAST(one AS UTINYINT)", R.OOR, "SUB_I CHECK_I")
# -x of an unsigned value fits only for 0, so it has no place among the non-raising cases
E("uneg8", "-CAST(one AS UTINYINT)", R.OOR, "NEG_I CHECK_I")
E("uneg64", "-CAST(one AS UBIGINT)", R.OOR, "NEG_L CHECK_L")
for _t in ("TINYINT", "SMALLINT", "INTEGER", "UTINYINT", "USMALLINT", "UINTEGER"):
    _lo, _hi = R.INT_RANGE[_t]
    E(f"cast_{_t.lower()}_hi", f"CAST(one + {_hi} AS {_t})", R.CONV, "CHECK_I")
    E(f"cast_{_t.lower()}_lo", f"CAST({_lo} - one AS {_t})", R.CONV, "CHECK_I")
for _t in ("BIGINT", "UBIGINT"):
    _lo, _hi = R.INT_RANGE[_t]
    E(f"cast_{_t.lower()}_hi", f"CAST(hone + {_hi} AS {_t})", R.CONV, "L2I" if _t == "BIGINT" else "CHECK_L", "hone")
    E(f"cast_{_t.lower()}_lo", f"CAST(({_lo}) - hone AS {_t})", R.CONV, "L2I" if _t == "BIGINT" else "CHECK_L", "hone")
E("dec_width", "CAST(one + 999 AS DECIMAL(3,0))", R.CONV, "CHECK_I")
E("dec_width128", f"CAST(hone + {10 ** 38 - 1} AS DECIMAL(38,0))", R.CONV, "CHECK_L", "hone")
E("dec_scaleup64", "CAST(CAST(one * 90 + 9 AS DECIMAL(9,0)) AS DECIMAL(18,17))", R.CONV, "SCALEUP_I")
E("dec_scaleup128", "CAST(CAST(one * 9 + 9 AS DECIMAL(38,0)) AS DECIMAL(38,37))", R.CONV, "SCALEUP_L")
E("f2i_nan", "CAST((fone * 1e308 * 10) - (fone * 1e308 * 10) AS BIGINT)", R.CONV, "F2I", "fone")
E("f2i_inf", "CAST(fone * 1e308 * 10 AS BIGINT)", R.CONV, "F2I", "fone")
E("f2i_2p63", "CAST(fone * 1024 + 9.223372036854774784e18 AS BIGINT)", R.CONV, "F2I", "fone")
E("f2l_inf", "CAST(fone * 1e308 * 10 AS HUGEINT)", R.CONV, "F2L", "fone")
E("f2dec", "CAST(fone * 1e10 AS DECIMAL(9,2))", R.CONV, "F2DEC_I", "fone")
