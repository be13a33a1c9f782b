"""The exact model of the expression VM (csrc/vm.h): what every instruction
must return, written from the SQL / DuckDB semantics that vm.h and binder.cpp
document, with Python's exact `int` for integers and decimals and single IEEE
operations for doubles.  It is not a transcription of vm_step.

Every function returns a value, None for NULL, or raises VmError(kind), where
kind is the error family the engine reports: "Out of Range" for an arithmetic
overflow (E_OVF_*), "Conversion" for a cast that does not fit (E_CAST_RANGE,
which is also what a decimal rescale raises: only casts rescale).

Values: integers and booleans are `int` / `bool`, a DECIMAL is its unscaled
`int` (the case knows the scale), DOUBLE and FLOAT are `float`.

The two double conversions ("Expression VM"):
  * 128-bit integer -> DOUBLE is correctly rounded (Python's float(int)).
  * DECIMAL -> DOUBLE is double(unscaled) / double(10^scale): two correctly
    rounded steps, not the correctly rounded quotient.
"""
import math
import struct

OOR = "Out of Range"
CONV = "Conversion"


class VmError(Exception):
    def __init__(self, kind):
        super().__init__(kind)
        self.kind = kind


INT_RANGE = {
    "TINYINT": (-2 ** 7, 2 ** 7 - 1), "SMALLINT": (-2 ** 15, 2 ** 15 - 1), "INTEGER": (-2 ** 31, 2 ** 31 - 1),
    "BIGINT": (-2 ** 63, 2 ** 63 - 1), "HUGEINT": (-2 ** 127, 2 ** 127 - 1),
    "UTINYINT": (0, 2 ** 8 - 1), "USMALLINT": (0, 2 ** 16 - 1), "UINTEGER": (0, 2 ** 32 - 1),
    "UBIGINT": (0, 2 ** 64 - 1),
}
F_GUARD = 1.7014118346046923e38  # 2^127: nothing at or beyond it converts to an integer


def nulls(*a):
    return any(x is None for x in a)


# ---- integers ---------------------------------------------------------------
def div(a, b):
    """truncating division (C, SQL //)"""
    q = abs(a) // abs(b)
    return -q if (a < 0) != (b < 0) else q


def mod(a, b):
    """remainder with the sign of the dividend"""
    return a - div(a, b) * b


def round_half_away_div(v, d):
    q, r = divmod(abs(v), d)
    if 2 * r >= d:
        q += 1
    return -q if v < 0 else q


def in_range(v, t, kind):
    lo, hi = INT_RANGE[t]
    if v < lo or v > hi:
        raise VmError(kind)
    return v


def _arith(t, f, *a):
    if nulls(*a):
        return None
    return in_range(f(*a), t, OOR)


def add(t, a, b): return _arith(t, lambda x, y: x + y, a, b)
def sub(t, a, b): return _arith(t, lambda x, y: x - y, a, b)
def mul(t, a, b): return _arith(t, lambda x, y: x * y, a, b)
def neg(t, a): return _arith(t, lambda x: -x, a)
def abs_(t, a): return _arith(t, abs, a)


def idiv(t, a, b):
    if nulls(a, b) or b == 0:
        return None
    return in_range(div(a, b), t, OOR)


def imod(t, a, b):
    if nulls(a, b) or b == 0:
        return None
    return mod(a, b)


def cast_int(v, to):
    return None if v is None else in_range(v, to, CONV)


# ---- decimals (unscaled ints) -------------------------------------------------
def dec_phys(width):
    return "BIGINT" if width <= 18 else "HUGEINT"


def dec_check(raw, width):
    if abs(raw) > 10 ** width - 1:
        raise VmError(CONV)
    return raw


def rescale(raw, from_scale, to_scale):
    if to_scale >= from_scale:
        return raw * 10 ** (to_scale - from_scale)
    return round_half_away_div(raw, 10 ** (from_scale - to_scale))


def cast_dec(raw, from_scale, width, scale):
    """integer (from_scale 0) or decimal -> DECIMAL(width, scale)"""
    return None if raw is None else dec_check(rescale(raw, from_scale, scale), width)


def dec_to_int(raw, scale, to):
    return None if raw is None else in_range(round_half_away_div(raw, 10 ** scale), to, CONV)


def dec_arith(width, f, *a):
    """decimal + - * : the operands are already at the result's scale (add,
    sub) or keep their own (mul); only the storage class can overflow"""
    if nulls(*a):
        return None
    return in_range(f(*a), dec_phys(width), OOR)


def dec_to_f64(raw, scale):
    return None if raw is None else float(raw) / float(10 ** scale)


# ---- doubles --------------------------------------------------------------------
def f64(x):
    return struct.unpack("<d", struct.pack("<d", x))[0]


def f32(x):
    if x != x or math.isinf(x):
        return x
    try:
        return struct.unpack("<f", struct.pack("<f", x))[0]
    except OverflowError:
        return math.copysign(math.inf, x)


def bits(x):
    return struct.unpack("<Q", struct.pack("<d", x))[0]


def from_bits(u):
    return struct.unpack("<d", struct.pack("<Q", u))[0]


def _fmod(x, y):
    if x != x or y != y or math.isinf(x):
        return math.nan
    if math.isinf(y):
        return x
    return math.fmod(x, y)


def _fdiv(x, y):
    return x / y


def _ftrunc(r):
    if r != r or math.isinf(r):
        return r
    return math.copysign(float(abs(math.trunc(r))), r)


def fop(op, a, b, flt=False):
    """one IEEE double operation; FLOAT results are rounded to float once more"""
    if nulls(a, b):
        return None
    if op in "/%" or op == "//":
        if b == 0:
            return None
    r = {"+": lambda: a + b, "-": lambda: a - b, "*": lambda: a * b, "/": lambda: _fdiv(a, b),
         "%": lambda: _fmod(a, b), "//": lambda: _ftrunc(_fdiv(a, b))}[op]()
    return f32(r) if flt else r


def fneg(a): return None if a is None else -a
def fabs_(a): return None if a is None else math.fabs(a)


def cmp3(x, y):
    """NaN is greatest and equal to itself; -0.0 == +0.0"""
    nx, ny = x != x, y != y
    if nx or ny:
        return 0 if nx == ny else (1 if nx else -1)
    return -1 if x < y else 1 if x > y else 0


def compare(op, a, b):
    if nulls(a, b):
        return None
    c = cmp3(a, b)
    return {"=": c == 0, "<>": c != 0, "<": c < 0, "<=": c <= 0, ">": c > 0, ">=": c >= 0}[op]


def f_to_int(x, to):
    """round half to even, then the 2^127 guard, then the type's range"""
    if x is None:
        return None
    if x != x or math.isinf(x):
        raise VmError(CONV)
    r = round(x)  # exact int, ties to even
    if not (-F_GUARD <= float(r) < F_GUARD):
        raise VmError(CONV)
    return in_range(r, to, CONV)


def f_to_dec(x, width, scale):
    if x is None:
        return None
    s = x * float(10 ** scale)
    if s != s or math.isinf(s):
        raise VmError(CONV)
    r = round(s)
    if not (-F_GUARD <= float(r) < F_GUARD):
        raise VmError(CONV)
    return dec_check(r, width)


def int_to_f64(v): return None if v is None else float(v)
def to_f32(x): return None if x is None else f32(x)
def to_bool(v): return None if v is None else v != 0


# ---- logic ------------------------------------------------------------------------
def and3(a, b):
    if a is False or b is False:
        return False
    return None if nulls(a, b) else True


def or3(a, b):
    if a is True or b is True:
        return True
    return None if nulls(a, b) else False


def not3(a): return None if a is None else not a


def distinct(a, b):
    if nulls(a, b):
        return (a is None) != (b is None)
    return cmp3(a, b) != 0


def not_distinct(a, b): return not distinct(a, b)


def coalesce(*a):
    for x in a:
        if x is not None:
            return x
    return None


def case(pairs, els=None):
    for c, v in pairs:
        if c:
            return v
    return els


def synth(seed, i, m):
    if nulls(seed, i, m) or m % 2 ** 64 == 0:
        return None
    M = 2 ** 64 - 1
    z = (seed + i + 0x9E3779B97F4A7C15) & M
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M
    return (z ^ (z >> 31)) % (m % 2 ** 64)
