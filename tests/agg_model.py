"""The reference model of the aggregates: what COUNT(*), COUNT(v), SUM, MIN, MAX
and AVG must return per group, in plain Python (exact `int`, `Fraction` and
`math.fsum`; no numpy arithmetic).  Used by test_agg_model.py (hand-worked
cases) and test_gpu_aggregate_values.py (every aggregate path on the device).

Two value classes:
  * "int": HUGEINT, UBIGINT and DECIMAL as unscaled integers.  SUM, MIN and MAX
    are exact integers, AVG is Fraction(sum, count * 10^scale).
  * "f64": DOUBLE, and FLOAT widened to double first.  SUM is NaN if a NaN is
    present or both infinities are, +-inf if one infinity is, else math.fsum;
    abs_sum = fsum(|x|) over the finite values is what a tolerance scales with.
    MIN / MAX order as vm_reference.cmp3 does (NaN greatest, every NaN equal,
    -0.0 equal to +0.0) and are returned as the SET of acceptable bit patterns:
    both zeros where the two signs tie, NAN (any NaN) where a NaN wins.
A group without a non-NULL value has NULL (None) for everything but the counts.
"""
import functools
import math
from fractions import Fraction

import vm_reference as R

NAN = "nan"  # in a MIN / MAX set: any NaN bit pattern is acceptable


class Stats:
    """one group's aggregates; sum / min / max / avg / abs_sum are None for a group
    without a non-NULL value (abs_sum also for the integer class)"""

    def __init__(self, count_star, count, sum_, min_, max_, avg, abs_sum=None):
        self.count_star, self.count, self.sum, self.min, self.max, self.avg = count_star, count, sum_, min_, max_, avg
        self.abs_sum = abs_sum

    def __repr__(self):
        return (f"Stats(count_star={self.count_star}, count={self.count}, sum={self.sum!r}, min={self.min!r}, "
                f"max={self.max!r}, avg={self.avg!r}, abs_sum={self.abs_sum!r})")


def _extreme_set(xs, sign):
    """the bit patterns of the values that tie for least (sign -1) or greatest (+1) under cmp3"""
    best = functools.reduce(lambda a, b: b if sign * R.cmp3(b, a) > 0 else a, xs)
    if best != best:
        return {NAN}
    return {R.bits(x) for x in xs if R.cmp3(x, best) == 0}


def fsum_special(xs):
    """SUM over doubles: NaN, +-inf, or the correctly rounded sum"""
    pinf, ninf = any(x == math.inf for x in xs), any(x == -math.inf for x in xs)
    if any(x != x for x in xs) or (pinf and ninf):
        return math.nan
    if pinf or ninf:
        return math.inf if pinf else -math.inf
    return math.fsum(xs)


def stats(values, kind, scale=0):
    """the aggregates over one group's values (None for NULL); kind: "int" or "f64" """
    xs = [v for v in values if v is not None]
    n = len(xs)
    if not n:
        return Stats(len(values), 0, None, None, None, None)
    if kind == "int":
        s = sum(xs)
        return Stats(len(values), n, s, min(xs), max(xs), Fraction(s, n * 10 ** scale))
    assert kind == "f64", kind
    s = fsum_special(xs)
    abs_sum = math.fsum(abs(x) for x in xs if x == x and not math.isinf(x))
    return Stats(len(values), n, s, _extreme_set(xs, -1), _extreme_set(xs, 1), s / n, abs_sum)


def key_of(k):
    """the group a key value falls in: NULL is a group, every NaN is one group, -0.0 is 0.0"""
    if isinstance(k, float):
        return NAN if k != k else (0.0 if k == 0 else k)
    if isinstance(k, tuple):
        return tuple(key_of(x) for x in k)
    return k


def aggregate(pairs, kind, scale=0):
    """{group: Stats} over (key, value) pairs; None is NULL on either side (a NULL key is a group)"""
    groups = {}
    for k, v in pairs:
        groups.setdefault(key_of(k), []).append(v)
    return {k: stats(vs, kind, scale) for k, vs in groups.items()}


def count_distinct(values):
    """COUNT(DISTINCT v): NULLs do not count, every NaN is one value, -0.0 is 0.0"""
    return len({key_of(v) for v in values if v is not None})
