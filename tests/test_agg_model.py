"""Hand-worked cases for agg_model, the reference of test_gpu_aggregate_values.py."""
import math
from fractions import Fraction

import agg_model as M
import vm_reference as R

INF, NAN = math.inf, math.nan
NEG_NAN = R.from_bits(0xFFF8000000000001)


def test_nan_beats_inf_for_max_and_not_for_min():
    s = M.stats([1.0, INF, NAN, -INF], "f64")
    assert s.max == {M.NAN}
    assert s.min == {R.bits(-INF)}
    assert s.sum != s.sum and s.avg != s.avg
    assert s.abs_sum == 1.0  # the finite values only


def test_min_of_all_nan_is_nan():
    s = M.stats([NAN, NEG_NAN, None], "f64")
    assert s.min == {M.NAN} and s.max == {M.NAN}
    assert (s.count_star, s.count) == (3, 2)


def test_negative_nan_is_greatest_too():
    s = M.stats([NEG_NAN, 5.0], "f64")
    assert s.max == {M.NAN} and s.min == {R.bits(5.0)}


def test_cancelling_sum_is_exact():
    s = M.stats([1e16, 1.0, -1e16], "f64")
    assert s.sum == 1.0 and s.abs_sum == 2e16 + 1.0
    assert s.avg == 1.0 / 3
    assert sum([1e16, 1.0, -1e16]) != 1.0  # a plain left-to-right sum loses the 1.0


def test_sum_with_infinities():
    assert M.stats([1.0, INF, 2.0], "f64").sum == INF
    assert M.stats([-INF, 1e300, -INF], "f64").sum == -INF
    s = M.stats([INF, -INF, 1.0], "f64")
    assert s.sum != s.sum
    assert s.min == {R.bits(-INF)} and s.max == {R.bits(INF)}


def test_signed_zeros_tie():
    s = M.stats([0.0, -0.0, 3.0], "f64")
    assert s.min == {R.bits(0.0), R.bits(-0.0)} and s.max == {R.bits(3.0)}
    s = M.stats([-0.0, -1.0], "f64")
    assert s.max == {R.bits(-0.0)}
    assert M.stats([5e-324, -5e-324], "f64").min == {R.bits(-5e-324)}


def test_ubigint_above_2_63_is_not_negative():
    top = 2 ** 64 - 1
    assert top > 2 ** 63
    s = M.stats([1, 2 ** 63, top, 2 ** 63 - 1], "int")
    assert (s.min, s.max) == (1, top)
    assert s.sum == 1 + 2 ** 63 + top + 2 ** 63 - 1
    assert s.avg == Fraction(s.sum, 4)


def test_hugeint_values_that_differ_only_in_the_high_word():
    lo = 12345
    xs = [(3 << 64) + lo, (-2 << 64) + lo, (1 << 64) + lo, lo]
    s = M.stats(xs, "int")
    assert s.min == (-2 << 64) + lo and s.max == (3 << 64) + lo
    # ... and only in the low word, with the top bit of the low word set
    ys = [(7 << 64) + 2 ** 63, (7 << 64) + 1, (7 << 64) + 2 ** 64 - 1]
    s = M.stats(ys, "int")
    assert s.min == (7 << 64) + 1 and s.max == (7 << 64) + 2 ** 64 - 1


def test_decimal_avg_divides_by_the_scale():
    s = M.stats([-1, 250, None], "int", scale=2)  # -0.01, 2.50
    assert s.sum == 249 and s.avg == Fraction(249, 200)
    assert (s.count_star, s.count) == (3, 2)


def test_all_null_group_and_grouping():
    g = M.aggregate([(1, None), (1, None), (2, 5), (None, 7), (2, None)], "int")
    assert set(g) == {1, 2, None}
    a = g[1]
    assert (a.count_star, a.count, a.sum, a.min, a.max, a.avg) == (2, 0, None, None, None, None)
    assert (g[2].count_star, g[2].count, g[2].sum) == (2, 1, 5)
    assert g[None].max == 7


def test_double_keys_fold_zeros_and_nans():
    g = M.aggregate([(0.0, 1), (-0.0, 2), (NAN, 3), (NEG_NAN, 4), (INF, 5), (-INF, 6), (5e-324, 7)], "int")
    assert set(g) == {0.0, M.NAN, INF, -INF, 5e-324}
    assert g[0.0].sum == 3 and g[M.NAN].sum == 7
    assert M.count_distinct([0.0, -0.0, NAN, NEG_NAN, None, 1.5, 1.5]) == 3
    assert M.count_distinct([(1 << 64) + 5, (2 << 64) + 5, 5, 5]) == 3
