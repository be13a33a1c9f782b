"""The sort model (sort_model.py) against expectations written out by hand, and
its numpy path against its comparator path over every column of the vm_cases
tables.  The GPU sort tests trust this model, so it is pinned here first."""
import math

import numpy as np
import pytest

import sort_model as M
import vm_cases as V
import vm_reference as R

I64 = R.INT_RANGE["BIGINT"]
NAN2 = R.from_bits(0xFFF8000000000001)  # a negative NaN with a payload


def both(n, keys):
    a = M.order(n, keys)
    assert M.order_np(n, keys) == a
    return a


def ids(n):
    return (list(range(n)), None, "int", False, None)


def test_signed_extremes():
    v = [0, I64[1], I64[0], -1, 1, I64[0] + 1, I64[1] - 1]
    assert both(7, [(v, None, "int", False, None), ids(7)]) == [2, 5, 3, 0, 4, 6, 1]
    assert both(7, [(v, None, "int", True, None), ids(7)]) == [1, 6, 4, 0, 3, 5, 2]


def test_unsigned_extremes_are_not_negative():
    v = [2 ** 63, 0, 2 ** 64 - 1, 2 ** 63 - 1, 1]
    assert both(5, [(v, None, "int", False, None), ids(5)]) == [1, 4, 3, 0, 2]
    assert both(5, [(np.array(v, dtype=np.uint64), None, "int", True, None), ids(5)]) == [2, 0, 3, 4, 1]


def test_zeros_tie_and_the_id_decides():
    v = [0.0, -0.0, 1.0, -0.0, 0.0, -1.0]
    assert both(6, [(v, None, "f64", False, None), ids(6)]) == [5, 0, 1, 3, 4, 2]
    assert both(6, [(v, None, "f64", True, None), ids(6)]) == [2, 0, 1, 3, 4, 5]
    # with the id descending the tie runs the other way: the sign of a zero never decides
    assert both(6, [(v, None, "f64", False, None), (list(range(6)), None, "int", True, None)]) == [5, 4, 3, 1, 0, 2]


def test_nans_are_one_greatest_value():
    v = [math.nan, math.inf, NAN2, -math.inf, 5e-324, math.nan, -5e-324]
    assert both(7, [(v, None, "f64", False, None), ids(7)]) == [3, 6, 4, 1, 0, 2, 5]
    assert both(7, [(v, None, "f64", True, None), ids(7)]) == [0, 2, 5, 1, 4, 6, 3]
    assert both(7, [(v, None, "f32", False, None), ids(7)]) == [3, 6, 4, 1, 0, 2, 5]


def test_nulls_last_by_default_in_both_directions():
    v = [3, 1, 99, 2, -99]
    ok = [True, True, False, True, False]  # what stands under a NULL is ignored
    assert both(5, [(v, ok, "int", False, None), ids(5)]) == [1, 3, 0, 2, 4]
    assert both(5, [(v, ok, "int", True, None), ids(5)]) == [0, 3, 1, 2, 4]
    assert both(5, [(v, ok, "int", False, False), ids(5)]) == [1, 3, 0, 2, 4]
    assert both(5, [(v, ok, "int", False, True), ids(5)]) == [2, 4, 1, 3, 0]
    assert both(5, [(v, ok, "int", True, True), ids(5)]) == [2, 4, 0, 3, 1]


def test_bool():
    v = [True, False, True, False]
    assert both(4, [(v, [True, True, False, True], "bool", False, None), ids(4)]) == [1, 3, 0, 2]
    assert both(4, [(v, None, "bool", True, None), ids(4)]) == [0, 2, 1, 3]


def test_empty_string_is_not_null():
    v = ["", "a", "", "", "b"]
    ok = [True, True, False, True, True]
    assert both(5, [(v, ok, "str", False, None), ids(5)]) == [0, 3, 1, 4, 2]
    assert both(5, [(v, ok, "str", False, True), ids(5)]) == [2, 0, 3, 1, 4]
    assert both(5, [(v, ok, "str", True, None), ids(5)]) == [4, 1, 0, 3, 2]


def test_bytes_compare_unsigned():
    v = ["aé", "a\x7f", "a", "b", "aéa"]  # 0x61 0xC3 0xA9 is above 0x61 0x7F
    assert both(5, [(v, None, "str", False, None), ids(5)]) == [2, 1, 0, 4, 3]
    assert both(5, [([s.encode() for s in v], None, "str", True, None), ids(5)]) == [3, 4, 0, 1, 2]


def test_strings_sharing_an_eight_byte_prefix():
    p = "abcdefgh"
    v = [p + "ijklmnopq", p, p + "ijklmnop", p + "i", p + "ijklmnopp", p + "h", "abcdefg"]  # 17, 8, 16, 9, 17, 9, 7 bytes
    assert [len(s) for s in v] == [17, 8, 16, 9, 17, 9, 7]
    assert both(7, [(v, None, "str", False, None), ids(7)]) == [6, 1, 5, 3, 2, 4, 0]
    assert both(7, [(v, None, "str", True, None), ids(7)]) == [0, 4, 2, 3, 5, 1, 6]


def test_keys_compare_left_to_right():
    a = [1, 0, 1, 0, 1, 0]
    s = ["x", "y", "x", "x", "w", "y"]
    d = [0.0, 2.0, -0.0, math.nan, 1.0, NAN2]
    keys = [(a, None, "int", True, None), (s, [True] * 4 + [False, True], "str", False, True),
            (d, None, "f64", True, None), ids(6)]
    # a = 1: the NULL string first, then "x" twice with equal zeros (id decides); a = 0: "x", then "y" twice
    # with NaN above 2.0, descending
    assert both(6, keys) == [4, 0, 2, 3, 5, 1]


def test_a_subset_of_the_rows():
    v = [5, 3, 4, 1, 2]
    keys = [(v, None, "int", False, None), ids(5)]
    assert M.order([0, 2, 4], keys) == M.order_np([0, 2, 4], keys) == [4, 2, 0]


@pytest.mark.parametrize("table", [t for t in V.TABLES if t != "tr"])
def test_numpy_path_agrees_on_the_case_tables(table):
    t = V.TABLES[table]
    id_ = M.key_of(t.cols["id"])
    for k, (name, c) in enumerate(t.cols.items()):
        if name == "id":
            continue
        for desc, nf in ((False, None), (True, True), (True, False)):
            keys = [M.key_of(c, desc, nf), id_]
            assert M.order_np(V.N, keys) == M.order(V.N, keys), (table, name, desc, nf)
    names = [n for n in t.cols if n != "id"]
    keys = [M.key_of(t.cols[names[-1]], True, True), M.key_of(t.cols[names[0]], False, None), id_]
    assert M.order_np(V.N, keys) == M.order(V.N, keys), table
