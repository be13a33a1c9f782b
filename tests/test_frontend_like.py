"""LIKE and VARCHAR comparisons in the front end, on a connection without a GPU:
the parser accepts [NOT] LIKE ... [ESCAPE ...], the binder folds constant
predicates through the matcher of csrc/str_match.h, raises DuckDB's two
pattern errors and keeps "Not implemented" for ILIKE / SIMILAR TO / GLOB and
non-constant patterns; EXPLAIN prints the predicate."""
import pytest

from conftest import q


def fold(conn, expr):
    res = q(conn, f"SELECT {expr}")
    assert res.column_types == ["Boolean"], (expr, res.column_types)
    return None if res.nulls[0][0] else res.rows[0][0] == "true"


@pytest.mark.parametrize("expr, want", [
    ("'abc' LIKE 'a%'", True), ("'abc' LIKE 'b%'", False), ("'abc' LIKE 'abc'", True), ("'abc' LIKE 'ab'", False),
    ("'abc' LIKE '%bc'", True), ("'abc' LIKE '%b%'", True), ("'abc' LIKE '%'", True), ("'' LIKE '%'", True),
    ("'' LIKE ''", True), ("'a' LIKE ''", False), ("'abc' LIKE 'a_c'", True), ("'abc' LIKE '_'", False),
    ("'é' LIKE '_'", True), ("'aXbYc' LIKE 'a%b%c'", True), ("'aXbY' LIKE 'a%b%c'", False),
    ("'abc' NOT LIKE 'a%'", False), ("'abc' NOT LIKE 'b%'", True),
    ("'50%' LIKE '%\\%%' ESCAPE '\\'", True), ("'50' LIKE '%\\%%' ESCAPE '\\'", False),
    ("'a_c' LIKE 'a#_c' ESCAPE '#'", True), ("'abc' LIKE 'a#_c' ESCAPE '#'", False),
    ("'a\\c' LIKE 'a\\c'", True),  # no ESCAPE clause: the backslash is an ordinary byte
    ("'abc' LIKE 'a%' ESCAPE ''", True),
    ("NULL LIKE 'a%'", None), ("'abc' LIKE NULL", None), ("'abc' NOT LIKE NULL", None),
    ("'abc' LIKE 'a%' ESCAPE NULL", None),
    ("starts_with('abc', 'ab')", True), ("prefix('abc', 'bc')", False), ("ends_with('abc', 'bc')", True),
    ("suffix('abc', 'ab')", False), ("contains('abc', 'b')", True), ("contains('abc', 'x')", False),
    ("contains('a%c', '%')", True), ("starts_with('abc', 'a%')", False), ("starts_with(NULL, 'a')", None),
    ("starts_with('abc', NULL)", None), ("starts_with('abc', '')", True),
    ("'b' BETWEEN 'a' AND 'c'", True), ("'d' BETWEEN 'a' AND 'c'", False), ("'b' NOT BETWEEN 'a' AND 'c'", False),
    ("'b' IN ('a', 'b')", True), ("'c' IN ('a', 'b')", False), ("'c' IN ('a', NULL)", None),
    ("'a' < 'ab'", True), ("'é' > 'z'", True), ("'a' = 'a'", True), ("'a' <> 'a'", False),
    ("'a' IS DISTINCT FROM NULL::VARCHAR", True), ("NULL::VARCHAR IS NOT DISTINCT FROM NULL::VARCHAR", True),
])
def test_constant_folds(hostconn, expr, want):
    assert fold(hostconn, expr) is want, expr


def test_pattern_errors(hostconn, mbx):
    r = hostconn.query("SELECT 'abc' LIKE 'a%' ESCAPE 'xy'")
    assert isinstance(r, mbx.Err)
    assert r.error.message == "Invalid Input Error: Invalid escape string. Escape string must be empty or one character."
    r = hostconn.query("SELECT 'abc' LIKE 'ab\\' ESCAPE '\\'")
    assert isinstance(r, mbx.Err)
    assert r.error.message == "Invalid Input Error: Like pattern must not end with escape character!"
    # the same two over a table column: raised at bind, before any launch
    q(hostconn, "CREATE TABLE t (s VARCHAR, p VARCHAR)")
    r = hostconn.query("SELECT s FROM t WHERE s LIKE 'x#' ESCAPE '#'")
    assert isinstance(r, mbx.Err) and "must not end with escape character" in r.error.message
    r = hostconn.query("SELECT s FROM t WHERE s LIKE 'x' ESCAPE '##'")
    assert isinstance(r, mbx.Err) and "Invalid escape string" in r.error.message


def test_what_stays_not_implemented(hostconn, mbx):
    q(hostconn, "CREATE TABLE t (s VARCHAR, p VARCHAR)")
    for sql, word in [("SELECT 'abc' ILIKE 'A%'", "ILIKE"), ("SELECT 'abc' NOT ILIKE 'A%'", "ILIKE"),
                      ("SELECT 'abc' SIMILAR TO 'a.*'", "SIMILAR TO"), ("SELECT 'abc' GLOB 'a*'", "GLOB"),
                      ("SELECT regexp_matches('abc', 'a.*')", "regexp_matches"),
                      ("SELECT s FROM t WHERE s LIKE p", "non-constant"),
                      ("SELECT s FROM t WHERE lower(s) LIKE 'a%'", "string expression"),
                      ("SELECT s FROM t WHERE contains(s || 'x', 'a')", "string expression"),
                      ("SELECT s FROM t WHERE s LIKE 'a' ESCAPE p", "non-constant"),
                      ("SELECT s FROM t WHERE starts_with(s, p)", "non-constant"),
                      ("SELECT s FROM t WHERE s LIKE '" + "x" * 256 + "'", "255 bytes")]:
        r = hostconn.query(sql)
        assert isinstance(r, mbx.Err), sql
        assert r.error.message.startswith("Not implemented Error") and word in r.error.message, (sql, r.error.message)


def test_explain_shows_the_predicate(hostconn):
    q(hostconn, "CREATE TABLE t (s VARCHAR, x INTEGER)")
    plan = hostconn.explain("SELECT COUNT(*) FROM t WHERE s LIKE 'a%' AND x > 3")
    assert "(#0 LIKE 'a%')" in plan and plan.rstrip().endswith("[device]"), plan
    plan = hostconn.explain("SELECT x FROM t WHERE s NOT LIKE 'a#%' ESCAPE '#'")
    assert "(NOT (#0 LIKE 'a#%' ESCAPE '#'))" in plan, plan
    plan = hostconn.explain("SELECT starts_with(s, 'ab'), ends_with(s, 'c'), contains(s, 'b') FROM t WHERE s >= 'm'")
    assert "prefix(#0, 'ab')" in plan and "suffix(#0, 'c')" in plan and "contains(#0, 'b')" in plan, plan
    assert "(#0 >= 'm')" in plan, plan
