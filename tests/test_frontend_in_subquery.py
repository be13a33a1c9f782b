"""x [NOT] IN (subquery) in the front end: parser, binder and EXPLAIN, on a
connection without a GPU.  The tables are empty (DDL only), so every statement
binds and nothing executes: what is checked is the bound plan -- the BOOLEAN
leaf where it stands in the expression, one `IN SUBQUERY <n> key <TYPE>: <left>`
line per subquery followed by the subquery's own plan, both sides cast to the
type `=` gives them (the join key's rule) -- the leaf in every clause, the
errors (column count, correlation, each key type that is not stored as an
integer of at most 8 bytes), that an expression list after IN binds as it
always did, and that a prepared statement with a parameter inside the subquery
keeps its plan."""
import pytest


@pytest.fixture()
def fe(hostconn, mbx):
    for ddl in ("CREATE TABLE a (k BIGINT, v INTEGER, s VARCHAR, dc DECIMAL(15,2))",
                "CREATE TABLE b (k TINYINT, w BIGINT, d DOUBLE)",
                "CREATE TABLE u (k UINTEGER, i INTEGER, h HUGEINT, big DECIMAL(38,2), iv INTERVAL, f FLOAT)"):
        assert isinstance(hostconn.query(ddl), mbx.Ok)
    return hostconn


def lines(plan):
    return [ln.rstrip() for ln in plan.splitlines()]


def test_explain_shows_leaf_subquery_line_key_type_and_plan(fe):
    plan = fe.explain("SELECT v FROM a WHERE k IN (SELECT k FROM b WHERE w > 3)")
    assert lines(plan) == [
        "SELECT #1 AS v :: INTEGER",
        "  FROM TABLE a",
        "  WHERE (#0 IN SUBQUERY 1)",
        "  IN SUBQUERY 1 key BIGINT: #0",
        "    SELECT CAST(#0 AS BIGINT) AS k :: BIGINT",
        "      FROM TABLE b",
        "      WHERE (#1 > 3)",
        "[device]",
    ]


@pytest.mark.parametrize("left, sub, key, left_txt, sub_out", [
    ("k", "SELECT k FROM b", "BIGINT", "#0", "CAST(#0 AS BIGINT) AS k :: BIGINT"),            # BIGINT against TINYINT
    ("v", "SELECT w FROM b", "BIGINT", "CAST(#1 AS BIGINT)", "#1 AS w :: BIGINT"),            # INTEGER against BIGINT
    ("v + 1", "SELECT k FROM b", "INTEGER", "(#1 + 1)", "CAST(#0 AS INTEGER) AS k :: INTEGER"),  # an expression
    ("dc", "SELECT i FROM u", "DECIMAL(15,2)", "#3", "CAST(#1 AS DECIMAL(15,2)) AS i :: DECIMAL(15,2)"),
])
def test_both_sides_are_cast_to_the_common_type(fe, left, sub, key, left_txt, sub_out):
    plan = lines(fe.explain(f"SELECT 1 FROM a WHERE {left} IN ({sub})"))
    assert f"  WHERE ({left_txt} IN SUBQUERY 1)" in plan
    at = plan.index(f"  IN SUBQUERY 1 key {key}: {left_txt}")
    assert plan[at + 1] == "    SELECT " + sub_out


def test_unsigned_with_signed_meets_in_bigint(fe):
    plan = lines(fe.explain("SELECT 1 FROM u WHERE k IN (SELECT v FROM a)"))  # UINTEGER with INTEGER
    at = plan.index("  IN SUBQUERY 1 key BIGINT: CAST(#0 AS BIGINT)")
    assert plan[at + 1] == "    SELECT CAST(#1 AS BIGINT) AS v :: BIGINT"


def test_not_in_is_a_not_over_the_same_leaf(fe):
    plan = lines(fe.explain("SELECT v FROM a WHERE k NOT IN (SELECT k FROM b)"))
    assert "  WHERE (NOT (#0 IN SUBQUERY 1))" in plan
    assert "  IN SUBQUERY 1 key BIGINT: #0" in plan
    pos = lines(fe.explain("SELECT v FROM a WHERE k IN (SELECT k FROM b)"))
    assert [ln for ln in plan if "WHERE" not in ln] == [ln for ln in pos if "WHERE" not in ln]


def test_leaf_in_select_list_and_case(fe):
    plan = lines(fe.explain("SELECT k IN (SELECT k FROM b) AS m, CASE WHEN v IN (SELECT w FROM b) THEN 1 ELSE 0 END AS c "
                            "FROM a"))
    assert plan[0] == ("SELECT (#0 IN SUBQUERY 1) AS m :: BOOLEAN, "
                       "CASE (CAST(#1 AS BIGINT) IN SUBQUERY 2) 1 0 END AS c :: INTEGER")
    assert "  IN SUBQUERY 1 key BIGINT: #0" in plan and "  IN SUBQUERY 2 key BIGINT: CAST(#1 AS BIGINT)" in plan
    assert plan.index("  IN SUBQUERY 1 key BIGINT: #0") < plan.index("  IN SUBQUERY 2 key BIGINT: CAST(#1 AS BIGINT)")


def test_leaf_in_having_reads_the_aggregate_relation(fe):
    plan = lines(fe.explain("SELECT v, COUNT(*) FROM a GROUP BY v HAVING MAX(k) IN (SELECT w FROM b)"))
    assert "  HAVING (#2 IN SUBQUERY 1)" in plan
    assert "  IN SUBQUERY 1 key BIGINT: #2" in plan


def test_leaf_as_group_key_and_in_an_aggregate_argument(fe):
    plan = lines(fe.explain("SELECT k IN (SELECT k FROM b) AS m, COUNT(*) FROM a GROUP BY k IN (SELECT k FROM b)"))
    assert plan[0] == "SELECT #0 AS m :: BOOLEAN, #1 AS count_star() :: BIGINT"  # the list's copy matched the key
    assert "  AGGREGATE groups=[(#0 IN SUBQUERY 1)] aggs=[count_star() :: BIGINT]" in plan
    assert sum(ln.startswith("  IN SUBQUERY") for ln in plan) == 1
    plan = lines(fe.explain("SELECT SUM(CASE WHEN k IN (SELECT k FROM b) THEN v END) FROM a"))
    assert "  AGGREGATE groups=[] aggs=[sum(CASE (#0 IN SUBQUERY 1) #1 END) :: HUGEINT]" in plan


def test_leaf_in_an_on_residual(fe):
    plan = lines(fe.explain("SELECT 1 FROM a JOIN b ON a.k = b.k AND a.v IN (SELECT i FROM u)"))
    assert "    RESIDUAL (#1 IN SUBQUERY 1)" in plan
    at = plan.index("  IN SUBQUERY 1 key INTEGER: #1")
    assert plan[at + 1:at + 3] == ["    SELECT #1 AS i :: INTEGER", "      FROM TABLE u"]


def test_subquery_may_hold_what_a_from_subquery_may(fe):
    plan = fe.explain("SELECT v FROM a WHERE k IN (SELECT w FROM b GROUP BY w UNION ALL "
                      "SELECT x.k FROM a x JOIN b y ON x.k = y.k ORDER BY 1 LIMIT 5)")
    assert "IN SUBQUERY 1 key BIGINT: #0" in plan
    assert "AGGREGATE groups=[#1]" in plan and "UNION ALL" in plan and "HASH JOIN key BIGINT" in plan
    assert "LIMIT 5 OFFSET 0" in plan
    # nested: the inner subquery is the inner select's, numbered after the outer one
    plan = lines(fe.explain("SELECT v FROM a WHERE k IN (SELECT w FROM b WHERE k IN (SELECT i FROM u))"))
    assert "  IN SUBQUERY 1 key BIGINT: #0" in plan
    assert "      WHERE (CAST(#0 AS INTEGER) IN SUBQUERY 2)" in plan
    assert "      IN SUBQUERY 2 key INTEGER: CAST(#0 AS INTEGER)" in plan


def test_one_row_select_is_not_host_constant(fe):
    plan = lines(fe.explain("SELECT 3 IN (SELECT k FROM b)"))
    assert plan[1] == "  FROM <one row>" and plan[-1] == "[device]"
    assert "  IN SUBQUERY 1 key INTEGER: 3" in plan


def test_expression_list_explains_as_before(fe):
    plan = fe.explain("SELECT v FROM a WHERE k IN (1, 2, 3)")
    assert lines(plan) == ["SELECT #1 AS v :: INTEGER", "  FROM TABLE a",
                           "  WHERE (((#0 = 1) OR (#0 = 2)) OR (#0 = 3))", "[device]"]
    plan = fe.explain("SELECT v FROM a WHERE k NOT IN (1, v)")
    assert "  WHERE (NOT ((#0 = 1) OR (#0 = CAST(#1 AS BIGINT))))" in lines(plan)
    assert "[host-constant]" in fe.explain("SELECT 2 IN (1, 2)")


def test_two_columns_is_a_binder_error(fe):
    with pytest.raises(Exception, match="Binder Error: Subquery returns 2 columns - expected 1"):
        fe.explain("SELECT v FROM a WHERE k IN (SELECT k, w FROM b)")
    with pytest.raises(Exception, match="Binder Error: Subquery returns 3 columns - expected 1"):
        fe.explain("SELECT v FROM a WHERE k IN (SELECT * FROM b)")


@pytest.mark.parametrize("sub", [
    "SELECT k FROM b WHERE b.w = a.v",
    "SELECT k FROM b WHERE w = v",
    "SELECT w + v FROM b",
])
def test_correlated_reference_is_refused(fe, sub):
    with pytest.raises(Exception, match="Not implemented Error: .*correlated subquery.*\"v\""):
        fe.explain(f"SELECT 1 FROM a WHERE k IN ({sub})")


def test_unknown_name_is_still_a_binder_error(fe):
    with pytest.raises(Exception, match="Binder Error: Referenced column \"nope\" not found"):
        fe.explain("SELECT 1 FROM a WHERE k IN (SELECT nope FROM b)")


@pytest.mark.parametrize("sql, typ", [
    ("SELECT 1 FROM a WHERE s IN (SELECT s FROM a)", "VARCHAR"),
    ("SELECT 1 FROM a WHERE k IN (SELECT d FROM b)", "DOUBLE"),
    ("SELECT 1 FROM b WHERE d IN (SELECT k FROM a)", "DOUBLE"),
    ("SELECT 1 FROM u WHERE f IN (SELECT f FROM u)", "FLOAT"),
    ("SELECT 1 FROM u WHERE h IN (SELECT h FROM u)", "HUGEINT"),
    ("SELECT 1 FROM u WHERE big IN (SELECT k FROM a)", r"DECIMAL\(38,2\)"),
    ("SELECT 1 FROM u WHERE iv IN (SELECT iv FROM u)", "INTERVAL"),
])
def test_refused_key_types_are_named(fe, sql, typ):
    with pytest.raises(Exception, match=r"Not implemented Error: IN \(subquery\) over a key of type " + typ + " "):
        fe.explain(sql)


def test_scalar_subquery_stays_refused(fe):
    with pytest.raises(Exception, match="Not implemented Error: scalar subqueries"):
        fe.explain("SELECT v FROM a WHERE k = (SELECT MAX(k) FROM b)")


def test_prepared_parameter_inside_the_subquery_keeps_one_bind(fe):
    st = fe.prepare("SELECT COUNT(*) FROM a WHERE k IN (SELECT k FROM b WHERE w > ?) AND v <> ?").value
    for i in range(4):
        st.bind_bigint(1, i)
        st.bind_bigint(2, i + 1)
        st.execute()  # no GPU: the statement binds (or patches its plan) and then has nowhere to run
    assert st.plan_stats() == {"binds": 1, "reuses": 3}
    st.close()
