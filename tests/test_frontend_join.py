"""Inner equi-joins in the front end: parser, binder and EXPLAIN, on a
connection without a GPU.  The tables are empty (DDL only), so every statement
binds and nothing executes: what is checked is the bound plan -- both inputs,
the join key cast to the common type of its two sides, the residual -- the
scope of a join (qualified names, *, alias.*, ambiguity, duplicate aliases),
the forms that stay refused, each with its own Not implemented message, and
that a prepared statement with parameters in ON and WHERE keeps its plan."""
import pytest


@pytest.fixture()
def fe(hostconn, mbx):
    for ddl in ("CREATE TABLE a (k BIGINT, v INTEGER, s VARCHAR)",
                "CREATE TABLE b (k TINYINT, w BIGINT, d DOUBLE)",
                "CREATE TABLE u (k UINTEGER, i INTEGER, h HUGEINT, big DECIMAL(38,2), iv INTERVAL)"):
        assert isinstance(hostconn.query(ddl), mbx.Ok)
    return hostconn


def test_explain_shows_inputs_key_and_residual(fe):
    plan = fe.explain("SELECT a.v, b.w FROM a JOIN b ON a.k = b.k AND a.v < b.w")
    assert "HASH JOIN key BIGINT: left #0 = right CAST(#0 AS BIGINT)" in plan
    assert "RESIDUAL (CAST(#1 AS BIGINT) < #4)" in plan
    assert "LEFT TABLE a" in plan and "RIGHT TABLE b" in plan
    assert plan.index("LEFT TABLE a") < plan.index("RIGHT TABLE b")
    # outputs read the joined columns: a's three, then b's
    assert "SELECT #1 AS v :: INTEGER, #4 AS w :: BIGINT" in plan
    # INNER is optional, the sides of the equality may come in either order
    again = fe.explain("SELECT a.v, b.w FROM a INNER JOIN b ON b.k = a.k AND a.v < b.w")
    assert again == plan


def test_two_key_equality_keeps_the_second_as_residual(fe):
    plan = fe.explain("SELECT 1 FROM a JOIN b ON a.k = b.k AND a.v = b.w")
    assert "HASH JOIN key BIGINT: left #0 = right CAST(#0 AS BIGINT)" in plan
    assert "RESIDUAL (CAST(#1 AS BIGINT) = #4)" in plan


def test_star_gives_left_then_right_with_both_copies(fe):
    plan = fe.explain("SELECT * FROM a JOIN b ON a.k = b.k")
    assert plan.splitlines()[0] == ("SELECT #0 AS k :: BIGINT, #1 AS v :: INTEGER, #2 AS s :: VARCHAR, "
                                    "#3 AS k :: TINYINT, #4 AS w :: BIGINT, #5 AS d :: DOUBLE")


def test_alias_star_gives_one_input(fe):
    plan = fe.explain("SELECT b.* FROM a JOIN b ON a.k = b.k")
    assert plan.splitlines()[0] == "SELECT #3 AS k :: TINYINT, #4 AS w :: BIGINT, #5 AS d :: DOUBLE"
    plan = fe.explain("SELECT y.*, x.v FROM a x JOIN b y ON x.k = y.k")
    assert plan.splitlines()[0] == "SELECT #3 AS k :: TINYINT, #4 AS w :: BIGINT, #5 AS d :: DOUBLE, #1 AS v :: INTEGER"
    with pytest.raises(Exception, match="Binder Error.*\"zz\""):
        fe.explain("SELECT zz.* FROM a JOIN b ON a.k = b.k")
    # one table: the qualifier is honoured too
    assert fe.explain("SELECT t.* FROM a t").splitlines()[0].startswith("SELECT #0 AS k :: BIGINT, #1 AS v")


def test_unqualified_shared_name_is_ambiguous(fe):
    with pytest.raises(Exception, match="Binder Error: Ambiguous reference to column name \"k\""):
        fe.explain("SELECT k FROM a JOIN b ON a.k = b.k")
    with pytest.raises(Exception, match="Ambiguous reference to column name \"k\""):
        fe.explain("SELECT a.v FROM a JOIN b ON k = b.k")
    # a name only one side owns needs no qualifier
    assert "SELECT #1 AS v :: INTEGER, #4 AS w :: BIGINT" in fe.explain("SELECT v, w FROM a JOIN b ON a.k = b.k")


def test_duplicate_alias_is_a_binder_error(fe):
    with pytest.raises(Exception, match="Binder Error: Duplicate alias \"a\""):
        fe.explain("SELECT 1 FROM a JOIN a ON a.k = a.k")
    with pytest.raises(Exception, match="Binder Error: Duplicate alias \"x\""):
        fe.explain("SELECT 1 FROM a x JOIN b x ON x.k = x.w")
    with pytest.raises(Exception, match="Binder Error: Duplicate alias \"a\""):
        fe.explain("SELECT 1 FROM a JOIN b ON a.k = b.k JOIN u a ON a.i = b.k")


def test_self_join_under_two_aliases(fe):
    plan = fe.explain("SELECT x.k, y.v FROM a x JOIN a y ON x.k = y.k")
    assert "HASH JOIN key BIGINT: left #0 = right #0" in plan
    assert plan.count("TABLE a") == 2
    assert plan.splitlines()[0] == "SELECT #0 AS k :: BIGINT, #4 AS v :: INTEGER"


def test_three_table_chain_is_left_deep(fe):
    plan = fe.explain("SELECT COUNT(*) FROM a JOIN b ON a.k = b.k JOIN u ON u.i = a.v WHERE u.k > 3")
    lines = [ln.strip() for ln in plan.splitlines()]
    outer, inner = lines.index("FROM HASH JOIN key INTEGER: left #1 = right #1"), \
        lines.index("LEFT HASH JOIN key BIGINT: left #0 = right CAST(#0 AS BIGINT)")
    assert outer < inner < lines.index("LEFT TABLE a") < lines.index("RIGHT TABLE b") < lines.index("RIGHT TABLE u")
    assert "WHERE (CAST(#6 AS BIGINT) > 3)" in plan  # u.k is the joined relation's column 6


def test_inputs_of_every_kind(fe):
    plan = fe.explain("SELECT r.range, t.s, q.kk FROM range(5) r JOIN (VALUES (1, 'x'), (2, 'y')) t(k, s) "
                      "ON r.range = t.k JOIN (SELECT k + 1 AS kk FROM a) q ON q.kk = r.range")
    assert "RANGE(0, 5, 1)" in plan and "VALUES[2 rows]" in plan and "RIGHT (" in plan and "TABLE a" in plan
    assert plan.splitlines()[0] == "SELECT #0 AS range :: BIGINT, #2 AS s :: VARCHAR, #3 AS kk :: BIGINT"
    plan = fe.explain("SELECT g.generate_series FROM generate_series(1, 3) g JOIN a ON a.k = g.generate_series")
    assert "RANGE(1, 3, 1, inclusive)" in plan


@pytest.mark.parametrize("on, key", [
    ("a.k = b.k", "BIGINT: left #0 = right CAST(#0 AS BIGINT)"),           # BIGINT with TINYINT
    ("b.k = a.k", "BIGINT: left #0 = right CAST(#0 AS BIGINT)"),
    ("a.v = b.k", "INTEGER: left #1 = right CAST(#0 AS INTEGER)"),
    ("a.k = b.k + 1", "BIGINT: left #0 = right CAST((CAST(#0 AS INTEGER) + 1) AS BIGINT)"),
    ("a.k - 1 = b.w * 2", "BIGINT: left (#0 - 1) = right (#1 * 2)"),
])
def test_key_common_type(fe, on, key):
    assert "HASH JOIN key " + key in fe.explain("SELECT 1 FROM a JOIN b ON " + on)


def test_key_common_type_unsigned_with_signed(fe):
    plan = fe.explain("SELECT 1 FROM u JOIN a ON u.k = a.v")  # UINTEGER with INTEGER
    assert "HASH JOIN key BIGINT: left CAST(#0 AS BIGINT) = right CAST(#1 AS BIGINT)" in plan


@pytest.mark.parametrize("sql, reason", [
    ("SELECT 1 FROM a LEFT JOIN b ON a.k = b.k", "LEFT JOIN"),
    ("SELECT 1 FROM a LEFT OUTER JOIN b ON a.k = b.k", "LEFT JOIN"),
    ("SELECT 1 FROM a RIGHT JOIN b ON a.k = b.k", "RIGHT JOIN"),
    ("SELECT 1 FROM a FULL OUTER JOIN b ON a.k = b.k", "FULL JOIN"),
    ("SELECT 1 FROM a CROSS JOIN b", "CROSS JOIN"),
    ("SELECT 1 FROM a, b", "comma join"),
    ("SELECT 1 FROM a x, b y WHERE x.k = y.k", "comma join"),
    ("SELECT 1 FROM a JOIN b USING (k)", "USING"),
    ("SELECT 1 FROM a NATURAL JOIN b", "NATURAL JOIN"),
    ("SELECT 1 FROM a SEMI JOIN b ON a.k = b.k", "SEMI JOIN"),
    ("SELECT 1 FROM a ANTI JOIN b ON a.k = b.k", "ANTI JOIN"),
    ("SELECT 1 FROM a JOIN b ON a.v < b.w", "no equality between"),
    ("SELECT 1 FROM a JOIN b ON a.k = 1", "no equality between"),
    ("SELECT 1 FROM a JOIN b ON a.k = a.v", "no equality between"),
    ("SELECT 1 FROM a JOIN b ON a.k = b.k OR a.v = b.w", "no equality between"),
    ("SELECT 1 FROM a x JOIN a y ON x.s = y.s", "join key of type VARCHAR"),
    ("SELECT 1 FROM a JOIN b ON a.k = b.d", "join key of type DOUBLE"),
    ("SELECT 1 FROM b JOIN b c ON b.d = c.d", "join key of type DOUBLE"),
    ("SELECT 1 FROM u JOIN u w ON u.h = w.h", "join key of type HUGEINT"),
    ("SELECT 1 FROM u JOIN u w ON u.big = w.big", r"join key of type DECIMAL\(38,2\)"),
    ("SELECT 1 FROM u JOIN u w ON u.iv = w.iv", "join key of type INTERVAL"),
])
def test_out_of_scope_forms_name_their_reason(fe, sql, reason):
    with pytest.raises(Exception, match="Not implemented Error: .*" + reason):
        fe.explain(sql)


def test_join_words_are_still_names_elsewhere(fe, mbx):
    # NATURAL / FULL / SEMI / ANTI are refused in front of JOIN only
    assert "TABLE a" in fe.explain("SELECT natural.k FROM a natural")
    assert "HASH JOIN" in fe.explain("SELECT semi.k FROM a AS semi JOIN b ON semi.k = b.k")
    assert isinstance(fe.query("CREATE TABLE anti (full_ INTEGER)"), mbx.Ok)


def test_prepared_join_reuses_its_plan(fe):
    st = fe.prepare("SELECT COUNT(*) FROM a JOIN b ON a.k = b.w + ? AND a.k <> ? WHERE b.w > ?").value
    for i in range(4):
        for p in (1, 2, 3):
            st.bind_bigint(p, i)
        st.execute()  # no GPU: the statement binds (or patches its plan) and then has nowhere to run
    assert st.plan_stats() == {"binds": 1, "reuses": 3}
    st.close()
