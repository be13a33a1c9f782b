"""Window functions in the front end: parser, binder and EXPLAIN, on a
connection without a GPU.  The tables are empty (DDL only), so every statement
binds and nothing executes.  What is checked is the bound plan: one WINDOW
line per distinct call --

  WINDOW f(arg[, offset]) [PARTITION BY e, ..] [ORDER BY e ASC|DESC NULLS FIRST|LAST, ..]
         FRAME <resolved frame> SPEC <specification number> :: <result type>

with the resolved frame spelled ROWS TO CURRENT ROW (the running value; also
what the rank functions, LAG and LEAD print: they ignore the frame), RANGE TO
CURRENT ROW (up to the last peer) or WHOLE PARTITION -- the result types, the
sharing of calls and specifications, every form that stays refused by the word
that names it, the Binder errors, and that the window keywords are still names."""
import pytest


@pytest.fixture()
def fe(hostconn, mbx):
    for ddl in ("CREATE TABLE t (k BIGINT, v INTEGER, s VARCHAR, d DOUBLE, h HUGEINT, big DECIMAL(38,2), "
                "iv INTERVAL, dc DECIMAL(10,2), rows INTEGER, f FLOAT)",
                "CREATE TABLE b (k TINYINT, w BIGINT)"):
        assert isinstance(hostconn.query(ddl), mbx.Ok)
    return hostconn


def windows(plan):
    return [ln.strip() for ln in plan.splitlines() if ln.strip().startswith("WINDOW ")]


def test_explain_of_each_function(fe):
    spec = "PARTITION BY #0 ORDER BY #1 ASC NULLS LAST"
    for sql, line in (
            ("row_number()", f"WINDOW row_number() {spec} FRAME ROWS TO CURRENT ROW SPEC 0 :: BIGINT"),
            ("rank()", f"WINDOW rank() {spec} FRAME ROWS TO CURRENT ROW SPEC 0 :: BIGINT"),
            ("dense_rank()", f"WINDOW dense_rank() {spec} FRAME ROWS TO CURRENT ROW SPEC 0 :: BIGINT"),
            ("count(*)", f"WINDOW count_star() {spec} FRAME RANGE TO CURRENT ROW SPEC 0 :: BIGINT"),
            ("count(s)", None),
            ("count(v)", f"WINDOW count(#1) {spec} FRAME RANGE TO CURRENT ROW SPEC 0 :: BIGINT"),
            ("sum(v)", f"WINDOW sum(#1) {spec} FRAME RANGE TO CURRENT ROW SPEC 0 :: HUGEINT"),
            ("sum(dc)", f"WINDOW sum(#7) {spec} FRAME RANGE TO CURRENT ROW SPEC 0 :: DECIMAL(38,2)"),
            ("sum(f)", f"WINDOW sum(CAST(#9 AS DOUBLE)) {spec} FRAME RANGE TO CURRENT ROW SPEC 0 :: DOUBLE"),
            ("min(h)", f"WINDOW min(#4) {spec} FRAME RANGE TO CURRENT ROW SPEC 0 :: HUGEINT"),
            ("max(d)", f"WINDOW max(#3) {spec} FRAME RANGE TO CURRENT ROW SPEC 0 :: DOUBLE"),
            ("avg(v)", f"WINDOW avg(#1) {spec} FRAME RANGE TO CURRENT ROW SPEC 0 :: DOUBLE"),
            ("lag(big)", f"WINDOW lag(#5, 1) {spec} FRAME ROWS TO CURRENT ROW SPEC 0 :: DECIMAL(38,2)"),
            ("lead(v, 3)", f"WINDOW lead(#1, 3) {spec} FRAME ROWS TO CURRENT ROW SPEC 0 :: INTEGER"),
            ("lag(v, 0)", f"WINDOW lag(#1, 0) {spec} FRAME ROWS TO CURRENT ROW SPEC 0 :: INTEGER")):
        if line is None:
            continue  # (a VARCHAR argument: refused, below)
        plan = fe.explain(f"SELECT {sql} OVER (PARTITION BY k ORDER BY v) FROM t")
        assert windows(plan) == [line], (sql, plan)


FRAMES = [("", "WHOLE PARTITION", "RANGE TO CURRENT ROW"),
          ("ROWS BETWEEN UNBOUNDED PRECEDING AND CURRENT ROW", "ROWS TO CURRENT ROW", "ROWS TO CURRENT ROW"),
          ("ROWS UNBOUNDED PRECEDING", "ROWS TO CURRENT ROW", "ROWS TO CURRENT ROW"),
          # without ORDER BY every row of a partition is a peer of every other
          ("RANGE BETWEEN UNBOUNDED PRECEDING AND CURRENT ROW", "WHOLE PARTITION", "RANGE TO CURRENT ROW"),
          ("RANGE UNBOUNDED PRECEDING", "WHOLE PARTITION", "RANGE TO CURRENT ROW"),
          ("ROWS BETWEEN UNBOUNDED PRECEDING AND UNBOUNDED FOLLOWING", "WHOLE PARTITION", "WHOLE PARTITION"),
          ("RANGE BETWEEN UNBOUNDED PRECEDING AND UNBOUNDED FOLLOWING", "WHOLE PARTITION", "WHOLE PARTITION")]


@pytest.mark.parametrize("frame,unordered,ordered", FRAMES)
def test_accepted_frames_resolve(fe, frame, unordered, ordered):
    plan = fe.explain(f"SELECT sum(v) OVER (PARTITION BY k {frame}) FROM t")
    assert windows(plan) == [f"WINDOW sum(#1) PARTITION BY #0 FRAME {unordered} SPEC 0 :: HUGEINT"]
    plan = fe.explain(f"SELECT sum(v) OVER (ORDER BY k DESC {frame}) FROM t")
    assert windows(plan) == [f"WINDOW sum(#1) ORDER BY #0 DESC NULLS LAST FRAME {ordered} SPEC 0 :: HUGEINT"]
    # the rank functions ignore the frame
    plan = fe.explain(f"SELECT rank() OVER (ORDER BY k {frame}) FROM t")
    assert windows(plan) == ["WINDOW rank() ORDER BY #0 ASC NULLS LAST FRAME ROWS TO CURRENT ROW SPEC 0 :: BIGINT"]


def test_over_without_anything_and_without_from(fe):
    assert windows(fe.explain("SELECT count(*) OVER () FROM t")) == ["WINDOW count_star() FRAME WHOLE PARTITION SPEC 0 :: BIGINT"]
    plan = fe.explain("SELECT ROW_NUMBER() OVER ()")
    assert "FROM <one row>" in plan and "[device]" in plan  # never host-constant
    assert windows(plan) == ["WINDOW row_number() FRAME ROWS TO CURRENT ROW SPEC 0 :: BIGINT"]


def test_null_placement_and_direction_print(fe):
    plan = fe.explain("SELECT rank() OVER (ORDER BY k DESC NULLS FIRST, v NULLS FIRST, d ASC NULLS LAST) FROM t")
    assert "ORDER BY #0 DESC NULLS FIRST, #1 ASC NULLS FIRST, #3 ASC NULLS LAST" in windows(plan)[0]


def test_output_names_and_types(fe):
    plan = fe.explain("SELECT k, sum(v) OVER (ORDER BY k) AS run, avg(v) OVER (), rank() OVER (ORDER BY v) FROM t")
    # the outputs read [source columns (10), window results]
    assert plan.splitlines()[0] == ("SELECT #0 AS k :: BIGINT, #10 AS run :: HUGEINT, #11 AS avg(v) OVER () :: DOUBLE, "
                                    "#12 AS rank() OVER (ORDER BY v) :: BIGINT")


def test_identical_calls_bind_once(fe):
    plan = fe.explain("SELECT sum(v) OVER (PARTITION BY k ORDER BY v), SUM(v) OVER (PARTITION BY k ORDER BY v ASC NULLS LAST) + 1 FROM t")
    assert len(windows(plan)) == 1
    assert plan.splitlines()[0].startswith("SELECT #10 AS ")
    assert "(#10 + 1)" in plan.splitlines()[0]
    # an explicit frame equal to the default is the same call
    plan = fe.explain("SELECT sum(v) OVER (ORDER BY k), sum(v) OVER (ORDER BY k RANGE UNBOUNDED PRECEDING) FROM t")
    assert len(windows(plan)) == 1


def test_calls_with_one_specification_share_it(fe):
    plan = fe.explain("SELECT row_number() OVER (PARTITION BY k ORDER BY v), sum(v) OVER (PARTITION BY k ORDER BY v), "
                      "sum(v) OVER (PARTITION BY k ORDER BY v DESC), count(*) OVER (), lag(d) OVER (PARTITION BY k ORDER BY v) FROM t")
    assert [ln.split(" SPEC ")[1].split(" ")[0] for ln in windows(plan)] == ["0", "0", "1", "2", "0"]


def test_window_inside_arithmetic(fe):
    plan = fe.explain("SELECT v - lag(v) OVER (ORDER BY k), 100 * sum(v) OVER (PARTITION BY k) / sum(v) OVER () FROM t")
    assert plan.splitlines()[0].startswith("SELECT (#1 - #10) AS ")
    assert "(CAST((100 * #11) AS DOUBLE) / CAST(#12 AS DOUBLE))" in plan.splitlines()[0]
    assert len(windows(plan)) == 3


def test_key_and_argument_expressions(fe):
    plan = fe.explain("SELECT sum(v * 2) OVER (PARTITION BY k % 3 ORDER BY -v) FROM t")
    assert windows(plan) == ["WINDOW sum((#1 * 2)) PARTITION BY (#0 % 3) ORDER BY -(#1) ASC NULLS LAST "
                             "FRAME RANGE TO CURRENT ROW SPEC 0 :: HUGEINT"]


def test_window_over_a_group_by_subquery(fe):
    # an aggregating select takes no window call; its aggregate goes into a subquery
    plan = fe.explain("SELECT k, c, RANK() OVER (ORDER BY c DESC) FROM (SELECT k, COUNT(*) c FROM t GROUP BY k) g")
    assert windows(plan) == ["WINDOW rank() ORDER BY #1 DESC NULLS LAST FRAME ROWS TO CURRENT ROW SPEC 0 :: BIGINT"]
    assert "AGGREGATE groups=[#0]" in plan
    plan = fe.explain("SELECT k, s, RANK() OVER (ORDER BY s DESC) FROM (SELECT k, SUM(d) s FROM t GROUP BY k) g")
    assert len(windows(plan)) == 1
    # SUM of an integer is a HUGEINT, which no key may be: the subquery casts it
    plan = fe.explain("SELECT k, s, RANK() OVER (ORDER BY s DESC) FROM (SELECT k, SUM(v)::BIGINT s FROM t GROUP BY k) g")
    assert len(windows(plan)) == 1
    with pytest.raises(Exception, match="Not implemented Error.*key of type HUGEINT"):
        fe.explain("SELECT k, s, RANK() OVER (ORDER BY s DESC) FROM (SELECT k, SUM(v) s FROM t GROUP BY k) g")


def test_window_over_join_union_order_limit(fe):
    plan = fe.explain("SELECT t.v, row_number() OVER (PARTITION BY b.w ORDER BY t.v) FROM t JOIN b ON t.k = b.k")
    assert "HASH JOIN" in plan and windows(plan)[0].startswith("WINDOW row_number() PARTITION BY #11 ORDER BY #1 ASC")
    plan = fe.explain("SELECT k FROM t UNION ALL SELECT rank() OVER (ORDER BY k) FROM t")
    assert "UNION ALL" in plan and len(windows(plan)) == 1
    plan = fe.explain("SELECT k, rank() OVER (ORDER BY v) r FROM t ORDER BY r DESC, 1 LIMIT 3")
    assert "ORDER BY #1 DESC" in plan and "LIMIT 3" in plan


REFUSED = [
    ("SELECT sum(v) OVER (ORDER BY k ROWS BETWEEN 1 PRECEDING AND CURRENT ROW) FROM t", "n PRECEDING"),
    ("SELECT sum(v) OVER (ORDER BY k ROWS BETWEEN UNBOUNDED PRECEDING AND 1 FOLLOWING) FROM t", "n FOLLOWING"),
    ("SELECT sum(v) OVER (ORDER BY k RANGE BETWEEN CURRENT ROW AND UNBOUNDED FOLLOWING) FROM t", "starts anywhere but UNBOUNDED PRECEDING"),
    ("SELECT sum(v) OVER (ORDER BY k ROWS CURRENT ROW) FROM t", "starts anywhere but UNBOUNDED PRECEDING"),
    ("SELECT sum(v) OVER (ORDER BY k GROUPS UNBOUNDED PRECEDING) FROM t", "GROUPS"),
    ("SELECT sum(v) OVER (ORDER BY k ROWS UNBOUNDED PRECEDING EXCLUDE CURRENT ROW) FROM t", "EXCLUDE"),
    ("SELECT ntile(4) OVER (ORDER BY k) FROM t", "NTILE"),
    ("SELECT first_value(v) OVER (ORDER BY k) FROM t", "FIRST_VALUE"),
    ("SELECT last_value(v) OVER (ORDER BY k) FROM t", "LAST_VALUE"),
    ("SELECT nth_value(v, 2) OVER (ORDER BY k) FROM t", "NTH_VALUE"),
    ("SELECT percent_rank() OVER (ORDER BY k) FROM t", "PERCENT_RANK"),
    ("SELECT cume_dist() OVER (ORDER BY k) FROM t", "CUME_DIST"),
    ("SELECT lag(v, 1, 0) OVER (ORDER BY k) FROM t", "third \\(default\\) argument"),
    ("SELECT lead(v, -1) OVER (ORDER BY k) FROM t", "negative offset"),
    ("SELECT lag(v, v) OVER (ORDER BY k) FROM t", "non-constant offset"),
    ("SELECT sum(v) OVER w FROM t WINDOW w AS (ORDER BY k)", "named windows"),
    ("SELECT sum(v) OVER (w ORDER BY k) FROM t", "named windows"),
    ("SELECT k FROM t WINDOW w AS (ORDER BY k)", "named windows"),
    ("SELECT k FROM t QUALIFY row_number() OVER (ORDER BY k) = 1", "QUALIFY"),
    ("SELECT count(DISTINCT v) OVER (PARTITION BY k) FROM t", "DISTINCT inside a window aggregate"),
    ("SELECT rank() OVER (ORDER BY s) FROM t", "key of type VARCHAR"),
    ("SELECT rank() OVER (PARTITION BY h) FROM t", "key of type HUGEINT"),
    ("SELECT rank() OVER (ORDER BY big) FROM t", "key of type DECIMAL\\(38,2\\)"),
    ("SELECT rank() OVER (PARTITION BY iv) FROM t", "key of type INTERVAL"),
    ("SELECT min(s) OVER (PARTITION BY k) FROM t", "argument of type VARCHAR"),
    ("SELECT lag(s) OVER (ORDER BY k) FROM t", "argument of type VARCHAR"),
    ("SELECT max(iv) OVER (ORDER BY k) FROM t", "argument of type INTERVAL"),
    ("SELECT k, count(*), rank() OVER (ORDER BY k) FROM t GROUP BY k", "select that also aggregates"),
    ("SELECT sum(v), rank() OVER () FROM t", "select that also aggregates"),
    ("SELECT rank() OVER (ORDER BY sum(v)) FROM t", "select that also aggregates"),
    ("SELECT DISTINCT rank() OVER (ORDER BY k) FROM t", "select that also aggregates"),
    ("SELECT k FROM t ORDER BY rank() OVER (ORDER BY k)", "ORDER BY that is not also an output column"),
    ("SELECT sum(v) FILTER (WHERE v > 1) FROM t", "FILTER"),
    ("SELECT sum(v) FILTER (WHERE v > 1) OVER (ORDER BY k) FROM t", "FILTER"),
]


@pytest.mark.parametrize("sql,word", REFUSED, ids=[f"{i}-{w[:24]}" for i, (_, w) in enumerate(REFUSED)])
def test_refused_forms_name_what_they_refuse(fe, sql, word):
    with pytest.raises(Exception, match="Not implemented Error.*" + word):
        fe.explain(sql)


def test_filter_message_names_only_filter(fe):
    with pytest.raises(Exception) as ei:
        fe.explain("SELECT sum(v) FILTER (WHERE v > 1) FROM t")
    assert "FILTER" in str(ei.value) and "window" not in str(ei.value)


def test_binder_errors(fe):
    for sql, msg in (("SELECT k FROM t WHERE rank() OVER (ORDER BY k) = 1", "WHERE clause cannot contain window functions"),
                     ("SELECT k FROM t GROUP BY rank() OVER (ORDER BY k)", "GROUP BY clause cannot contain window functions"),
                     ("SELECT k FROM t GROUP BY k HAVING rank() OVER (ORDER BY k) = 1", "HAVING clause cannot contain window functions"),
                     ("SELECT 1 FROM t JOIN b ON t.k = b.k AND rank() OVER (ORDER BY b.w) = 1", "JOIN condition cannot contain window functions"),
                     ("SELECT sum(rank() OVER (ORDER BY k)) OVER () FROM t", "window function calls cannot be nested"),
                     ("SELECT rank() OVER (ORDER BY row_number() OVER ()) FROM t", "window function calls cannot be nested"),
                     ("SELECT rank() OVER (PARTITION BY lag(v) OVER (ORDER BY k)) FROM t", "window function calls cannot be nested"),
                     ("SELECT rank(k) OVER (ORDER BY k) FROM t", "rank\\(\\) takes no arguments"),
                     ("SELECT dense_rank(1) OVER (ORDER BY k) FROM t", "dense_rank\\(\\) takes no arguments"),
                     ("SELECT rank() OVER (ORDER BY nope) FROM t", "nope")):
        with pytest.raises(Exception, match="Binder Error.*" + msg):
            fe.explain(sql)


def test_window_keywords_are_still_names(fe, mbx):
    assert fe.explain("SELECT rows FROM t").splitlines()[0] == "SELECT #8 AS rows :: INTEGER"
    assert "RANGE(0, 3, 1)" in fe.explain("SELECT range FROM range(3)")
    assert fe.explain("SELECT over.k FROM t AS over").splitlines()[0] == "SELECT #0 AS k :: BIGINT"
    assert isinstance(fe.query("CREATE TABLE kw (partition INTEGER, preceding INTEGER, unbounded INTEGER, following INTEGER, "
                               "current INTEGER, range INTEGER)"), mbx.Ok)
    plan = fe.explain("SELECT partition, preceding + unbounded, following, current, range FROM kw")
    assert plan.splitlines()[0].startswith("SELECT #0 AS partition :: INTEGER, (#1 + #2) AS ")
    # and inside a window: a column called rows as key and argument
    plan = fe.explain("SELECT sum(rows) OVER (PARTITION BY rows ORDER BY rows ROWS UNBOUNDED PRECEDING) FROM t")
    assert windows(plan) == ["WINDOW sum(#8) PARTITION BY #8 ORDER BY #8 ASC NULLS LAST FRAME ROWS TO CURRENT ROW SPEC 0 :: HUGEINT"]


def test_prepared_window_argument_keeps_consistent_stats(fe):
    st = fe.prepare("SELECT sum(v + ?) OVER (PARTITION BY k ORDER BY v) FROM t WHERE v > ?").value
    for i in range(4):
        st.bind_bigint(1, i)
        st.bind_bigint(2, 10 * i)
        st.execute()  # no GPU: the statement binds (or patches its plan) and then has nowhere to run
    stats = st.plan_stats()
    # the parameters live in nodes of the plan (the window's argument tree is walked), so the plan is patched
    assert stats == {"binds": 1, "reuses": 3}
    st.close()
    # a parameter the binder consumes (the offset) leaves no node: every execution binds again
    st = fe.prepare("SELECT lag(v, ?) OVER (ORDER BY k) FROM t").value
    for i in range(3):
        st.bind_bigint(1, i)
        st.execute()
    assert st.plan_stats() == {"binds": 3, "reuses": 0}
    st.close()
