"""VARCHAR predicates on the device (csrc/str_kernels.hip, LowerStringPredicates):
comparisons, BETWEEN, IN, LIKE and starts_with / ends_with / contains over
string columns, in every position a BOOLEAN expression can take.

The expected values come from the model in this file: Python `bytes`
comparison (unsigned bytes, a prefix is smaller), LIKE as the textbook
recurrence over the pattern ('%' any run of bytes, '_' one byte and the
10xxxxxx bytes after it, the escape makes the next byte literal) and None for
NULL with three-valued logic.  Every row of every query is compared.

Shapes: 0, 1, 255, 256, 257 and 4097 rows (a wave step is 256 rows); strings of
0, 1, 15, 16, 17, 31, 32 and 33 bytes (the staging moves 16-byte pieces);
NULLs in 1/7 of the rows and an all-NULL column; multi-byte UTF-8; strings
holding '%', '_' and the escape; one 13000-byte string among short ones and one
whole step of 200-byte rows, neither of which fits a step's 12 KiB LDS region,
and one 6000-byte string that does.  Every string
column of the engine starts at offset 0 of an aligned buffer, so a span start
that is no multiple of 16 is met from the second step on: the fixture asserts
that the first 256 rows of the big tables end off a 16-byte boundary."""
import pytest

from conftest import q
from gpu_tables import fill

pytestmark = pytest.mark.gpu

VOCAB = ["", "a", "abc", "ab", "bc", "abd", "b", "aXbYc", "a_c", "a%c", "50%", "100%!", "\\", "a\\c", "é", "aéc",
         "€uro", "😀", "z", "Zebra", "x" * 15, "y" * 16, "abc" + "z" * 14, "q" * 31, "ab" + "r" * 30, "%" + "s" * 32,
         "abcabc", "ab%", "_", "__", "cab", "abcbc", "aébc", "b😀c"]
assert sorted({len(v.encode()) for v in VOCAB} & {0, 1, 15, 16, 17, 31, 32, 33}) == [0, 1, 15, 16, 17, 31, 32, 33]
SIZES = (0, 1, 255, 256, 257, 4097)


def gen(i):
    """row i of the generated tables: (id, s or None, x)"""
    s = None if i % 7 == 3 else VOCAB[(i * 7 + i // 13) % len(VOCAB)]
    return i, s, (i * 37) % 50


# ---- the model ---------------------------------------------------------------
def B(s):
    return None if s is None else s.encode("utf-8")


def tokens(pat, esc=None):
    out, i = [], 0
    while i < len(pat):
        c = pat[i]
        if esc is not None and c == esc:
            assert i + 1 < len(pat)
            out.append(pat[i + 1])
            i += 2
            continue
        out.append("any" if c == 0x25 else "one" if c == 0x5F else c)
        i += 1
    return out


def like(s, pat, esc=None):
    """s LIKE pat over bytes; m[p][i]: tokens p.. match s[i:]"""
    if s is None or pat is None:
        return None
    tk = tokens(pat, esc)
    n = len(s)
    nxt = [True if i == n else False for i in range(n + 1)]
    for t in reversed(tk):
        cur = [False] * (n + 1)
        for i in range(n, -1, -1):
            if t == "any":
                cur[i] = nxt[i] or (i < n and cur[i + 1])
            elif i < n and t == "one":
                j = i + 1
                while j < n and (s[j] & 0xC0) == 0x80:
                    j += 1
                cur[i] = nxt[j]
            elif i < n:
                cur[i] = s[i] == t and nxt[i + 1]
        nxt = cur
    return nxt[0]


def cmp3(op, a, b):
    if a is None or b is None:
        return None
    return {"=": a == b, "<>": a != b, "<": a < b, "<=": a <= b, ">": a > b, ">=": a >= b}[op]


def not3(a):
    return None if a is None else not a


def and3(a, b):
    if a is False or b is False:
        return False
    return None if a is None or b is None else True


def or3(a, b):
    return not3(and3(not3(a), not3(b)))


def distinct(a, b):
    return (a is None) != (b is None) if a is None or b is None else a != b


def cell(v):
    return "" if v is None else "true" if v else "false"


# ---- tables ------------------------------------------------------------------
class Db:
    pass


@pytest.fixture(scope="module")
def db(mbx):
    cfg = mbx.Config.create()
    cfg.set("mbx_profile", "true")
    r = mbx.connect_with_config(cfg)
    assert isinstance(r, mbx.Ok), r.error.message
    d = Db()
    d.c = r.value
    d.t = {}
    for n in SIZES:
        d.t[n] = [gen(i) for i in range(n)]
        fill(d.c, f"t{n}", "id INTEGER, s VARCHAR, x INTEGER", d.t[n])
    assert sum(len(B(s) or b"") for _, s, _ in d.t[4097][:256]) % 16 != 0
    # step 0 (rows 0..255): a 6000-byte string whose step still fits the region (one lane matches 6 KB out
    # of LDS); step 1 (256..511): a 13000-byte string among short ones; step 2 (512..767): 200-byte rows.
    # Steps 1 and 2 are over the 12 KiB budget and are read from global memory; step 3 on is short again
    big = []
    for i in range(1100):
        _, s, x = gen(i)
        if i == 100:
            s = "ab" + "c" * 5990 + "%b_éabc"
        elif i == 300:
            s = "ab" + "c" * 12990 + "%b_éabc"
        elif 512 <= i < 768 and s is not None:
            s = (s + "abc-" * 50)[:196] + "%abc"
        big.append((i, s, x))
    span = lambda a, b: sum(len(B(s) or b"") for _, s, _ in big[a:b])
    budget = 12 << 10  # kSpanBytes of csrc/str_kernels.hip; the staged span adds at most 15 bytes of round-down
    assert len(B(big[100][1])) >= 6000 and span(0, 256) + 15 <= budget
    assert len(B(big[300][1])) > budget and span(256, 512) > budget and span(512, 768) > budget
    assert span(768, 1024) + 15 <= budget and span(0, 256) % 16 != 0
    d.big = big
    fill(d.c, "tbig", "id INTEGER, s VARCHAR, x INTEGER", big)
    d.nul = [(i, None, i % 5) for i in range(300)]
    fill(d.c, "tnull", "id INTEGER, s VARCHAR, x INTEGER", d.nul)
    # two NULL-able string columns and one without NULLs
    d.cc = []
    for i in range(1000):
        a, b = gen(i)[1], gen(i * 3 + 1)[1]
        if i % 11 == 0:
            b = a
        d.cc.append((i, a, b, VOCAB[(i * 5) % len(VOCAB)]))
    fill(d.c, "tcc", "id INTEGER, a VARCHAR, b VARCHAR, c VARCHAR", d.cc)
    yield d
    d.c.close()


def check(c, table, rows, sql_expr, model):
    """the expression as an output (every row, with NULLs) and as WHERE"""
    want = [model(r) for r in rows]
    res = q(c, f"SELECT id, {sql_expr} FROM {table}")
    assert res.row_count() == len(rows), sql_expr
    got = [None if nl[1] else row[1] == "true" for row, nl in zip(res.rows, res.nulls)]
    bad = [(r, g, w) for r, g, w in zip(rows, got, want) if g is not w]
    assert not bad, (table, sql_expr, len(bad), bad[:5])
    assert [int(row[0]) for row in res.rows] == [r[0] for r in rows]
    ids = [int(row[0]) for row in q(c, f"SELECT id FROM {table} WHERE {sql_expr}").rows]
    assert ids == [r[0] for r, w in zip(rows, want) if w is True], (table, sql_expr)


LIKES = [("'abc'", b"abc", None), ("'ab%'", b"ab%", None), ("'%bc'", b"%bc", None), ("'%b%'", b"%b%", None),
         ("'%'", b"%", None), ("''", b"", None), ("'_'", b"_", None), ("'a_c'", b"a_c", None),
         ("'a%b%c'", b"a%b%c", None), ("'%\\%%' ESCAPE '\\'", b"%\\%%", 0x5C), ("'%é%'", "%é%".encode(), None),
         ("'__'", b"__", None), ("'%c'", b"%c", None), ("'%\\_%' ESCAPE '\\'", b"%\\_%", 0x5C)]


@pytest.mark.parametrize("n", SIZES)
def test_row_counts_every_form(db, n):
    rows, t = db.t[n], f"t{n}"
    for sql, pat, esc in LIKES[:10]:
        check(db.c, t, rows, f"s LIKE {sql}", lambda r: like(B(r[1]), pat, esc))
    check(db.c, t, rows, "s = 'abc'", lambda r: cmp3("=", B(r[1]), b"abc"))
    check(db.c, t, rows, "s < 'b'", lambda r: cmp3("<", B(r[1]), b"b"))
    check(db.c, t, rows, "s IS DISTINCT FROM 'abc'", lambda r: distinct(B(r[1]), b"abc"))
    assert q(db.c, f"SELECT COUNT(*) FROM {t} WHERE s >= 'abc'").rows == \
        [[str(sum(1 for r in rows if cmp3(">=", B(r[1]), b"abc")))]]


def test_comparisons_constant_on_either_side(db):
    rows = db.t[4097]
    flip = {"=": "=", "<>": "<>", "<": ">", "<=": ">=", ">": "<", ">=": "<="}
    for k in ("abc", "", "é", "a_c", "y" * 16, "zz"):
        for op in flip:
            check(db.c, "t4097", rows, f"s {op} '{k}'", lambda r: cmp3(op, B(r[1]), B(k)))
            check(db.c, "t4097", rows, f"'{k}' {op} s", lambda r: cmp3(op, B(k), B(r[1])))
    check(db.c, "t4097", rows, "s IS DISTINCT FROM 'ab'", lambda r: distinct(B(r[1]), b"ab"))
    check(db.c, "t4097", rows, "s IS NOT DISTINCT FROM 'ab'", lambda r: not distinct(B(r[1]), b"ab"))
    check(db.c, "t4097", rows, "'ab' IS NOT DISTINCT FROM s", lambda r: not distinct(B(r[1]), b"ab"))
    # a NULL constant: NULL for the ordinary operators, the column's NULL test for the DISTINCT forms
    check(db.c, "t4097", rows, "s = NULL", lambda r: None)
    check(db.c, "t4097", rows, "s IS DISTINCT FROM NULL", lambda r: r[1] is not None)
    check(db.c, "t4097", rows, "s IS NOT DISTINCT FROM NULL", lambda r: r[1] is None)


def test_between_and_in(db):
    rows = db.t[4097]
    check(db.c, "t4097", rows, "s BETWEEN 'ab' AND 'b'",
          lambda r: and3(cmp3(">=", B(r[1]), b"ab"), cmp3("<=", B(r[1]), b"b")))
    check(db.c, "t4097", rows, "s NOT BETWEEN 'ab' AND 'b'",
          lambda r: not3(and3(cmp3(">=", B(r[1]), b"ab"), cmp3("<=", B(r[1]), b"b"))))
    check(db.c, "t4097", rows, "s IN ('abc', 'é', '')",
          lambda r: None if r[1] is None else r[1] in ("abc", "é", ""))
    inn = lambda r: or3(cmp3("=", B(r[1]), b"abc"), or3(cmp3("=", B(r[1]), b"z"), None))
    check(db.c, "t4097", rows, "s IN ('abc', 'z', NULL)", inn)
    check(db.c, "t4097", rows, "s NOT IN ('abc', 'z', NULL)", lambda r: not3(inn(r)))


def test_like_forms_and_functions(db):
    rows = db.t[4097]
    for sql, pat, esc in LIKES:
        check(db.c, "t4097", rows, f"s LIKE {sql}", lambda r: like(B(r[1]), pat, esc))
        check(db.c, "t4097", rows, f"s NOT LIKE {sql}", lambda r: not3(like(B(r[1]), pat, esc)))
    for fn, mk in (("starts_with", lambda k: k + b"%"), ("prefix", lambda k: k + b"%"), ("ends_with", lambda k: b"%" + k),
                   ("suffix", lambda k: b"%" + k), ("contains", lambda k: b"%" + k + b"%")):
        for k in ("ab", "c", "é", ""):
            check(db.c, "t4097", rows, f"{fn}(s, '{k}')", lambda r: like(B(r[1]), mk(B(k))))
    # the functions take their constant literally
    check(db.c, "t4097", rows, "contains(s, '%')", lambda r: None if r[1] is None else "%" in r[1])
    check(db.c, "t4097", rows, "starts_with(s, '_')", lambda r: None if r[1] is None else r[1].startswith("_"))
    check(db.c, "t4097", rows, "s LIKE NULL", lambda r: None)


def test_spans_over_the_lds_budget(db):
    """the step with the 13000-byte row and the step of 200-byte rows exceed the
    LDS region and are read from global memory inside the same launch; the
    step with the 6000-byte row is staged; the rows after them stay right"""
    rows = db.big
    for sql, pat, esc in LIKES[:10] + [("'%abc'", b"%abc", None), ("'ab%c%'", b"ab%c%", None)]:
        check(db.c, "tbig", rows, f"s LIKE {sql}", lambda r: like(B(r[1]), pat, esc))
    for op in ("=", "<", ">="):
        check(db.c, "tbig", rows, f"s {op} 'abc'", lambda r: cmp3(op, B(r[1]), b"abc"))
    check(db.c, "tbig", rows, f"s = '{rows[600][1]}'", lambda r: cmp3("=", B(r[1]), B(rows[600][1])))
    check(db.c, "tbig", rows, "s IS NOT DISTINCT FROM 'abc'", lambda r: not distinct(B(r[1]), b"abc"))


def test_all_null_column(db):
    for e in ("s = 'a'", "s LIKE 'a%'", "s LIKE '%'", "'a' < s", "contains(s, 'a')"):
        check(db.c, "tnull", db.nul, e, lambda r: None)
    check(db.c, "tnull", db.nul, "s IS DISTINCT FROM 'a'", lambda r: True)
    check(db.c, "tnull", db.nul, "s IS NOT DISTINCT FROM 'a'", lambda r: False)


def test_column_against_column(db):
    rows = db.cc
    for op in ("=", "<>", "<", "<=", ">", ">="):
        check(db.c, "tcc", rows, f"a {op} b", lambda r: cmp3(op, B(r[1]), B(r[2])))      # both NULL-able
        check(db.c, "tcc", rows, f"a {op} c", lambda r: cmp3(op, B(r[1]), B(r[3])))      # one NULL-able
        check(db.c, "tcc", rows, f"c {op} b", lambda r: cmp3(op, B(r[3]), B(r[2])))
    check(db.c, "tcc", rows, "a IS DISTINCT FROM b", lambda r: distinct(B(r[1]), B(r[2])))
    check(db.c, "tcc", rows, "a IS NOT DISTINCT FROM b", lambda r: not distinct(B(r[1]), B(r[2])))
    check(db.c, "tcc", rows, "c IS DISTINCT FROM a", lambda r: distinct(B(r[3]), B(r[1])))
    check(db.c, "tcc", rows, "a = b AND c LIKE '%a%'", lambda r: and3(cmp3("=", B(r[1]), B(r[2])), like(B(r[3]), b"%a%")))


def test_positions(db):
    rows, c = db.t[4097], db.c
    la = lambda r: like(B(r[1]), b"a%")
    check(c, "t4097", rows, "s LIKE 'a%' AND x > 24", lambda r: and3(la(r), r[2] > 24))
    check(c, "t4097", rows, "s = 'abc' OR x < 5", lambda r: or3(cmp3("=", B(r[1]), b"abc"), r[2] < 5))
    check(c, "t4097", rows, "NOT (s LIKE 'a%')", lambda r: not3(la(r)))
    check(c, "t4097", rows, "NOT (s < 'b' AND x > 10)", lambda r: not3(and3(cmp3("<", B(r[1]), b"b"), r[2] > 10)))
    check(c, "t4097", rows, "COALESCE(s = 'abc', x > 40)",
          lambda r: r[2] > 40 if r[1] is None else r[1] == "abc")
    check(c, "t4097", rows, "s LIKE 'a%' AND s LIKE '%c' AND s LIKE 'a%'", lambda r: and3(la(r), like(B(r[1]), b"%c")))
    # CASE
    res = q(c, "SELECT id, CASE WHEN s LIKE 'a%' THEN 1 WHEN s >= 'z' THEN 2 ELSE 0 END FROM t4097")
    assert [int(v[1]) for v in res.rows] == [1 if la(r) else 2 if cmp3(">=", B(r[1]), b"z") else 0 for r in rows]
    # aggregates under a string WHERE
    sel = [r for r in rows if la(r)]
    assert q(c, "SELECT COUNT(*), SUM(x) FROM t4097 WHERE s LIKE 'a%'").rows == [[str(len(sel)), str(sum(r[2] for r in sel))]]
    sel = [r for r in rows if and3(cmp3("=", B(r[1]), b"abc"), r[2] > 10)]
    assert q(c, "SELECT COUNT(*), SUM(x), MIN(id) FROM t4097 WHERE s = 'abc' AND x > 10").rows == \
        [[str(len(sel)), str(sum(r[2] for r in sel)), str(min(r[0] for r in sel))]]
    assert q(c, "SELECT COUNT(*), SUM(x) FROM t4097 WHERE s = 'no such string'").rows == [["0", ""]]
    # an aggregate argument
    assert q(c, "SELECT COUNT(s LIKE 'a%'), SUM(CASE WHEN s LIKE 'a%' THEN x ELSE 0 END) FROM t4097").rows == \
        [[str(sum(1 for r in rows if r[1] is not None)), str(sum(r[2] for r in rows if la(r)))]]
    # a GROUP BY key
    want = {}
    for r in rows:
        k = cell(la(r))
        want[k] = [want.get(k, [0, 0])[0] + 1, want.get(k, [0, 0])[1] + r[2]]
    res = q(c, "SELECT s LIKE 'a%', COUNT(*), SUM(x) FROM t4097 GROUP BY s LIKE 'a%'")
    assert sorted(res.rows) == sorted([k, str(v[0]), str(v[1])] for k, v in want.items()) and len(res.rows) == 3
    # HAVING over a VARCHAR group key
    cnt = {}
    for r in rows:
        cnt[r[1]] = cnt.get(r[1], 0) + 1
    res = q(c, "SELECT s, COUNT(*) FROM t4097 GROUP BY s HAVING s LIKE 'a%' AND s <> 'abc' ORDER BY s")
    assert res.rows == [[k, str(cnt[k])] for k in sorted((k for k in cnt if k is not None), key=B)
                        if like(B(k), b"a%") and k != "abc"]
    # a subquery's string column (not a table column) and ORDER BY / LIMIT around the filter
    res = q(c, "SELECT id FROM (SELECT id, s FROM t4097 WHERE x > 10) u WHERE s LIKE '%c' ORDER BY id DESC LIMIT 7")
    assert [int(v[0]) for v in res.rows] == [r[0] for r in reversed(rows) if r[2] > 10 and like(B(r[1]), b"%c")][:7]


def test_arrow_and_stream(db, mbx):
    rows, c = db.t[4097], db.c
    a = c.query_arrow("SELECT id, s LIKE 'a%', s >= 'b' FROM t4097").value
    for col, model in ((1, lambda r: like(B(r[1]), b"a%")), (2, lambda r: cmp3(">=", B(r[1]), b"b"))):
        vals, valid = a.get_column_bool_nullable(col)
        assert [v if ok else None for v, ok in zip(vals, valid)] == [model(r) for r in rows]
    a.close()
    a = c.query_arrow("SELECT id FROM t4097 WHERE s LIKE '%b%'").value
    assert a.get_column_int32(0) == [r[0] for r in rows if like(B(r[1]), b"%b%")]
    a.close()
    st = c.query_stream("SELECT id, s FROM t4097 WHERE ends_with(s, 'c')").value
    got = []
    while True:
        ch = st.next().value
        if ch is None:
            break
        got.extend((int(row[0]), row[1]) for row in ch.rows)
    st.close()
    assert got == [(r[0], r[1]) for r in rows if like(B(r[1]), b"%c")]


def test_prepared_statements_reuse_the_plan(db):
    rows, c = db.t[4097], db.c
    st = c.prepare("SELECT COUNT(*), SUM(x) FROM t4097 WHERE s = ?").value
    for k in ("abc", "é"):
        st.bind_varchar(1, k)
        sel = [r for r in rows if r[1] == k]
        assert st.execute().value.rows == [[str(len(sel)), str(sum(r[2] for r in sel))]], k
    assert st.plan_stats() == {"binds": 1, "reuses": 1}
    st.close()
    st = c.prepare("SELECT id FROM t4097 WHERE s LIKE ?").value
    for k in ("ab%", "%c", "a_c"):
        st.bind_varchar(1, k)
        assert [int(v[0]) for v in st.execute().value.rows] == [r[0] for r in rows if like(B(r[1]), B(k))], k
    assert st.plan_stats() == {"binds": 1, "reuses": 2}
    st.close()


def test_profile_names_the_kernel(db):
    c = db.c
    names = lambda: [k["name"] for k in c.last_profile()["kernels"]]
    q(c, "SELECT COUNT(*) FROM t4097 WHERE s = 'abc'")
    assert "str_match" in names()
    q(c, "SELECT id FROM tcc WHERE a < b")
    assert "str_match" in names()
    # LIKE '%' over a column without NULLs is true for every row: nothing to launch
    assert q(c, "SELECT COUNT(*) FROM tcc WHERE c LIKE '%'").rows == [["1000"]]
    assert "str_match" not in names()
    # the same leaf twice is evaluated once
    q(c, "SELECT id, s LIKE 'a%' FROM t4097 WHERE s LIKE 'a%'")
    assert names().count("str_match") == 1


def test_string_expressions_keep_their_error(db, mbx):
    r = db.c.query("SELECT id FROM t4097 WHERE lower(s) = 'abc'")
    assert isinstance(r, mbx.Err) and r.error.message.startswith("Not implemented Error"), r
    assert "string expression" in r.error.message


def test_sharded(db, mbx):
    """a string WHERE under COUNT and under a row SELECT over a 2-shard table:
    equal to the unsharded answer and to the model"""
    n = 20011
    ctas = ("CREATE TABLE h AS SELECT i AS id, CASE WHEN i % 7 = 3 THEN NULL WHEN i % 5 = 0 THEN 'apple' "
            "WHEN i % 5 = 1 THEN 'apricot' WHEN i % 5 = 2 THEN 'fig' WHEN i % 5 = 3 THEN 'grape%' ELSE '' END AS s, "
            f"i % 50 AS x FROM range({n}) tbl(i)")
    words = ["apple", "apricot", "fig", "grape%", ""]
    rows = [(i, None if i % 7 == 3 else words[i % 5], i % 50) for i in range(n)]
    cfg = mbx.Config.create()
    assert isinstance(cfg.set("gpu_devices", "0,0"), mbx.Ok)
    sc = mbx.connect_with_config(cfg).value
    q(sc, ctas)
    q(db.c, ctas)
    for where, model in (("s LIKE 'ap%'", lambda r: like(B(r[1]), b"ap%")), ("s >= 'fig' AND x > 24",
                         lambda r: and3(cmp3(">=", B(r[1]), b"fig"), r[2] > 24)),
                         ("s LIKE '%\\%' ESCAPE '\\' OR s = ''", lambda r: or3(like(B(r[1]), b"%\\%", 0x5C),
                                                                             cmp3("=", B(r[1]), b"")))):
        sel = [r for r in rows if model(r) is True]
        for sql, want in ((f"SELECT COUNT(*), SUM(x) FROM h WHERE {where}", [[str(len(sel)), str(sum(r[2] for r in sel))]]),
                          (f"SELECT id, s FROM h WHERE {where}", [[str(r[0]), r[1]] for r in sel])):
            got = q(sc, sql).rows
            assert got == want, sql
            assert q(db.c, sql).rows == got, sql
    sc.close()
    q(db.c, "DROP TABLE h")
