"""The hash GROUP BY (HashAggregate, hash_insert_kernel, csrc/group_hash.h) on
every key type, VARCHAR above all: the last path of Aggregate(), the only one
that hashes and compares strings on the device.

The model is a Python dict over the same rows, never another connection of the
engine.  Every statement asserts hash_group_assign in the profile's kernel list
and that no group_part* kernel ran; rows are compared as sets (the order is
undefined), every key must appear once and only once, NULL cells are told from
'' by the null flags, float key cells are read as raw bytes.

  a. the string edge table: lengths 0 .. 4 097 around the 8- and 16-byte and
     256-byte marks, keys that differ only in length, in the last or the first
     byte, multi-byte UTF-8, '' beside NULL;
  b. two VARCHAR keys whose bytes concatenate alike;
  c. every fixed-width key type at its extremes, each beside a VARCHAR key;
     eight keys; nine keys and an INTERVAL key are refused cleanly;
  d. 70 001 rows: all keys distinct, 1 024 and 1 025 keys (the LDS /
     group_reduce switch of the second stage), one key, two keys alternating;
  e. the table's capacity steps: 512, 513, 1 024, 1 025 distinct BIGINT keys;
  f. crafted chains (hash_group_model): 250 keys with home slot 1023 of 1024,
     120 pairs of keys with equal tag and home slot; BIGINT and 8-byte strings;
  g. keys from UNION ALL, a join's gathered column, a subquery, a CASE, an
     appended table; empty inputs; one row; VARCHAR columns that hold no
     character at all (only NULLs, only '');
  h. two shards: the host merge by key.

DOUBLE sums are held to 1e-9 * sum|x| of math.fsum ("Floating-point
sums"; every input's sum|x| is below 1e300), MIN / MAX of DOUBLE to the bit
pattern, everything else is exact."""
import math
import struct
from fractions import Fraction

import pytest

import agg_model as M
import hash_group_model as H
import vm_cases as V
import vm_reference as R
from conftest import q
from gpu_tables import fill, kernels, load

pytestmark = pytest.mark.gpu

NAN, NEG_NAN, INF, SUB = math.nan, R.from_bits(0xFFF8000000000001), math.inf, 5e-324
KD = [0.0, -0.0, NAN, NEG_NAN, INF, -INF, SUB, 1.5, -2.5]  # as test_gpu_aggregate_values: seven groups


@pytest.fixture(autouse=True)
def no_jit(monkeypatch):
    monkeypatch.setenv("MBX_JIT", "0")


def connect(mbx, **opts):
    cfg = mbx.Config.create()
    for k, v in dict(mbx_profile="true", **opts).items():
        assert isinstance(cfg.set(k, str(v)), mbx.Ok), (k, v)
    r = mbx.connect_with_config(cfg)
    assert isinstance(r, mbx.Ok), r.error.message
    return r.value


def on_hash_path(c, sql=""):
    ks = kernels(c)
    assert "hash_group_assign" in ks, (sql, ks)
    assert not any(k.startswith("group_part") for k in ks), (sql, ks)
    return ks


def _float(raw):
    return struct.unpack("<d", raw)[0] if len(raw) == 8 else struct.unpack("<f", raw)[0]


def ints(vals):
    """COUNT(*), COUNT(v), SUM(v), MIN(v), MAX(v) of Python ints (None: NULL), as result cells (None: NULL)"""
    xs = [v for v in vals if v is not None]
    return [str(len(vals)), str(len(xs))] + ([str(sum(xs)), str(min(xs)), str(max(xs))] if xs else [None] * 3)


INTS = "COUNT(*), COUNT(v), SUM(v), MIN(v), MAX(v)"


def group(rows, nk):
    """{key tuple: [the value column]} over rows (key..., v)"""
    out = {}
    for r in rows:
        out.setdefault(M.key_of(tuple(r[:nk])), []).append(r[nk])
    return out


def result(c, sql, nk, decode=None):
    """{key tuple: the row's other cells (None for NULL)} of a statement whose first nk columns are the
    keys; a key twice is an error.  decode[g](text, raw) turns key cell g into the model's value"""
    res = c.query_raw(sql)
    try:
        text, nulls = res.cells()
        out = {}
        for i in range(res.row_count()):
            key = []
            for g in range(nk):
                if nulls[i][g]:
                    key.append(None)
                elif decode and decode[g]:
                    key.append(decode[g](text[i][g], lambda g=g, i=i: res.raw(g, i)))
                else:
                    key.append(text[i][g])
            key = M.key_of(tuple(key))
            assert key not in out, (sql, "group twice", key)
            out[key] = [None if n else t for t, n in zip(text[i][nk:], nulls[i][nk:])]
        return out
    finally:
        res.close()


def check(c, sql, nk, want, decode=None):
    """the statement against {key tuple: expected cells}"""
    got = result(c, sql, nk, decode)
    ks = on_hash_path(c, sql)
    assert set(got) == set(want), (sql, sorted(map(repr, set(got) ^ set(want)))[:10])
    for k, cells in want.items():
        assert got[k] == cells, (sql, k, got[k], cells)
    return ks


def decoder_int(text, raw):
    return int(text)


# ---- a. the string edge table ---------------------------------------------------------------------
def edge_keys():
    alpha = "".join(chr(97 + (i * 7) % 26) for i in range(4097))
    keys = [None]
    for n in (0, 1, 7, 8, 9, 15, 16, 17, 255, 256, 257, 4097):
        s = alpha[:n]  # each a prefix of the next: they differ only in length
        keys.append(s)
        if n:
            keys.append(s[:-1] + "#")  # only the last byte differs (for 4 097 bytes: byte 4 096)
            keys.append("#" + s[1:])   # only the first
    keys = list(dict.fromkeys(keys))  # (at one byte the two variants are one string)
    # two-, three- and four-byte UTF-8 characters, beside their ASCII look-alikes and each other
    keys += ["é", "e", "éé", "é" * 8, "€", "€uro", "\U0001F600", "\U0001F600\U0001F600", "e\u0301", "aé", "a€", "日本語", "日本"]
    assert len(keys) == len(set(keys)) and all(k is None or "\0" not in k for k in keys)
    return keys


EDGE_N = 3000


def edge_rows():
    """(s, v): every key about 60 times in scattered order; two keys live only at the table's two ends (for
    the shards); v is NULL in every 11th row"""
    keys = edge_keys()
    rows = []
    for r in range(EDGE_N):
        s = "only at the start" if r < 5 else "only at the end" if r >= EDGE_N - 5 else keys[(r * 7919 + r // 13) % len(keys)]
        rows.append((s, None if r % 11 == 3 else (r * 37) % 1001 - 500))
    assert {s for s, _ in rows} == set(keys) | {"only at the start", "only at the end"}
    return rows


def check_edge_table(c):
    rows = edge_rows()
    want = {k: ints(v) for k, v in group(rows, 1).items()}
    assert (None,) in want and ("",) in want and len(want) == len(edge_keys()) + 2
    check(c, f"SELECT s, {INTS} FROM edge GROUP BY s", 1, want)
    kept = [r for r in rows if r[1] is not None and r[1] % 3 != 0]
    check(c, f"SELECT s, {INTS} FROM edge WHERE v % 3 <> 0 GROUP BY s", 1, {k: ints(v) for k, v in group(kept, 1).items()})
    check(c, "SELECT DISTINCT s FROM edge", 1, {k: [] for k in want})
    assert q(c, "SELECT COUNT(DISTINCT s), COUNT(s) FROM edge").rows == \
        [[str(len(want) - 1), str(sum(s is not None for s, _ in rows))]]
    on_hash_path(c, "COUNT(DISTINCT s)")


@pytest.fixture(scope="module")
def edge(mbx):
    c = connect(mbx)
    fill(c, "edge", "s VARCHAR, v BIGINT", edge_rows())
    yield c
    c.close()


def test_edge_keys_are_what_the_cases_need():
    keys = [k for k in edge_keys() if k is not None]
    assert {0, 1, 7, 8, 9, 15, 16, 17, 255, 256, 257, 4097} <= {len(k.encode()) for k in keys}
    long = [k for k in keys if len(k) == 4097]
    assert any(a[:4096] == b[:4096] and a[4096] != b[4096] for a in long for b in long)
    assert any(a[1:] == b[1:] and a[0] != b[0] for a in long for b in long)
    assert {len(k.encode()) // len(k) for k in ("é", "€", "\U0001F600")} == {2, 3, 4}


def test_string_edge_table(edge):
    check_edge_table(edge)


# ---- b. two VARCHAR keys ----------------------------------------------------------------------------
SEVEN = [("ab", "c"), ("a", "bc"), ("", "abc"), (None, "abc"), ("abc", None), (None, None), ("", None)]


def pair_rows():
    rows = []
    for i in range(500):
        rows.append((f"a{i % 25}", f"b{(i * 7) % 20}" if i % 17 else None, i))
        if i % 14 == 0:
            rows.append(SEVEN[(i // 14) % 7] + (1000 + i,))
    assert all(sum(r[:2] == k for r in rows) >= 5 for k in SEVEN)
    return rows


def check_pairs(c):
    rows = pair_rows()
    want = {k: ints(v) for k, v in group(rows, 2).items()}
    assert all(k in want for k in SEVEN)
    check(c, f"SELECT a, b, {INTS} FROM ab GROUP BY a, b", 2, want)
    check(c, "SELECT DISTINCT a, b FROM ab", 2, {k: [] for k in want})


def test_two_varchar_keys(mbx):
    c = connect(mbx)
    fill(c, "ab", "a VARCHAR, b VARCHAR, v BIGINT", pair_rows())
    check_pairs(c)
    c.close()


# ---- c. every key type, beside a VARCHAR key ------------------------------------------------------------
I64, U64, H127, D38 = 2 ** 63, 2 ** 64, 2 ** 127, 10 ** 38 - 1
TYPE_EDGES = {
    "b": ("BOOLEAN", [True, False]),
    "i8": ("TINYINT", [-128, 127, 0, -1]),
    "i16": ("SMALLINT", [-32768, 32767, 0, -1]),
    "i32": ("INTEGER", [-2 ** 31, 2 ** 31 - 1, 0, -1]),
    "i64": ("BIGINT", [-I64, I64 - 1, 0, -1, 2 ** 32, -2 ** 32]),
    "u8": ("UTINYINT", [0, 255, 128, 127]),
    "u16": ("USMALLINT", [0, 65535, 32768, 32767]),
    "u32": ("UINTEGER", [0, 2 ** 32 - 1, 2 ** 31, 2 ** 31 - 1]),
    "u64": ("UBIGINT", [0, I64 - 1, I64, U64 - 1, 1]),
    "h": ("HUGEINT", [1, U64 + 1, -1, U64 - 1, -H127, H127 - 1]),  # equal low words under different high words
    "m": ("DECIMAL(38,2)", [1, U64 + 1, -1, U64 - 1, -D38, D38]),
    "dt": ("DATE", [-25567, -1, 0, 1, 19000, 47482]),
    "ts": ("TIMESTAMP", [0, -1, 1, 1700000000000000, 1700000000000001, -2208988800000000]),
    "f": ("FLOAT", [16777216.0, 16777218.0, R.f32(0.1), 0.0, -0.0, NAN]),
    "d": ("DOUBLE", KD),
}
TYPE_N = 300


def type_table():
    """row r: the VARCHAR key by r mod 3 (NULL for 2), each typed key walks its edge list every third row and
    is NULL in one row of ten"""
    cols = [V.Col("id", "BIGINT", range(TYPE_N))]
    for j, (name, (t, edges)) in enumerate(TYPE_EDGES.items()):
        cols.append(V.Col(name, t, [edges[(r // 3 + r // 40) % len(edges)] for r in range(TYPE_N)],
                          [(r + j) % 10 != 7 for r in range(TYPE_N)]))
    return V.Table("t", cols)


def s_of(r):
    return ["x", "yy", None][r % 3]


def decoder(col):
    if col.sqltype in ("DATE", "TIMESTAMP"):
        return lambda text, raw: int.from_bytes(raw(), "little", signed=True)
    if col.kind in ("f64", "f32"):
        return lambda text, raw: _float(raw())
    if col.kind == "dec":
        return lambda text, raw: int(text.replace(".", ""))
    if col.kind == "bool":
        return lambda text, raw: {"true": True, "false": False}[text]
    return lambda text, raw: int(text)


@pytest.fixture(scope="module")
def typed(mbx):
    c = connect(mbx)
    t = type_table()
    load(mbx, c, t, "t", list(range(TYPE_N)), list(t.cols))
    q(c, "CREATE TABLE tk AS SELECT CASE WHEN id % 3 = 0 THEN 'x' WHEN id % 3 = 1 THEN 'yy' END AS s, id AS v, " +
         ", ".join(TYPE_EDGES) + " FROM t")
    yield c, t
    c.close()


@pytest.mark.parametrize("name", list(TYPE_EDGES))
def test_key_type_beside_a_varchar_key(typed, name):
    c, t = typed
    col = t.cols[name]
    rows = [(s_of(r), col.get(r), r) for r in range(TYPE_N)]
    want = {k: ints(v) for k, v in group(rows, 2).items()}
    # every edge value is a group of its own beside each string (one zero and one NaN for the floats), and NULL
    distinct = {M.key_of(v) for v in TYPE_EDGES[name][1]}
    assert {k[1] for k in want} == distinct | {None}, name
    assert all((s, v) in want for s in ("x", "yy", None) for v in distinct), name
    check(c, f"SELECT s, {name}, {INTS} FROM tk GROUP BY s, {name}", 2, want, [None, decoder(col)])
    check(c, f"SELECT {name}, s, {INTS} FROM tk GROUP BY {name}, s", 2,
          {(k[1], k[0]): v for k, v in want.items()}, [decoder(col), None])


def test_ubigint_above_2_63_and_equal_low_words_stay_apart(typed):
    c, t = typed
    for name, vals in (("u64", [I64, U64 - 1, I64 - 1]), ("h", [1, U64 + 1, -1, U64 - 1]), ("m", [1, U64 + 1, -1, U64 - 1])):
        got = result(c, f"SELECT s, {name}, COUNT(*) FROM tk WHERE s = 'x' GROUP BY s, {name}", 2, [None, decoder(t.cols[name])])
        on_hash_path(c)
        for v in vals:
            n = sum(1 for r in range(TYPE_N) if s_of(r) == "x" and t.cols[name].get(r) == v)
            assert n > 0 and got[("x", v)] == [str(n)], (name, v)


def test_eight_keys_answer_nine_and_interval_are_refused(mbx, typed):
    c, t = typed
    names = ["b", "i8", "u16", "u64", "h", "f", "d"]
    rows = [(s_of(r),) + tuple(t.cols[k].get(r) for k in names) + (r,) for r in range(TYPE_N)]
    want = {k: ints(v) for k, v in group(rows, 8).items()}
    assert len(want) > 100
    keys = ", ".join(["s"] + names)
    check(c, f"SELECT {keys}, {INTS} FROM tk GROUP BY {keys}", 8, want, [None] + [decoder(t.cols[k]) for k in names])
    r = c.query(f"SELECT {keys}, i16, COUNT(*) FROM tk GROUP BY {keys}, i16")
    assert isinstance(r, mbx.Err) and "GROUP BY with more than 8 keys" in r.error.message, r
    check(c, f"SELECT s, b, {INTS} FROM tk GROUP BY s, b", 2, {k: ints(v) for k, v in group([(a[0], a[1], a[-1]) for a in rows], 2).items()},
          [None, decoder(t.cols["b"])])
    q(c, "CREATE TABLE iv (s VARCHAR, i INTERVAL, v BIGINT)")
    q(c, "INSERT INTO iv VALUES ('a', INTERVAL 1 day, 1), ('a', INTERVAL 2 day, 2), ('b', INTERVAL 1 day, 3), (NULL, NULL, 4)")
    r = c.query("SELECT s, i, COUNT(*) FROM iv GROUP BY s, i")
    assert isinstance(r, mbx.Err) and "GROUP BY on INTERVAL keys is not supported on device" in r.error.message, r
    check(c, f"SELECT s, {INTS} FROM iv GROUP BY s", 1, {("a",): ints([1, 2]), ("b",): ints([3]), (None,): ints([4])})


# ---- d. many groups ----------------------------------------------------------------------------------------
BIG_N = 70_001
SHAPES = {"sa": BIG_N, "s1024": 1024, "s1025": 1025, "so": 1, "st": 2}


def name_of(k):
    """distinct strings of mixed lengths, many sharing long prefixes"""
    return f"group-{k % 97}-" + "pad" * (k % 5) + f"-{k}"


def big_row(r):
    w = (r * 2654435761) % 2 ** 32 - 2 ** 31  # every int32; the HUGEINT argument is w * 10^18
    d = None if r % 13 == 5 else (-1.0 if r % 3 == 1 else 1.0) * (1 + (r * 37 % 1000) / 1000) * 10.0 ** ((r * 13) % 16 - 3)
    return (name_of(r), name_of(r % 1024), name_of(r % 1025), "the only key", ["left", "right"][r % 2],
            None if r % 7 == 2 else (r * 31) % 100_003 - 50_000, w, d)


@pytest.fixture(scope="module")
def big(mbx):
    """the one 70 001-row VARCHAR table, filled once"""
    c = connect(mbx)
    rows = [big_row(r) for r in range(BIG_N)]
    fill(c, "big", "sa VARCHAR, s1024 VARCHAR, s1025 VARCHAR, so VARCHAR, st VARCHAR, v BIGINT, w BIGINT, d DOUBLE", rows)
    yield c, rows
    c.close()


def check_double_block(cells, raw, j, vals, where):
    """SUM(d), AVG(d), MIN(d), MAX(d) at raw result columns j .. j + 3"""
    st = M.stats(vals, "f64")
    if st.count == 0:
        assert cells[j:j + 4] == [None] * 4, where
        return
    assert st.abs_sum < 1e300
    tol = Fraction(st.abs_sum) / 10 ** 9
    s, a = _float(raw(j)), _float(raw(j + 1))
    assert math.isfinite(s) and abs(Fraction(s) - Fraction(st.sum)) <= tol, where + ("sum", s, st.sum)
    assert math.isfinite(a) and abs(Fraction(a) - Fraction(st.sum) / st.count) <= tol / st.count, where + ("avg", a)
    for o, want in ((2, st.min), (3, st.max)):
        b = raw(j + o)
        assert len(b) == 8 and R.bits(_float(b)) in want, where + (o, b, want)


@pytest.mark.parametrize("shape", list(SHAPES))
def test_many_groups(big, shape):
    c, rows = big
    col = list(SHAPES).index(shape)
    by = {}
    for r in rows:
        by.setdefault(r[col], []).append(r)
    assert len(by) == SHAPES[shape]
    # a NULL-able BIGINT: exact
    ks = check(c, f"SELECT {shape}, {INTS} FROM big GROUP BY {shape}", 1, {(k,): ints([r[5] for r in g]) for k, g in by.items()})
    assert "group_reduce" in ks and "group_direct" not in ks, ks  # (the LDS reduction declines NULL-able values)
    # a BIGINT without NULLs: the second stage reduces up to 1024 groups in LDS, more through group_reduce
    ks = check(c, f"SELECT {shape}, COUNT(*), COUNT(w), SUM(w), MIN(w), MAX(w) FROM big GROUP BY {shape}", 1,
               {(k,): ints([r[6] for r in g]) for k, g in by.items()})
    if SHAPES[shape] <= 1024:
        assert "group_direct" in ks and "group_reduce" not in ks, (shape, ks)
    else:
        assert "group_reduce" in ks and "group_direct" not in ks, (shape, ks)
    # a HUGEINT argument (exact) and a DOUBLE one
    hx = "CAST(w AS HUGEINT) * 1000000000000000000"
    sql = f"SELECT {shape}, SUM({hx}), MIN({hx}), MAX({hx}), SUM(d), AVG(d), MIN(d), MAX(d) FROM big GROUP BY {shape}"
    res = c.query_raw(sql)
    try:
        on_hash_path(c, sql)
        text, nulls = res.cells()
        seen = set()
        for i in range(res.row_count()):
            assert not nulls[i][0] and text[i][0] in by and text[i][0] not in seen, (sql, text[i][0])
            seen.add(text[i][0])
            g = by[text[i][0]]
            h = [r[6] * 10 ** 18 for r in g]
            assert text[i][1:4] == [str(sum(h)), str(min(h)), str(max(h))] and not any(nulls[i][1:4]), (shape, text[i][:4])
            cells = [None if n else t for t, n in zip(text[i], nulls[i])]
            check_double_block(cells, lambda j, i=i: res.raw(j, i), 4, [r[7] for r in g], (shape, text[i][0]))
        assert seen == set(by)
    finally:
        res.close()


# ---- e. the table's capacity steps ----------------------------------------------------------------------------
@pytest.mark.parametrize("n", [512, 513, 1024, 1025])
def test_capacity_steps_all_keys_distinct(mbx, n):
    """BIGINT keys i * 1000003: a range too wide for every other path below 2^16 rows.  The table has 1024
    entries up to 512 rows, 2048 at 513 and 1024, 4096 at 1025; 1024 groups are the last the LDS stage takes"""
    c = connect(mbx)
    q(c, f"CREATE TABLE e AS SELECT i * 1000003 AS k, i - 300 AS v FROM range({n}) tbl(i)")
    ks = check(c, f"SELECT k, {INTS} FROM e GROUP BY k", 1, {(i * 1000003,): ints([i - 300]) for i in range(n)}, [decoder_int])
    assert ("group_reduce" in ks) == (n > 1024) and ("group_direct" in ks) == (n <= 1024), (n, ks)
    c.close()


# ---- f. crafted chains ------------------------------------------------------------------------------------------
def chain_rows(kind):
    """250 keys whose home is the last slot of the 1024-entry table, each twice with its twin 250 rows away"""
    keys = H.cluster(1024, 1023, 250, kind)
    return [(k, i) for i, k in enumerate(keys + keys)]


def tag_pair_rows(kind):
    """120 pairs of keys with equal tag and home slot, then 130 of those keys again: 370 rows, 240 groups"""
    pairs = H.tag_pairs(1024, 120, kind)
    keys = [k for p in pairs for k in p]
    return [(k, i) for i, k in enumerate(keys + keys[:130])]


@pytest.mark.parametrize("kind", ["int", "str"])
@pytest.mark.parametrize("rows_of", [chain_rows, tag_pair_rows], ids=["chain", "tag_pairs"])
def test_crafted_collisions(mbx, kind, rows_of):
    rows = rows_of(kind)
    assert len(rows) <= 512  # a 1024-entry table
    want = {k: ints(v) for k, v in group(rows, 1).items()}
    assert len(want) == (250 if rows_of is chain_rows else 240)
    assert sorted(int(w[0]) for w in want.values()) == ([2] * 250 if rows_of is chain_rows else [1] * 110 + [2] * 130)
    c = connect(mbx)
    if kind == "int":
        t = V.Table("cr", [V.Col("k", "BIGINT", [r[0] for r in rows]), V.Col("v", "BIGINT", [r[1] for r in rows])])
        load(mbx, c, t, "cr", list(range(len(rows))), ["k", "v"])
    else:
        fill(c, "cr", "k VARCHAR, v BIGINT", rows)
    check(c, f"SELECT k, {INTS} FROM cr GROUP BY k", 1, want, [decoder_int if kind == "int" else None])
    c.close()


# ---- g. where the keys come from -----------------------------------------------------------------------------------
def test_keys_from_union_join_subquery_case_and_append(mbx):
    c = connect(mbx)
    names = [None, "", "u", "union", "é" * 9, "long" * 10, "long" * 10 + "!", "z"]
    ua = [(names[(k * 5) % 8], k) for k in range(130)]
    ub = [(names[(k * 3 + 1) % 8] if k % 9 else "only in b", 1000 + k) for k in range(67)]
    fill(c, "ua", "s VARCHAR, v BIGINT", ua)
    fill(c, "ub", "s VARCHAR, v BIGINT", ub)
    # the second branch's offsets are rebased behind the first's
    check(c, f"SELECT s, {INTS} FROM (SELECT s, v FROM ua UNION ALL SELECT s, v FROM ub) u GROUP BY s", 1,
          {k: ints(v) for k, v in group(ua + ub, 1).items()})
    check(c, f"SELECT s, {INTS} FROM (SELECT s, v FROM ub UNION ALL SELECT s, v FROM ua UNION ALL SELECT s, v FROM ub) u GROUP BY s", 1,
          {k: ints(v) for k, v in group(ub + ua + ub, 1).items()})
    # a subquery with a filter of its own
    check(c, f"SELECT s, {INTS} FROM (SELECT s, v FROM ua WHERE v % 4 <> 1) u GROUP BY s", 1,
          {k: ints(v) for k, v in group([r for r in ua if r[1] % 4 != 1], 1).items()})
    # a CASE that mixes pooled constants with the column's strings
    def case(s, v):
        return "even" if v % 2 == 0 else "" if v % 3 == 0 else s
    check(c, f"SELECT CASE WHEN v % 2 = 0 THEN 'even' WHEN v % 3 = 0 THEN '' ELSE s END AS g, {INTS} FROM ua GROUP BY g", 1,
          {k: ints(v) for k, v in group([(case(s, v), v) for s, v in ua], 1).items()})
    # a join's gathered right-hand VARCHAR column, more than 1024 groups
    dim = [(k, name_of(k % 1300)) for k in range(1500)]  # 200 names under two keys each
    fact = [((i * 7) % 1600, i) for i in range(4000)]    # keys 1500 .. 1599 find no partner
    fill(c, "dim", "k BIGINT, name VARCHAR", dim)
    fill(c, "fact", "k BIGINT, v BIGINT", fact)
    name = dict(dim)
    joined = [(name[k], v) for k, v in fact if k < 1500]
    want = {k: ints(v) for k, v in group(joined, 1).items()}
    assert len(want) == 1300
    ks = check(c, f"SELECT dim.name, COUNT(*), COUNT(fact.v), SUM(fact.v), MIN(fact.v), MAX(fact.v) FROM fact JOIN dim ON fact.k = dim.k "
                  "GROUP BY dim.name", 1, want)
    assert "join_gather" in ks, ks
    # a table grown by a second append after its first GROUP BY
    more = [(names[(k * 3) % 8] if k % 5 else "appended", 5000 + k) for k in range(90)]
    ap = c.create_appender("main", "ua").value
    for s, v in more:
        ap.begin_row()
        ap.append_null() if s is None else ap.append_varchar(s)
        ap.append_int(v)
        ap.end_row()
    ap.flush()
    ap.close()
    check(c, f"SELECT s, {INTS} FROM ua GROUP BY s", 1, {k: ints(v) for k, v in group(ua + more, 1).items()})
    c.close()


def test_no_rows_and_one_row(mbx):
    c = connect(mbx)
    q(c, "CREATE TABLE z (s VARCHAR, v BIGINT)")
    check(c, f"SELECT s, {INTS} FROM z GROUP BY s", 1, {})
    check(c, "SELECT DISTINCT s FROM z", 1, {})
    fill(c, "o", "s VARCHAR, v BIGINT", [("lonely", -7)])
    check(c, f"SELECT s, {INTS} FROM o GROUP BY s", 1, {("lonely",): ints([-7])})
    check(c, f"SELECT s, {INTS} FROM o WHERE v > 0 GROUP BY s", 1, {})
    fill(c, "n1", "s VARCHAR, v BIGINT", [(None, None)])
    check(c, f"SELECT s, {INTS} FROM n1 GROUP BY s", 1, {(None,): ints([None])})
    # columns without a single character: only NULLs, only '', both
    fill(c, "n3", "s VARCHAR, v BIGINT", [(None, 1), (None, 2), (None, None)])
    check(c, f"SELECT s, {INTS} FROM n3 GROUP BY s", 1, {(None,): ints([1, 2, None])})
    fill(c, "blank", "s VARCHAR, v BIGINT", [("", 1), (None, 2), ("", 3), ("", None), (None, 5)])
    check(c, f"SELECT s, {INTS} FROM blank GROUP BY s", 1, {("",): ints([1, 3, None]), (None,): ints([2, 5])})
    check(c, "SELECT DISTINCT s FROM blank", 1, {("",): [], (None,): []})
    assert q(c, "SELECT COUNT(DISTINCT s), COUNT(s) FROM blank").rows == [["1", "3"]]
    on_hash_path(c)
    c.close()


# ---- h. shards -----------------------------------------------------------------------------------------------------
SHARD_ROWS = 256


def check_split(c, table, rows):
    """the table's first SHARD_ROWS rows are one part, the rest the other: each shard's partial of a filtered
    count against the model over its rows (v: the last column)"""
    q(c, f"SELECT COUNT(*), SUM(v) FROM {table} WHERE v > -1000000")
    for i, part in enumerate((rows[:SHARD_ROWS], rows[SHARD_ROWS:])):
        vs = [r[-1] for r in part if r[-1] is not None]
        p = c.shard_partial(i)
        assert p is not None and vs, (table, i)
        assert [p.value(0, 0), p.value(1, 0)] == [str(len(vs)), str(sum(vs))], (table, i, p.cells())
        p.close()


def test_two_shards_merge_by_key(mbx):
    # (a flush of the row appender goes to one part whole: flushes of a part's size split the tables)
    c = connect(mbx, gpu_devices="0,0", mbx_shard_rows=SHARD_ROWS, mbx_appender_flush_rows=SHARD_ROWS)
    assert c.shard_stats()["shards"] == 2
    rows = edge_rows()
    fill(c, "edge", "s VARCHAR, v BIGINT", rows)
    check_split(c, "edge", rows)
    a, b = {s for s, _ in rows[:SHARD_ROWS]}, {s for s, _ in rows[SHARD_ROWS:]}
    assert (a & b) - {None} and a - b and b - a and None in a | b  # groups in both parts, in one, and NULL
    check_edge_table(c)
    fill(c, "ab", "a VARCHAR, b VARCHAR, v BIGINT", pair_rows())
    check_split(c, "ab", pair_rows())
    check_pairs(c)
    m = [(name_of(r % 1025) if r % 50 else None, r - 2000) for r in range(4100)]
    fill(c, "m", "s VARCHAR, v BIGINT", m)
    check_split(c, "m", m)
    assert {s for s, _ in m[SHARD_ROWS:]} - {s for s, _ in m[:SHARD_ROWS]}  # most groups live in the second part only
    want = {k: ints(v) for k, v in group(m, 1).items()}
    assert len(want) == 1026
    check(c, f"SELECT s, {INTS} FROM m GROUP BY s", 1, want)
    assert q(c, "SELECT COUNT(DISTINCT s) FROM m").rows == [["1025"]]
    on_hash_path(c, "COUNT(DISTINCT s), sharded")
    c.close()
