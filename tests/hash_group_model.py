"""A numpy restatement of the hash GROUP BY's row hash (duckdb.mbt_amd/csrc/
group_hash.h) for the two key shapes the crafted tests need -- one BIGINT key and
one byte string of a fixed length -- and two brute-force searches over it:
cluster() finds keys that share a home slot, tag_pairs() pairs of different keys
with equal tag and equal home slot.  test_group_hash_plan.py ties the restatement
to the header (the harness's `hashes` output); the searches assert that they
found what was asked for, so that a later change of the hash makes the crafted
tests fail instead of passing without a single collision.

The searches run over i * 1000003 for i < 2^22, and for strings over the
zero-padded 8-digit decimal spelling of i."""
import functools

import numpy as np

U = np.uint64
SEED, NULL_WORD, HIGH_ADD = U(0x9E3779B97F4A7C15), U(0x5BD1E9955BD1E995), U(0x632BE59BD9B4E019)
STR_SEED, STR_PRIME = U(0xCBF29CE484222325), U(0x100000001B3)
TAG_SHIFT = U(40)
SEARCH = 1 << 22
STEP = 1000003


def hmix(z):
    z = (z ^ (z >> U(30))) * U(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> U(27))) * U(0x94D049BB133111EB)
    return z ^ (z >> U(31))


def hash_bigint(keys):
    """the row hash of one BIGINT key per row (an int64 array): the value, then its sign extension"""
    k = np.asarray(keys, dtype=np.int64)
    h = hmix(SEED ^ k.view(np.uint64))
    return hmix(h ^ ((k >> 63).view(np.uint64) + HIGH_ADD))


def hash_bytes(rows):
    """the row hash of one VARCHAR key per row: a (n, length) uint8 array, every string `length` bytes"""
    b = np.asarray(rows, dtype=np.uint8)
    f = np.full(b.shape[0], STR_SEED ^ U(b.shape[1]), dtype=np.uint64)
    for j in range(b.shape[1]):
        f = (f ^ b[:, j].astype(np.uint64)) * STR_PRIME
    return hmix(SEED ^ f)


def hash_row(cells):
    """the row hash of one key row of any shape, in Python integers: None is NULL, bytes a string, a float a
    DOUBLE key, an int a fixed-width key of up to 128 bits (negative: sign-extended; UBIGINT: high word 0)"""
    m = (1 << 64) - 1

    def mix(z):
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & m
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & m
        return z ^ (z >> 31)

    h = int(SEED)
    for c in cells:
        if c is None:
            h = mix(h ^ int(NULL_WORD))
        elif isinstance(c, bytes):
            f = int(STR_SEED) ^ len(c)
            for b in c:
                f = ((f ^ b) * int(STR_PRIME)) & m
            h = mix(h ^ f)
        else:
            if isinstance(c, float):  # one zero, one NaN
                c = 0x7FF8000000000000 if c != c else 0 if c == 0 else int(np.float64(c).view(np.uint64))
            h = mix(h ^ (c & m))
            h = mix(h ^ ((((c >> 64) & m) + int(HIGH_ADD)) & m))
    return h


# the fixed list whose hashes tests/plan_harness/group_hash.cpp prints (`hashes`), in its order
HASHED_ROWS = [
    [0], [-1], [-2 ** 63], [2 ** 63 - 1], [12345 * STEP],
    [2 ** 64 + 1], [2 ** 64 - 1], [-1], [2 ** 63],  # HUGEINT words; UBIGINT 2^63 (BIGINT -1 and HUGEINT -1 hash alike)
    [1.5], [-0.0], [float(np.uint64(0xFFF8000000000001).view(np.float64))], [5e-324],
    [b""], [b"a"], [b"abc"], [b"\xff\x80\xc3\xa9"], [b"00001234"], [b"seventeen bytes!!"],
    [None],
    [b"ab", None, 7],
]


def digits(i):
    """the zero-padded 8-digit decimal spelling of each i, as a (n, 8) uint8 array"""
    i = np.asarray(i, dtype=np.int64)
    return np.stack([(i // 10 ** (7 - j)) % 10 + ord("0") for j in range(8)], axis=1).astype(np.uint8)


def _candidates(kind):
    i = np.arange(SEARCH, dtype=np.int64)
    if kind == "int":
        return i * STEP, hash_bigint(i * STEP)
    assert kind == "str", kind
    return i, hash_bytes(digits(i))


def _keys(kind, v):
    return [int(x) for x in v] if kind == "int" else ["%08d" % int(x) for x in v]


@functools.lru_cache(maxsize=None)
def _home_hits(cap, slot, kind):
    v, h = _candidates(kind)
    return v[(h & U(cap - 1)) == U(slot)]


def cluster(cap, slot, count, kind="int"):
    """`count` keys whose home slot in a table of `cap` entries is `slot`"""
    hit = _home_hits(cap, slot, kind)
    assert len(hit) >= count, f"only {len(hit)} {kind} keys with home slot {slot} of {cap}: has the hash changed?"
    return _keys(kind, hit[:count])


@functools.lru_cache(maxsize=None)
def _all_pairs(cap, kind):
    v, h = _candidates(kind)
    both = ((h >> TAG_SHIFT) << TAG_SHIFT) | (h & U(cap - 1))
    order = np.argsort(both, kind="stable")
    s = both[order]
    same = np.nonzero(s[1:] == s[:-1])[0]
    pairs, last = [], -2
    for j in same:  # a run of three gives one pair
        if j > last + 1:
            pairs.append((v[order[j]], v[order[j + 1]]))
            last = j
    return pairs


def tag_pairs(cap, count, kind="int"):
    """`count` pairs (a, b) of different keys with the same tag and the same home slot in a table of `cap`
    entries; no key is in two pairs"""
    pairs = _all_pairs(cap, kind)
    assert len(pairs) >= count, f"only {len(pairs)} {kind} tag pairs at capacity {cap}: has the hash changed?"
    a, b = _keys(kind, [p[0] for p in pairs[:count]]), _keys(kind, [p[1] for p in pairs[:count]])
    assert all(x != y for x, y in zip(a, b))
    return list(zip(a, b))
