"""The table of the hash GROUP BY (duckdb.mbt_amd/csrc/group_hash.h), checked on
the host: a stand-alone C++ program (tests/plan_harness/group_hash.cpp, its own
main) includes the header and is built with the host compiler under
AddressSanitizer and UBSan.  Through the header's own insert walk, with a
single-threaded claim, it checks the capacity rule, chains of >= 250 keys that
share the last slot of a 1024-entry table and wrap to slot 0, >= 100 pairs of
different keys with equal tag and equal home slot (BIGINT keys and 8-byte
strings, found by brute force against the header's hash), the equality and hash
of fixed-width, DOUBLE, FLOAT and string keys, '' beside NULL, a lost
compare-and-swap, and the bounded-walk verdict on a table without an empty slot.

tests/hash_group_model.py restates the hash in numpy for the GPU suite's crafted
key sets; here it is tied to the header (the program's `hashes` output) and its
two searches are held to their floors."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import hash_group_model as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("group_hash") / "group_hash")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=undefined", "-I", os.path.join(ROOT, "duckdb.mbt_amd", "csrc"),
           os.path.join(ROOT, "tests", "plan_harness", "group_hash.cpp"), "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True)
    assert b.returncode == 0, b.stdout + b.stderr
    return exe


def test_group_hash_host_program(harness):
    p = subprocess.run([harness], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "group hash: ok" in p.stdout


def test_model_equals_header(harness):
    p = subprocess.run([harness, "hashes"], capture_output=True, text=True, timeout=60)
    assert p.returncode == 0, p.stdout + p.stderr
    got = [int(line, 16) for line in p.stdout.split()]
    assert len(got) == len(H.HASHED_ROWS)
    for row, h in zip(H.HASHED_ROWS, got):
        assert H.hash_row(row) == h, (row, hex(H.hash_row(row)), hex(h))
    # the vectorised forms against the scalar one, on the list's BIGINT keys and 8-byte string and beyond
    ints = [r[0] for r in H.HASHED_ROWS[:5]] + [7 * H.STEP, -7 * H.STEP]
    assert [int(x) for x in H.hash_bigint(np.array(ints, dtype=np.int64))] == [H.hash_row([k]) for k in ints]
    strs = [b"00001234", b"04194303", b"\xff\x80\xc3\xa9zzzz"]
    rows = np.frombuffer(b"".join(strs), dtype=np.uint8).reshape(len(strs), 8)
    assert [int(x) for x in H.hash_bytes(rows)] == [H.hash_row([s]) for s in strs]
    assert H.hash_row([b"00001234"]) == got[17]
    assert bytes(H.digits([1234, 4194303])[1]) == b"04194303" and bytes(H.digits([1234])[0]) == b"00001234"


@pytest.mark.parametrize("kind", ["int", "str"])
def test_searches_find_their_collisions(kind):
    cap = 1024
    one = (lambda k: [k]) if kind == "int" else (lambda k: [k.encode()])
    keys = H.cluster(cap, cap - 1, 250, kind)
    assert len(keys) == len(set(keys)) == 250
    assert all(H.hash_row(one(k)) & (cap - 1) == cap - 1 for k in keys)
    pairs = H.tag_pairs(cap, 120, kind)
    assert len(pairs) == 120 and len({k for p in pairs for k in p}) == 240
    for a, b in pairs:
        ha, hb = H.hash_row(one(a)), H.hash_row(one(b))
        assert a != b and ha >> 40 == hb >> 40 and ha & (cap - 1) == hb & (cap - 1), (a, b)
    # more than the floors the crafted tests ask for: the range holds thousands of keys per slot, hundreds of pairs
    assert len(H.cluster(cap, cap - 1, 1000, kind)) == 1000 and len(H.tag_pairs(cap, 300, kind)) == 300
    with pytest.raises(AssertionError, match="has the hash changed"):
        H.cluster(cap, cap - 1, 1 << 22, kind)
