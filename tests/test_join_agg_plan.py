"""The fused probe-and-aggregate's host header (duckdb.mbt_amd/csrc/join_agg_plan.h),
checked on the host: a stand-alone C++ program (tests/plan_harness/join_agg_plan.cpp,
its own main) includes the header and is built with the host compiler under
AddressSanitizer and UBSan.  It checks the decision function on every reason to
decline and on the boundary max_run == limit / limit + 1, and the merge of two
partial records against constants computed in Python: low words that carry, sums
of values at +-(2^63 - 1), an empty side in both orders, min / max of negatives.
Associativity: this test writes 1000 shuffled records (a tenth of them empty) and
their merge, computed here with Python integers; the program merges them in four
orders and each must give exactly that record (the double sums are of integers
below 2^40, so they are exact in any order)."""
import os
import random
import shutil
import struct
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIG = 2 ** 63 - 1
EMPTY = (0, 0, 0, BIG, -BIG - 1, 0.0, 2 ** 64 - 1, 0)


def _record(rng):
    """(count, int sum, min, max, double sum, min_f, max_f) of a few random values; about a tenth are empty"""
    if rng.random() < 0.1:
        return None
    vals = [rng.choice([BIG, -BIG, rng.randint(-BIG, BIG), rng.randint(-1000, 1000)]) for _ in range(rng.randint(1, 5))]
    keys = [rng.getrandbits(64) for _ in vals]
    return (len(vals), sum(vals), min(vals), max(vals), float(sum(rng.randint(-2 ** 40, 2 ** 40) for _ in vals)),
            min(keys), max(keys))


def _line(rec):
    if rec is None:
        count, total, mn, mx, sf, mnf, mxf = EMPTY[0], 0, EMPTY[3], EMPTY[4], EMPTY[5], EMPTY[6], EMPTY[7]
    else:
        count, total, mn, mx, sf, mnf, mxf = rec
    lo, hi = total & (2 ** 64 - 1), total >> 64  # two's complement: the high word keeps the sign
    fbits = struct.unpack("<Q", struct.pack("<d", sf))[0]
    return f"{count} {lo} {hi} {mn} {mx} {fbits} {mnf} {mxf}\n"


def test_join_agg_plan_host_program(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "join_agg_plan")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=undefined", "-I", os.path.join(ROOT, "duckdb.mbt_amd", "csrc"),
           os.path.join(ROOT, "tests", "plan_harness", "join_agg_plan.cpp"), "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True)
    assert b.returncode == 0, b.stdout + b.stderr

    rng = random.Random(20261020)
    recs = [_record(rng) for _ in range(1000)]
    rng.shuffle(recs)
    full = [r for r in recs if r is not None]
    assert 850 < len(full) < 950
    want = (sum(r[0] for r in full), sum(r[1] for r in full), min(r[2] for r in full), max(r[3] for r in full),
            float(sum(int(r[4]) for r in full)), min(r[5] for r in full), max(r[6] for r in full))
    assert abs(want[1]) > 2 ** 64 or any(abs(r[1]) > 2 ** 64 for r in full)  # high words are in play
    path = tmp_path / "records.txt"
    path.write_text(f"{len(recs)}\n" + _line(want) + "".join(_line(r) for r in recs))

    p = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=60)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "join agg plan: ok" in p.stdout
