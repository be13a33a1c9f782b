"""The window stage's host header (duckdb.mbt_amd/csrc/window_plan.h), checked on
the host: a stand-alone C++ program (tests/plan_harness/window_plan.cpp, its own
main) includes the header and is built with the host compiler under
AddressSanitizer and UBSan.  It checks the frame-resolution table on every
(function, ORDER BY, frame) combination, the grouping of calls by
specification, and the segmented operator (fa, a) (+) (fb, b) =
(fa | fb, fb ? b : merge(a, b)) of every state kind.

Associativity: this test writes 1000 random elements, about a tenth of them
flagged as segment starts and about a tenth NULL, and beside each element the
running value of every state kind, computed here with Python integers: int128
sums of values at +-(2^63 - 1), so the high word carries in both directions;
double sums of integers below 2^40, exact in any order; min / max of negatives
as order-preserving keys; 128-bit min / max; the segment's first position.  The
program folds the elements four ways (left fold, right-nested fold, tiles of 7
and of 256 with a carry scan) and each must give those running values element
by element."""
import os
import random
import shutil
import struct
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIG = 2 ** 63 - 1
M64 = 2 ** 64 - 1


def _u64(x):
    return x & M64


def _elements(rng, n):
    lines, carried = [], False
    cnt = total = 0
    fsum = 0
    mn = mx = mn8 = mx8 = None
    pos = 0
    for i in range(n):
        flag = 1 if i == 0 or rng.random() < 0.1 else 0
        valid = 0 if rng.random() < 0.1 else 1
        v = rng.choice([BIG, BIG, -BIG, -BIG, rng.randint(-BIG, BIG), rng.randint(-1000, -1)])
        d = rng.randint(-2 ** 40, 2 ** 40)
        h = v * rng.choice([3, 5, 2 ** 40])  # beyond 64 bits, either sign
        if flag:
            cnt = total = fsum = 0
            mn = mx = mn8 = mx8 = None
            pos = i
        if valid:
            cnt += 1
            total += v
            fsum += d
            mn, mx = (v if mn is None else min(mn, v)), (v if mx is None else max(mx, v))
            mn8, mx8 = (h if mn8 is None else min(mn8, h)), (h if mx8 is None else max(mx8, h))
        carried |= abs(total) > 2 ** 64
        fbits = struct.unpack("<Q", struct.pack("<d", float(fsum)))[0]
        key = lambda x: _u64(x) ^ 2 ** 63
        mn64, mx64 = (M64, 0) if mn is None else (key(mn), key(mx))
        mn128 = (M64, BIG) if mn8 is None else (_u64(mn8), mn8 >> 64)
        mx128 = (0, -BIG - 1) if mx8 is None else (_u64(mx8), mx8 >> 64)
        dbits = struct.unpack("<Q", struct.pack("<d", float(d)))[0]
        lines.append(f"{flag} {valid} {v} {dbits} {_u64(h)} {h >> 64} {cnt} {_u64(total)} {total >> 64} {fbits} "
                     f"{mn64} {mx64} {mn128[0]} {mn128[1]} {mx128[0]} {mx128[1]} {pos}\n")
    return lines, carried


def test_window_plan_host_program(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "window_plan")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=undefined", "-I", os.path.join(ROOT, "duckdb.mbt_amd", "csrc"),
           os.path.join(ROOT, "tests", "plan_harness", "window_plan.cpp"), "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True)
    assert b.returncode == 0, b.stdout + b.stderr

    rng = random.Random(20261021)
    lines, carried = _elements(rng, 1000)
    assert carried  # a running sum went past 2^64: the high words are in play
    flagged = sum(ln.startswith("1 ") for ln in lines)
    assert 60 < flagged < 150
    path = tmp_path / "elements.txt"
    path.write_text(f"{len(lines)}\n" + "".join(lines))

    p = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "window plan: ok" in p.stdout
