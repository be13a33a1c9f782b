"""The hash table of the inner equi-join (duckdb.mbt_amd/csrc/join_plan.h),
checked on the host: a stand-alone C++ program (tests/plan_harness/join_plan.cpp,
its own main) includes the header and is built with the host compiler under
AddressSanitizer and UBSan.  Through the header's own insert and lookup it
checks key sets whose probe sequences collide (found by brute force against the
header's hash) and wrap past the end of the table, keys 0, -1, INT64_MIN,
INT64_MAX and the multiples of 2^32, capacities 1, 2 and the power of two just
above 2n, a lookup of an absent key that walks a full cluster and stops at the
empty slot behind it, and the bounded-walk verdict of insert and lookup on a
table without an empty slot."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_join_plan_host_program(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "join_plan")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=undefined", "-I", os.path.join(ROOT, "duckdb.mbt_amd", "csrc"),
           os.path.join(ROOT, "tests", "plan_harness", "join_plan.cpp"), "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True)
    assert b.returncode == 0, b.stdout + b.stderr
    p = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "join plan: ok" in p.stdout
