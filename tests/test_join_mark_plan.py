"""The mark join's decision table (duckdb.mbt_amd/csrc/join_mark_plan.h),
checked on the host: a stand-alone C++ program
(tests/plan_harness/join_mark_plan.cpp, its own main) includes the header and is
built with the host compiler under AddressSanitizer and UBSan.  It checks the
cell function of x IN (subquery) on all 16 combinations of {key found, probe
key valid, set empty, set holds a NULL} against a truth table written out in
the program, and the host plan: the constant FALSE for an empty set, a validity
bitmap only for a NULL-able probe key or a set with a NULL, no table for a set
of NULLs only."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_join_mark_plan_host_program(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "join_mark_plan")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=undefined", "-I", os.path.join(ROOT, "duckdb.mbt_amd", "csrc"),
           os.path.join(ROOT, "tests", "plan_harness", "join_mark_plan.cpp"), "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True)
    assert b.returncode == 0, b.stdout + b.stderr
    p = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "join mark plan: ok" in p.stdout
