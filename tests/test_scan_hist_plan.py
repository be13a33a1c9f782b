"""The code histogram of a plane-image column (duckdb.mbt_amd/csrc/scan_hist.h),
checked on the host: a stand-alone C++ program
(tests/plan_harness/scan_hist_plan.cpp, its own main) includes the header and
is built with the host compiler under AddressSanitizer and UBSan.  For every b
in 1..8, every largest code and every clo <= chi it compares the fold of the
counters (the functions the kernel runs) with a loop over the rows they were
counted from: no row, one code only, every code once, seeded random codes, and
columns of 2^40 - 1 rows (kept as runs) in one code and spread over all; each
time the count, the code sum, the smallest and largest code, and the int128 SUM,
MIN and MAX with the base at INT64_MIN, INT64_MAX - 255 and 0.  A second part
goes through PlanScanPlanes: value bounds inside, at and outside the zone map
on both sides, against a loop over the values."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_scan_hist_plan_host_program(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "scan_hist_plan")
    cmd = [cxx, "-std=c++17", "-O2", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=undefined", "-I", os.path.join(ROOT, "duckdb.mbt_amd", "csrc"),
           os.path.join(ROOT, "tests", "plan_harness", "scan_hist_plan.cpp"), "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True)
    assert b.returncode == 0, b.stdout + b.stderr
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "scan hist plan: ok" in p.stdout
