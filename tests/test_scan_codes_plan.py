"""The planning of the scan code images (duckdb.mbt_amd/csrc/scan_codes.h),
checked on the host: a stand-alone C++ program
(tests/plan_harness/scan_codes_plan.cpp, its own main) includes the header and
is built with the host compiler under AddressSanitizer and UBSan.  It checks
the code width at ranges 1, 128, 129, 256, 257, 65536 and 65537 for both
physical types (INT32 never gets 2 bytes), the translation of a predicate range
against a brute-force loop over every value of small zone maps (bases at
INT64_MIN, INT64_MAX - 49, 0 and negative; bounds below, inside, at and above
the map and at the int64 extremes; the empty case), and the packed compare for
every clo <= chi below 128 and a sample below 32768."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_scan_codes_plan_host_program(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "scan_codes_plan")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=undefined", "-I", os.path.join(ROOT, "duckdb.mbt_amd", "csrc"),
           os.path.join(ROOT, "tests", "plan_harness", "scan_codes_plan.cpp"), "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True)
    assert b.returncode == 0, b.stdout + b.stderr
    p = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "scan codes plan: ok" in p.stdout
