"""The rounds of MIN / MAX over VARCHAR (duckdb.mbt_amd/csrc/str_minmax.h),
checked on the host: a stand-alone C++ program
(tests/plan_harness/str_minmax.cpp, its own main) includes the header and is
built with the host compiler under AddressSanitizer and UBSan.  It runs the
rounds the kernels run -- chunk keys, the length tie, the row tie, offered to one
64-bit word per kind -- in one thread over string sets and compares the winner
rows with a direct StrCompare scan: lengths 0 to 25 around the 8-byte chunk
borders, ties on the first 8 and 16 bytes, trailing NUL bytes, bytes >= 0x80
against ASCII, eight 0xFF bytes and '' only (keys that equal a word's initial
value), equal strings (the lowest row wins), no non-NULL row (no winner), and
200 seeded random sets over a 3-letter alphabet."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_str_minmax_plan_host_program(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "str_minmax")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=undefined", "-I", os.path.join(ROOT, "duckdb.mbt_amd", "csrc"),
           os.path.join(ROOT, "tests", "plan_harness", "str_minmax.cpp"), "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True)
    assert b.returncode == 0, b.stdout + b.stderr
    p = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "str minmax plan: ok" in p.stdout
