"""The one definition of an aggregate's output cell (duckdb.mbt_amd/csrc/emit_cell.h),
checked on the host: a stand-alone C++ program (tests/plan_harness/emit_cell.cpp,
its own main) includes the header the kernels compile and is built with the host
compiler under AddressSanitizer and UBSan.  Every kind (COUNT(*), COUNT, SUM, MIN,
MAX, AVG) at count 0, 1 and more, sums at +-2^63, +-2^64 and +-(2^103 - 1), bases
INT64_MIN, 0 and INT64_MAX - 255 and avg_scale 0, 2 and 18, against __int128
arithmetic written out in the program; the int128 -> double at the 53-bit
boundaries (2^53 + 1, 2^64 + 2^11 +- 1, ties) against doubles that are known and a
rounding done by hand; store_phys for every physical type; and the histogram's host
answer, fold -> values -> cells -> ResultBufferLayout offsets, into a byte buffer
for 1 and 6 columns of which no byte outside the cells and validity words may
change."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_emit_cell_host_program(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "emit_cell")
    cmd = [cxx, "-std=c++17", "-O2", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=undefined", "-I", os.path.join(ROOT, "duckdb.mbt_amd", "csrc"),
           os.path.join(ROOT, "tests", "plan_harness", "emit_cell.cpp"), "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True)
    assert b.returncode == 0, b.stdout + b.stderr
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "emit cell: ok" in p.stdout
