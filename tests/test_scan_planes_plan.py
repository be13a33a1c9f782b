"""The bit-plane scan code images (duckdb.mbt_amd/csrc/scan_planes.h), checked
on the host: a stand-alone C++ program
(tests/plan_harness/scan_planes_plan.cpp, its own main) includes the header and
is built with the host compiler under AddressSanitizer and UBSan.  It checks
which zone maps get planes (codes of 1 to 8 bits); the layout for every b (row
-> word, bit and piece offset against the design's formula and against the
segment view, buffer bytes for a capacity, reported bytes, the last-word mask,
codes read back from an image); the plan for every b <= 8, every largest code
and every clo <= chi against the definition (the compares over the planned
planes alone give clo <= c <= chi for every code, and no skipped plane's bit
changes any code's answer); and the compare, sum, min and max primitives
against a per-row loop over words with every code of every b at every bit
position in a word of zeros, largest codes or seeded random codes, random
words, and last-word masks.  In that last part the bounds are every value for
b <= 5 and a sample for b = 6..8 (the three lowest and highest, powers of two,
powers of two less one, multiples of 23): two drawn from them and the code
itself per word, and every pair of them over random words; the plan check
before it runs every bound pair over every code."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_scan_planes_plan_host_program(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "scan_planes_plan")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=undefined", "-I", os.path.join(ROOT, "duckdb.mbt_amd", "csrc"),
           os.path.join(ROOT, "tests", "plan_harness", "scan_planes_plan.cpp"), "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True)
    assert b.returncode == 0, b.stdout + b.stderr
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "scan planes plan: ok" in p.stdout
