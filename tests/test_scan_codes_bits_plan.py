"""The bit-packed scan code images (duckdb.mbt_amd/csrc/scan_codes.h), checked
on the host: a stand-alone C++ program
(tests/plan_harness/scan_codes_bits_plan.cpp, its own main) includes the header
and is built with the host compiler under AddressSanitizer and UBSan.  It
checks the fields per word at ranges 1, 2, 3, 4, 5, 8, 9, 16, 17, 32, 33, 64,
65, 128, 129, 256, 257, 1024, 1025, 65536 and 65537 for both physical types
(and every range up to 65536 against the rule "the most fields that hold the
largest code"), with and without bit fields; the layout (row -> word and shift,
words for n rows, rows per piece, reported bytes, zero padding) for every field
count; which compare the plan picks; and every word-parallel compare against a
per-field loop: for fields of up to 6 bits every largest code and every
clo <= chi, for 8, 10 and 16 bits a sample, over words with each field position
holding every code while the others hold 0, the largest code or seeded random
codes, plus random words.  Mask, popcount and the even / odd lane sum must all
equal the loop's."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_scan_codes_bits_plan_host_program(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "scan_codes_bits_plan")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=undefined", "-I", os.path.join(ROOT, "duckdb.mbt_amd", "csrc"),
           os.path.join(ROOT, "tests", "plan_harness", "scan_codes_bits_plan.cpp"), "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True)
    assert b.returncode == 0, b.stdout + b.stderr
    p = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "scan codes bits plan: ok" in p.stdout
