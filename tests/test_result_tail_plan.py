"""The result tail's host header (duckdb.mbt_amd/csrc/result_tail.h), checked on
the host: a stand-alone C++ program (tests/plan_harness/result_tail.cpp, its own
main) includes the header and is built with the host compiler under
AddressSanitizer and UBSan.  It checks that the layout function gives, byte for
byte, the offsets ToHost computed in place before the header existed (1, 2, 15
and 16 columns of 1-, 4-, 8- and 16-byte cells, with and without validity), and
that the decision function refuses every statement shape that must not take the
tail, at the column-count boundary and at the mapped buffer's size."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_result_tail_plan_host_program(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "result_tail_plan")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=undefined", "-I", os.path.join(ROOT, "duckdb.mbt_amd", "csrc"),
           os.path.join(ROOT, "tests", "plan_harness", "result_tail.cpp"), "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True)
    assert b.returncode == 0, b.stdout + b.stderr
    p = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "result tail plan: ok" in p.stdout
