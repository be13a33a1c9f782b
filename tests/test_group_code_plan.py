"""The group-code plan of the composite-key partitioned GROUP BY
(duckdb.mbt_amd/csrc/group_code.h), checked on the host: a stand-alone C++
program (tests/plan_harness/group_code_plan.cpp, its own main) includes the
header and is built with the host compiler under AddressSanitizer and UBSan.
It checks encode -> decode round trips at every key's min, max and NULL digit
for 1-4 keys, the total of NULL-able and plain mixes, the refusals (total >=
2^62, the whole INT64 range without signed overflow) and the last-key-fastest
stride order."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_group_code_plan_host_program(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "group_code_plan")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=undefined", "-I", os.path.join(ROOT, "duckdb.mbt_amd", "csrc"),
           os.path.join(ROOT, "tests", "plan_harness", "group_code_plan.cpp"), "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True)
    assert b.returncode == 0, b.stdout + b.stderr
    p = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "group code plan: ok" in p.stdout
