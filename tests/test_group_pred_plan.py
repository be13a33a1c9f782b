"""The predicate plan of the partitioned GROUP BY
(duckdb.mbt_amd/csrc/group_pred_plan.h), checked on the host: a stand-alone C++
program (tests/plan_harness/group_pred_plan.cpp, its own main) includes the
header and is built with the host compiler under AddressSanitizer and UBSan.
It checks every verdict (Unfit, Empty, All, Filter), the clamp of a range to
its column's zone map, lo / span at INT64_MIN and INT64_MAX and with __int128
bounds outside int64, = predicates, ranges just inside and outside a zone-map
edge, the fourth predicate column, the operands that coincide with a key or a
value column and the bytes counted once, and for every produced entry that the
device test (uint64_t)(x - lo) <= span equals the original range over a few
hundred values around the bounds."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_group_pred_plan_host_program(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "group_pred_plan")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=undefined", "-I", os.path.join(ROOT, "duckdb.mbt_amd", "csrc"),
           os.path.join(ROOT, "tests", "plan_harness", "group_pred_plan.cpp"), "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True)
    assert b.returncode == 0, b.stdout + b.stderr
    p = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "group pred plan: ok" in p.stdout
