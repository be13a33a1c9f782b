"""The launch plan of the direct GROUP BY (duckdb.mbt_amd/csrc/group_direct_plan.h),
checked on the host: a stand-alone C++ program
(tests/plan_harness/group_direct_plan.cpp, its own main) includes the header and
is built with the host compiler under AddressSanitizer and UBSan.  Over every
key count from 1 to 1025, 0 to 2 value columns of both widths under both key
widths, MIN/MAX on and off, all 8 masks of NULL-able columns, 0 to 3 predicate
slices, 8 value bounds from 0 to 2^63, 8 row counts from 1 to 2^30 and 256 and
64 CUs it checks that the replica count is a power of two up to 64, that the
ring offset and the LDS size are 16-aligned and under the cap of their
workgroups per CU, that trading replicas for ring space keeps the rows per
replica, that no replica's int64 sum can overflow between flushes, that the
records' size is the one the kernel writes, that the segmented form never
meets NULL-able columns or predicates, and that the layout equals the kernels'
own arithmetic.  It pins worked shapes of every form, the two shapes of
tests/test_gpu_aggregate_paths.py (f2_segmented, f2_refused) among them, and
the switches' rules ("seg" is ignored when a predicate is present)."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_group_direct_plan_host_program(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "group_direct_plan")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=undefined", "-I", os.path.join(ROOT, "duckdb.mbt_amd", "csrc"),
           os.path.join(ROOT, "tests", "plan_harness", "group_direct_plan.cpp"), "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True)
    assert b.returncode == 0, b.stdout + b.stderr
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "group direct plan: ok" in p.stdout
