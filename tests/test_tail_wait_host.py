"""The result tail's wait (duckdb.mbt_amd/csrc/tail_wait.h), checked on the host:
a stand-alone C++ program (tests/plan_harness/tail_wait.cpp, its own main)
instantiates the very template the executor does, with a writer thread in the
kernel's place, and is built with the host compiler once under AddressSanitizer
and UBSan and once under ThreadSanitizer.  It checks the hand-over's ordering
over 100,000 tickets with changing cells, that a ticket one below or one above
the wanted one is never taken, that an expired budget blocks exactly once and a
blocking wait that did not bring the ticket yields no row, that a budget of 0
never spins, that the counters add up, and the ledger of profile event pairs: no
pair reissued while a pending statement holds it, settled in statement order."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("sanitize", ["address,undefined", "thread"])
def test_tail_wait_host_program(tmp_path, sanitize):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "tail_wait")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-pthread", "-fsanitize=" + sanitize,
           "-fno-sanitize-recover=undefined", "-I", os.path.join(ROOT, "duckdb.mbt_amd", "csrc"),
           os.path.join(ROOT, "tests", "plan_harness", "tail_wait.cpp"), "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True)
    assert b.returncode == 0, b.stdout + b.stderr
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "tail wait: ok (100000 handovers)" in p.stdout
