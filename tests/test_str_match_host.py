"""The VARCHAR matcher (duckdb.mbt_amd/csrc/str_match.h), checked on the host: a
stand-alone C++ program (tests/plan_harness/str_match.cpp, its own main)
includes the header and is built with the host compiler under AddressSanitizer
and UBSan.  It compares LikeMatch and every plan form with a recursive
definition of LIKE over every pattern of length <= 5 over {a, b, %, _, \\}
(escape '\\'; patterns ending in the escape must be refused) and every string of
length <= 6 over {a, b}, then a hand list: empty string and pattern, '%%', '_'
against 2-, 3- and 4-byte UTF-8 characters and a lone continuation byte, bytes
>= 0x80 in StrCompare, 'a%a%a%b' against 200 a's, and patterns at the length
cap."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_str_match_host_program(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "str_match")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=undefined", "-I", os.path.join(ROOT, "duckdb.mbt_amd", "csrc"),
           os.path.join(ROOT, "tests", "plan_harness", "str_match.cpp"), "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True)
    assert b.returncode == 0, b.stdout + b.stderr
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "str match: ok" in p.stdout
