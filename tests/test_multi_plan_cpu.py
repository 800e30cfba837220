"""CPU: csrc/multi_plan.hpp -- the work list of the filtered k-NN call with one mask per query -- under AddressSanitizer + UBSan.
tests/cpp/multi_plan_asan.cpp (its own main, the host-only header, no HIP) checks the plan against a brute-force restatement: every
(query, allowed row) pair is covered by exactly one work item, the slots are a permutation, no item holds more than 8 queries or 256
rows, the chunks respect the budget; inputs include m = 0, m = 1, m at the 256 boundaries, buckets of 8 and 9 and a mask no query uses.
It is compiled with g++ -fsanitize=address,undefined and run as a child process in the environment it inherits; nothing is loaded into
this interpreter.  The sanitizer runtimes are linked statically, so the program does not depend on which shared libraries come first."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_multi_plan_under_asan_ubsan(tmp_path):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "multi_plan_asan")
    cmd = [gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-static-libasan", "-static-libubsan", "-fno-sanitize-recover=all", "-Wall", "-Werror",
           "-I", os.path.join(ROOT, "lab_1806_vec_db_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "multi_plan_asan.cpp"), "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True)
    assert b.returncode == 0, b.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout, r.stderr)
    assert "multi_plan ok" in r.stdout and "runtime error" not in r.stderr, (r.stdout, r.stderr)
