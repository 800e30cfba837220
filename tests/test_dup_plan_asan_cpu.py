"""CPU: csrc/dup_plan.hpp under AddressSanitizer + UBSan -- tests/cpp/dup_plan_asan.cpp (its own main, the host-only header, no HIP) is
compiled with g++ -fsanitize=address,undefined and run as a child process in the environment it inherits; nothing is loaded into this
interpreter.  The sanitizer runtimes are linked statically, so the program does not depend on which shared libraries come first."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_dup_plan_under_asan_ubsan(tmp_path):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "dup_plan_asan")
    cmd = [gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-static-libasan", "-static-libubsan", "-fno-sanitize-recover=all", "-Wall", "-Werror",
           "-I", os.path.join(ROOT, "lab_1806_vec_db_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "dup_plan_asan.cpp"), "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True)
    assert b.returncode == 0, b.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout, r.stderr)
    assert "dup_plan ok" in r.stdout and "runtime error" not in r.stderr, (r.stdout, r.stderr)
