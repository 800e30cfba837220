"""CPU: csrc/mask_partition.hpp -- the host part of the single-pass grouping of a label column by code (vdb_mask_create_partition,
vdb_index_label_counts) -- under AddressSanitizer + UBSan.  tests/cpp/mask_partition_asan.cpp (its own main, the one host-only header,
no HIP) drives the argument check (a duplicate at adjacent and at distant positions, LABEL_NONE in the list, the column and count
limits, a null array), the sorted table and its permutation for 0, 1, 1024, 1025 and 2049 codes across chunks, and compares
mask_partition_find -- the host twin of the binary search a lane runs -- by brute force for present, absent, smallest and largest codes.
It is compiled with g++ -fsanitize=address,undefined and run as a child process in the environment it inherits; nothing is loaded into
this interpreter.  The sanitizer runtimes are linked statically, so the program does not depend on which shared libraries come first."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_mask_partition_under_asan_ubsan(tmp_path):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "mask_partition_asan")
    cmd = [gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-static-libasan", "-static-libubsan", "-fno-sanitize-recover=all", "-Wall", "-Werror",
           "-I", os.path.join(ROOT, "lab_1806_vec_db_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "mask_partition_asan.cpp"), "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True)
    assert b.returncode == 0, b.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout, r.stderr)
    assert "mask_partition ok" in r.stdout and "runtime error" not in r.stderr, (r.stdout, r.stderr)
