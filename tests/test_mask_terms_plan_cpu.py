"""CPU: mask_terms_check of csrc/mask_sets.hpp -- the argument check of the equality masks (vdb_mask_create_where*) -- under
AddressSanitizer + UBSan.  tests/cpp/mask_terms_asan.cpp (its own main, the host-only header, no HIP) checks every rejection the call
documents with its whole message and in the order of detection -- null pointers, too many masks, a term_lims that does not start at 0
or decreases, nine terms in a mask (eight pass), column 16 (15 passes) -- and the legal edge forms (no masks with null pointers, masks
without terms).  It is compiled with g++ -fsanitize=address,undefined and run as a child process in the environment it inherits;
nothing is loaded into this interpreter.  The sanitizer runtimes are linked statically, so the program does not depend on which
shared libraries come first."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_mask_terms_under_asan_ubsan(tmp_path):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "mask_terms_asan")
    cmd = [gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-static-libasan", "-static-libubsan", "-fno-sanitize-recover=all", "-Wall", "-Werror",
           "-I", os.path.join(ROOT, "lab_1806_vec_db_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "mask_terms_asan.cpp"), "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True)
    assert b.returncode == 0, b.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout, r.stderr)
    assert "mask_terms ok" in r.stdout and "runtime error" not in r.stderr, (r.stdout, r.stderr)
