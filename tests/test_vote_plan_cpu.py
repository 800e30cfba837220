"""CPU: csrc/vote_plan.hpp through vdb_vote_plan (GpuIndex.vote_plan; no GPU): every refusal in its order, hand-written table capacities,
the LDS / scratch boundary and the sub-chunks; and the header on its own under AddressSanitizer + UBSan -- tests/cpp/vote_plan_asan.cpp (its
own main, no HIP) compiled with g++ and run as a child process; nothing sanitized is loaded into this interpreter."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _plan(*a, **kw):
    from lab_1806_vec_db_amd import GpuIndex

    return GpuIndex.vote_plan(*a, **kw)


@pytest.mark.parametrize("args,code", [
    (dict(k=0), 1), (dict(k=4097), 1), (dict(k=4097, c=0, mode=9, column=16), 1),
    (dict(k=10, c=0), 2), (dict(k=10, c=11), 2), (dict(k=10, c=11, mode=9), 2),
    (dict(k=10, mode=2), 3), (dict(k=10, mode=-1), 3), (dict(k=10, mode="rank"), 3),
    (dict(k=10, mode="inverse", eps=0.0), 4), (dict(k=10, mode="inverse", eps=-1.0), 4), (dict(k=10, mode="inverse", eps=float("inf")), 4),
    (dict(k=10, mode="inverse", eps=float("nan"), column=16), 4),
    (dict(k=10, column=16), 5), (dict(k=10, mode="uniform", eps=float("nan"), column=99), 5),
])
def test_refusals(args, code):
    assert _plan(**args) == (code, None, None, None, None)


@pytest.mark.parametrize("k,lg,in_lds,scratch", [
    (1, 7, 1, 0), (64, 7, 1, 0), (65, 8, 1, 0), (128, 8, 1, 0), (129, 9, 1, 0), (1024, 11, 1, 0),  # 20 B x 2^11 = 40 KiB: the last in LDS
    (1025, 12, 0, 20 << 12), (2048, 12, 0, 20 << 12), (2049, 13, 0, 20 << 13), (4096, 13, 0, 20 << 13),
])
def test_table_and_place(k, lg, in_lds, scratch):
    for mode, eps in (("uniform", 0.0), ("inverse", 1e-6)):
        assert _plan(k, k, mode, eps, 15)[:4] == (0, lg, in_lds, scratch)


def test_sub_chunks():
    assert _plan(10, nq=1000)[4] == 1000  # the default budget holds everything
    assert _plan(10, nq=1000, budget=1200)[4] == 10  # 120 B of lists a query
    assert _plan(10, nq=1000, budget=1)[4] == 1  # never 0
    assert _plan(4096, nq=1000, budget=1 << 20)[4] == 6  # 160 KiB of scratch a query, under the 48 KiB of its lists
    assert _plan(4096, nq=1 << 20)[4] == (256 << 20) // (20 << 13)
    assert _plan(1024, nq=1 << 20)[4] == (256 << 20) // (1024 * 12)
    assert _plan(10, nq=0)[4] == 0


def test_vote_plan_under_asan_ubsan(tmp_path):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "vote_plan_asan")
    cmd = [gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-static-libasan", "-static-libubsan", "-fno-sanitize-recover=all", "-Wall", "-Werror",
           "-I", os.path.join(ROOT, "lab_1806_vec_db_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "vote_plan_asan.cpp"), "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True)
    assert b.returncode == 0, b.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout, r.stderr)
    assert "vote_plan ok" in r.stdout and "runtime error" not in r.stderr, (r.stdout, r.stderr)
