"""CPU: csrc/mmr_plan.hpp -- the host arithmetic of the diversified Flat k-NN (vdb_flat_knn_mmr: the argument check, the LDS bytes of
k_mmr_select's state, the sub-chunks of queries under the memory budget, the list length of the call's round) -- against a restatement in
Python, under AddressSanitizer + UBSan.  tests/cpp/mmr_plan_asan.cpp (its own main, the one host-only header, no HIP) reads the cases this
file writes and prints what the header computes; the restatement below must give the same lines.  The program is compiled with g++
-fsanitize=address,undefined and run as a child process in the environment it inherits; nothing is loaded into this interpreter."""
import math
import os
import shutil
import struct
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUDGET = 256 << 20  # MMR_LIST_BUDGET
PAIR = 12           # MMR_PAIR_BYTES
MAX_FETCH = 4096    # MMR_MAX_FETCH
STAGE = 2048        # MMR_STAGE_FLOATS


def _bits(x):
    return struct.unpack("<I", struct.pack("<f", x))[0]


# ---- the restatement ----------------------------------------------------------------------------------------------------------------------
def check_args(k, fetch_k, lam_bits):
    lam = struct.unpack("<f", struct.pack("<I", lam_bits))[0]
    if math.isnan(lam) or lam < 0.0 or lam > 1.0:
        return 1
    if fetch_k < k:
        return 2
    if fetch_k > MAX_FETCH:
        return 3
    return 0


def layout(ld, dim):
    threads = 64 if ld <= 64 else 256
    pos = (max(ld, 1) + 3) // 4 * 4
    stage = min((max(dim, 1) + 3) // 4 * 4, STAGE)
    # d_p, m_p and the carried sum per position; the staged row; a (score, position) pair for each of 4 waves; a selected byte per position
    return threads, pos, stage, pos * 12 + stage * 4 + 4 * 8 + pos


def sub_chunk(nq, kp, budget):
    return max(1, min(nq, budget // (max(kp, 1) * PAIR)))


def list_len(fetch_k, max_m):
    return max(1, min(fetch_k, max_m))


# ---- the cases ----------------------------------------------------------------------------------------------------------------------------
def _cases():
    cases = []
    for lam in (0.0, -0.0, 0.25, 0.5, 1.0, 1.0000001, -1e-30, 2.0, -1.0, float("inf"), float("-inf")):
        cases.append(("A", 10, 40, _bits(lam)))
    for nan_bits in (0x7FC00000, 0xFFC00123, 0x7F800001):
        cases.append(("A", 10, 40, nan_bits))
    for k, fk in ((0, 0), (1, 1), (10, 9), (10, 10), (4096, 4096), (1, 4097), (4097, 4097), (5000, 4000), ((1 << 64) - 1, 4096), (0, (1 << 64) - 1)):
        cases.append(("A", k, fk, _bits(0.5)))
    cases.append(("A", 10, 9, _bits(2.0)))      # lambda is checked first
    cases.append(("A", 5000, 4097, _bits(0.5)))  # then fetch_k < k
    for ld in (0, 1, 2, 3, 4, 5, 63, 64, 65, 128, 200, 4095, 4096):
        for dim in (0, 1, 4, 5, 20, 960, 2047, 2048, 2049, 4096, 100000):
            cases.append(("L", ld, dim))
    per = 40 * PAIR
    for nq, kp, budget in ((1000, 40, BUDGET), (32768, 4096, BUDGET), (5462, 4096, BUDGET), (5461, 4096, BUDGET), (50, 40, 10 * per), (50, 40, 10 * per - 1),
                           (50, 40, 10 * per + 1), (5, 0, BUDGET), (1, 1, 1), (0, 10, BUDGET), (7, 4096, 1)):
        cases.append(("S", nq, kp, budget))
    for fk, m in ((40, 1000000), (40, 40), (40, 39), (40, 0), (1, 0), (0, 0), (4096, 300), (4096, 1 << 40)):
        cases.append(("F", fk, m))
    return cases


def _expected(c):
    if c[0] == "A":
        return "A %d" % check_args(*c[1:])
    if c[0] == "L":
        return "L %d %d %d %d" % layout(*c[1:])
    if c[0] == "S":
        return "S %d" % sub_chunk(*c[1:])
    return "F %d" % list_len(*c[1:])


def test_restatement_properties():
    """what the driver and the kernel rely on, checked on the restatement the header is compared with"""
    assert layout(4096, 100000)[3] == 61472 < 64 << 10  # the largest state fits the LDS a launch gets without asking for more
    assert layout(40, 960) == (64, 40, 960, 40 * 12 + 3840 + 32 + 40)
    assert all(layout(ld, d)[1] % 4 == 0 and layout(ld, d)[2] % 4 == 0 for ld in range(0, 70) for d in range(0, 70))  # the staged row is 16-byte aligned
    assert sub_chunk(50, 40, 10 * 480) == 10 and sub_chunk(50, 40, 10 * 480 - 1) == 9
    assert sub_chunk(32768, 4096, BUDGET) == 5461 and 5461 * 4096 * PAIR <= BUDGET < 5462 * 4096 * PAIR
    assert check_args(10, 40, _bits(0.5)) == 0 and check_args(10, 40, 0x7FC00000) == 1 and check_args(10, 40, _bits(-0.0)) == 0


def test_mmr_plan_under_asan_ubsan(tmp_path):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "mmr_plan_asan")
    cmd = [gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-static-libasan", "-static-libubsan", "-fno-sanitize-recover=all", "-Wall", "-Werror",
           "-I", os.path.join(ROOT, "lab_1806_vec_db_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "mmr_plan_asan.cpp"), "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True)
    assert b.returncode == 0, b.stderr
    cases = _cases()
    path = tmp_path / "cases.txt"
    path.write_text("\n".join(" ".join(str(x) for x in c) for c in cases) + "\n")
    r = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout, r.stderr)
    assert "runtime error" not in r.stderr, r.stderr
    lines = r.stdout.strip().split("\n")
    assert lines[-1] == "mmr_plan ok" and len(lines) == len(cases) + 1
    for c, got in zip(cases, lines):
        assert got == _expected(c), (c, got, _expected(c))
