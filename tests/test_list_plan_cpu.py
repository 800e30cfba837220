"""CPU: csrc/list_plan.hpp -- the host arithmetic the Flat list re-rankers share (grouped, MMR, by-example and fused search: the lists of a
sub-chunk under the memory budget, the clamp of a list length) -- against a restatement in Python, under AddressSanitizer + UBSan.
tests/cpp/list_plan_asan.cpp (its own main, the one host-only header, no HIP) reads the cases this file writes and prints what the header
computes; the restatement below must give the same lines.  The program is compiled with g++ -fsanitize=address,undefined and run as a
child process in the environment it inherits; nothing is loaded into this interpreter.

The cases are the union of the sub-chunk ("S") and list-length ("F" / "K") cases of test_grouped_plan_cpu.py, test_mmr_plan_cpu.py,
test_like_plan_cpu.py and test_fuse_plan_cpu.py, each brought to the arguments its feature hands the shared functions, and the overflow
corners of the shared functions themselves."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUDGET = 256 << 20  # LIST_BUDGET
PAIR = 12           # LIST_PAIR_BYTES
U64 = (1 << 64) - 1
SLOT = 16           # FUSE_SLOT_BYTES (the fused cases state budgets in table sizes)


# ---- the restatement ----------------------------------------------------------------------------------------------------------------------
def sub_chunk(rows, kp, budget):
    return max(1, min(rows, budget // min(max(kp, 1) * PAIR, U64)))


def list_len(want, max_m):
    return max(1, min(want, max_m))


# ---- the cases ----------------------------------------------------------------------------------------------------------------------------
def _sub_cases():
    out = []
    per = 1000 * PAIR  # grouped
    out += [(100, 1000, BUDGET), (100000, 1000, BUDGET), (50, 1000, 10 * per), (50, 1000, 10 * per - 1), (50, 1000, 10 * per + 1), (5, 1 << 30, BUDGET),
            (5, 0, BUDGET), (1, 1, 1), (0, 10, BUDGET), (7, U64, BUDGET), (22, 1000000, BUDGET), (23, 1000000, BUDGET)]
    per = 40 * PAIR  # MMR
    out += [(1000, 40, BUDGET), (32768, 4096, BUDGET), (5462, 4096, BUDGET), (5461, 4096, BUDGET), (50, 40, 10 * per), (50, 40, 10 * per - 1),
            (50, 40, 10 * per + 1), (5, 0, BUDGET), (1, 1, 1), (0, 10, BUDGET), (7, 4096, 1)]
    # by example
    out += [(1000, 20, BUDGET), (32768, 1034, BUDGET), (50, 40, 10 * per), (50, 40, 10 * per - 1), (50, 40, 10 * per + 1), (5, 0, BUDGET), (1, 1, 1),
            (0, 10, BUDGET), (0, 0, 0), (7, 4096, 1), (3, 1 << 62, BUDGET), (3, U64, BUDGET)]
    per = 4 * 40 * PAIR  # fused: (nq, s_max, kp, search, budget) -> the quotient over lists of min(max(s_max, 1), 32) x min(max(kp, 1), 4096) pairs
    for nq, s_max, kp, _search, budget in (
            (1000, 4, 40, 1, BUDGET), (50, 4, 40, 1, 10 * per), (50, 4, 40, 1, 10 * per - 1), (50, 4, 40, 1, 10 * per + 1),
            (100000, 8, 20, 1, BUDGET), (100000, 32, 20, 1, BUDGET), (100000, 1, 20, 1, BUDGET), (100000, 3, 20, 1, BUDGET),
            (1000, 16, 1024, 1, BUDGET), (1000, 16, 1024, 0, BUDGET),
            (1000, 16, 1024, 0, 10 * (SLOT << 15)), (1000, 16, 1024, 0, 10 * (SLOT << 15) - 1), (1000, 16, 1024, 0, 10 * (SLOT << 15) + 1),
            (1000, 4, 1024, 0, 1), (1000, 5, 1024, 0, 1),
            (0, 4, 40, 1, BUDGET), (0, 0, 0, 0, 0), (7, 4, 40, 1, 0), (5, 0, 0, 1, BUDGET), (5, U64, U64, 1, BUDGET), (U64, 1, 1, 0, U64)):
        out.append((nq, min(max(s_max, 1), 32) * min(max(kp, 1), 4096), budget))
    # the overflow corners: the multiply saturates, a budget of one byte, no rows
    out += [(5, U64, BUDGET), (5, U64, U64), (5, U64 // PAIR, U64), (5, U64 // PAIR + 1, U64), (U64, U64, U64), (U64, 1, U64), (9, 1, 1), (9, 0, 1),
            (0, 1, BUDGET), (0, U64, 1), (0, 0, 0)]
    return out


def _len_cases():
    out = []
    for k, ov, m in ((10, 4, 3000), (10, 1, 3000), (10, 16, 3000), (1, 4, 1), (1, 4, 0), (100, 4, 399), (100, 4, 400), (100, 4, 401), (7, 0, 1000),
                     (1, 1, 1 << 32), (1 << 31, 16, 1 << 40), (U64, U64, U64), (3, 4, 12), (3, 4, 13), (400, 4, 3000)):  # grouped: k x oversample, saturating
        out.append((min(k * max(ov, 1), U64), m))
    out += [(40, 1000000), (40, 40), (40, 39), (40, 0), (1, 0), (0, 0), (4096, 300), (4096, 1 << 40)]  # MMR
    for k, e, ex, m in ((10, 5, 1, 14), (10, 5, 1, 15), (10, 5, 1, 16), (10, 5, 0, 9), (10, 5, 0, 10), (10, 5, 0, 11), (10, 54, 1, 10 ** 6),
                        (10, 55, 1, 10 ** 6), (0, 0, 1, 100), (0, 0, 0, 100), (10, 5, 1, 0), (10, 5, 0, 0), (U64, 1024, 1, U64), (U64, 1024, 1, 300),
                        (1, 1024, 1, 1 << 40)):  # by example: k + e_max, saturating, when the examples are dropped
        out.append((min(k + e, U64) if ex else k, m))
    out += [(40, 1000), (40, 40), (40, 39), (40, 0), (0, 5), (4096, U64)]  # fused
    out += [(U64, 0), (0, U64), (U64, U64), (U64, 1), (1, U64)]  # the corners: nothing allowed, nothing wanted
    return out


def _cases():
    return [("S",) + c for c in _sub_cases()] + [("L",) + c for c in _len_cases()]


def _expected(c):
    if c[0] == "S":
        return "S %d" % sub_chunk(*c[1:])
    return "L %d" % list_len(*c[1:])


def test_restatement_properties():
    """what the drivers rely on, checked on the restatement the header is compared with"""
    assert sub_chunk(50, 40, 10 * 480) == 10 and sub_chunk(50, 40, 10 * 480 - 1) == 9 and sub_chunk(50, 40, 10 * 480 + 1) == 10
    assert sub_chunk(32768, 4096, BUDGET) == 5461 and 5461 * 4096 * PAIR <= BUDGET < 5462 * 4096 * PAIR
    assert sub_chunk(5, U64, BUDGET) == 1 and sub_chunk(9, 1, 1) == 1 and sub_chunk(0, 10, BUDGET) == 1  # kp = 2^64 - 1, budget = 1, rows = 0
    assert list_len(40, 0) == 1 and list_len(0, 5) == 1 and list_len(U64, 300) == 300                      # max_m = 0 -> 1
    for rows, kp, budget in _sub_cases():
        sub = sub_chunk(rows, kp, budget)
        assert sub >= 1 and sub <= max(rows, 1)
        assert sub == 1 or sub * max(kp, 1) * PAIR <= budget  # more than one list per sub-chunk only under the budget


def test_list_plan_under_asan_ubsan(tmp_path):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "list_plan_asan")
    cmd = [gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-static-libasan", "-static-libubsan", "-fno-sanitize-recover=all", "-Wall", "-Werror",
           "-I", os.path.join(ROOT, "lab_1806_vec_db_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "list_plan_asan.cpp"), "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True)
    assert b.returncode == 0, b.stderr
    cases = _cases()
    path = tmp_path / "cases.txt"
    path.write_text("\n".join(" ".join(str(x) for x in c) for c in cases) + "\n")
    r = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout, r.stderr)
    assert "runtime error" not in r.stderr, r.stderr
    lines = r.stdout.strip().split("\n")
    assert lines[-1] == "list_plan ok" and len(lines) == len(cases) + 1
    for c, got in zip(cases, lines):
        assert got == _expected(c), (c, got, _expected(c))
