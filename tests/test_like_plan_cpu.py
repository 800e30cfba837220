"""CPU: csrc/like_plan.hpp -- the host arithmetic of the search by example rows (vdb_flat_knn_like: the check of the list limits, the
longest example list e_max, the list length K' of the call's round, the sub-chunks of queries under the memory budget) -- against a
restatement in Python, under AddressSanitizer + UBSan.  tests/cpp/like_plan_asan.cpp (its own main, the one host-only header, no HIP)
reads the cases this file writes and prints what the header computes; the restatement below must give the same lines.  The program is
compiled with g++ -fsanitize=address,undefined and run as a child process in the environment it inherits; nothing is loaded into this
interpreter."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUDGET = 256 << 20  # LIKE_LIST_BUDGET
PAIR = 12           # LIKE_PAIR_BYTES
CAP = 1024          # LIKE_MAX_EXAMPLES
U64 = (1 << 64) - 1


# ---- the restatement ----------------------------------------------------------------------------------------------------------------------
def one_lims(lims):
    if lims[0] != 0:
        return 1
    if any(b < a for a, b in zip(lims, lims[1:])):
        return 2
    return 0


def check_lims(pl, nl):
    """-> (code, e_max): 0 accepted, 1 a start that is not 0, 2 a descent, 3 a query without a positive, 4 more than CAP examples"""
    for lims in (pl, nl):
        if lims is not None and one_lims(lims):
            return one_lims(lims), None
    e_max = 0
    for q in range(len(pl) - 1):
        p = pl[q + 1] - pl[q]
        g = nl[q + 1] - nl[q] if nl is not None else 0
        if p == 0:
            return 3, None
        if p + g > CAP:
            return 4, None
        e_max = max(e_max, p + g)
    return 0, e_max


def check_drop(lims):
    if one_lims(lims):
        return one_lims(lims)
    return 4 if any(b - a > CAP for a, b in zip(lims, lims[1:])) else 0


def list_len(k, e_max, exclude, max_m):
    return max(1, min(min(k + e_max, U64) if exclude else k, max_m))


def sub_chunk(nq, kp, budget):
    return 0 if nq == 0 else max(1, min(nq, budget // (max(kp, 1) * PAIR)))


# ---- the cases ----------------------------------------------------------------------------------------------------------------------------
def _cases():
    cases = []
    lims = [
        ([0, 1, 3, 6], None), ([0, 1, 3, 6], [0, 0, 2, 2]),
        ([1, 2, 3], None),                      # a gap in front
        ([0, 2, 3], [1, 1, 1]),                 # ... of the negatives
        ([0, 3, 2, 4], None),                   # a descent
        ([0, 1, 2], [0, 5, 3]),
        ([0, 2, 2, 5], None),                   # an empty positive list
        ([0, 2, 2, 5], [0, 0, 9, 9]),           # ... even with negatives
        ([0, 1024], None), ([0, 1025], None),   # the cap
        ([0, 1, 1025], None), ([0, 1, 1026], None),
        ([0, 1000], [0, 24]), ([0, 1000], [0, 25]), ([0, 1], [0, 1023]), ([0, 1], [0, 1024]),
        ([0, 5, U64], None),                    # (no overflow in the length)
        ([0, 1], [0, U64]),
        ([0], None), ([0], [0]), ([7], None), ([0], [3]),  # nq = 0
    ]
    for pl, nl in lims:
        cases.append(("C", len(pl) - 1, int(nl is not None), *pl, *(nl or [])))
    for dl in ([0, 0, 0], [0, 0, 1, 65, 1089], [0, 1024, 2048], [0, 1025], [2, 3], [0, 4, 3], [0], [5]):
        cases.append(("D", len(dl) - 1, *dl))
    cases.append(("N",))
    for k, e, ex, m in ((10, 5, 1, 14), (10, 5, 1, 15), (10, 5, 1, 16), (10, 5, 0, 9), (10, 5, 0, 10), (10, 5, 0, 11), (10, 54, 1, 10 ** 6),
                        (10, 55, 1, 10 ** 6), (0, 0, 1, 100), (0, 0, 0, 100), (10, 5, 1, 0), (10, 5, 0, 0), (U64, 1024, 1, U64), (U64, 1024, 1, 300),
                        (1, 1024, 1, 1 << 40)):
        cases.append(("K", k, e, ex, m))
    per = 40 * PAIR
    for nq, kp, budget in ((1000, 20, BUDGET), (32768, 1034, BUDGET), (50, 40, 10 * per), (50, 40, 10 * per - 1), (50, 40, 10 * per + 1), (5, 0, BUDGET),
                           (1, 1, 1), (0, 10, BUDGET), (0, 0, 0), (7, 4096, 1), (3, 1 << 62, BUDGET), (3, U64, BUDGET)):
        cases.append(("S", nq, kp, budget))
    return cases


def _expected(c):
    if c[0] == "C":
        nq, has_neg = c[1], c[2]
        pl = list(c[3:3 + nq + 1])
        nl = list(c[3 + nq + 1:]) if has_neg else None
        code, e = check_lims(pl, nl)
        return "C %d" % code if code else "C 0 %d" % e
    if c[0] == "D":
        return "D %d" % check_drop(list(c[2:]))
    if c[0] == "N":
        return "N 5"
    if c[0] == "K":
        return "K %d" % list_len(*c[1:])
    return "S %d" % sub_chunk(*c[1:])


def test_restatement_properties():
    """what the driver and the kernels rely on, checked on the restatement the header is compared with"""
    assert check_lims([0, 1024], None) == (0, 1024) and check_lims([0, 1025], None)[0] == 4
    assert check_lims([0, 2, 2, 5], None)[0] == 3 and check_lims([1, 2], None)[0] == 1 and check_lims([0, 3, 2], None)[0] == 2
    assert check_lims([0, 1, 3], [0, 2, 2]) == (0, 3)
    # K' = k + e_max holds k rows that are no examples whenever that many exist; it is clamped to the allowed rows
    assert list_len(10, 5, True, 14) == 14 and list_len(10, 5, True, 15) == 15 and list_len(10, 5, True, 16) == 15
    assert list_len(10, 54, True, 10 ** 6) == 64 and list_len(10, 55, True, 10 ** 6) == 65  # the last list on the 8-bit first pass, the first past it
    assert list_len(10, 5, False, 10 ** 6) == 10 and list_len(10, 5, True, 0) == 1
    assert sub_chunk(50, 40, 10 * 480) == 10 and sub_chunk(50, 40, 10 * 480 - 1) == 9 and sub_chunk(50, 40, 10 * 480 + 1) == 10
    assert sub_chunk(0, 10, BUDGET) == 0 and sub_chunk(3, U64, BUDGET) == 1


def test_like_plan_under_asan_ubsan(tmp_path):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "like_plan_asan")
    cmd = [gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-static-libasan", "-static-libubsan", "-fno-sanitize-recover=all", "-Wall", "-Werror",
           "-I", os.path.join(ROOT, "lab_1806_vec_db_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "like_plan_asan.cpp"), "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True)
    assert b.returncode == 0, b.stderr
    cases = _cases()
    path = tmp_path / "cases.txt"
    path.write_text("\n".join(" ".join(str(x) for x in c) for c in cases) + "\n")
    r = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout, r.stderr)
    assert "runtime error" not in r.stderr, r.stderr
    lines = r.stdout.strip().split("\n")
    assert lines[-1] == "like_plan ok" and len(lines) == len(cases) + 1
    for c, got in zip(cases, lines):
        assert got == _expected(c), (c, got, _expected(c))
