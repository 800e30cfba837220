"""CPU: csrc/grouped_plan.hpp -- the host arithmetic of the grouped Flat k-NN (vdb_flat_knn_grouped: list length per round, sub-chunks
under the memory budget, compaction of the open queries, capacity and hash of the walk's table) -- against a restatement in Python,
under AddressSanitizer + UBSan.  tests/cpp/grouped_plan_asan.cpp (its own main, the one host-only header, no HIP) reads the cases this
file writes and prints what the header computes; the restatement below must give the same lines.  The program is compiled with g++
-fsanitize=address,undefined and run as a child process in the environment it inherits; nothing is loaded into this interpreter."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U64 = (1 << 64) - 1
BUDGET = 256 << 20  # GROUPED_LIST_BUDGET
PAIR = 12           # GROUPED_PAIR_BYTES


# ---- the restatement ----------------------------------------------------------------------------------------------------------------------
def sat_mul(a, b):
    return min(a * b, U64)


def first_k(k, ov, m):
    return max(1, min(max(1, sat_mul(k, max(ov, 1))), m))


def next_k(kp, m):
    return max(1, min(sat_mul(kp, 4), m))


def k_sequence(k, ov, m):
    seq = [first_k(k, ov, m)]
    while seq[-1] < m and len(seq) <= 64:
        seq.append(next_k(seq[-1], m))
    return seq


def sub_chunk(nq, kp, budget):
    return max(1, min(nq, budget // sat_mul(max(kp, 1), PAIR)))


def table_lg(k, ld):
    need = 2 * (min(k, ld) + 64)
    lg = 7
    while (1 << lg) < need:
        lg += 1
    return lg


def hash_of(label, lg):
    return ((label * 2654435761) & 0xFFFFFFFF) >> (32 - lg)


def compact(kp, pairs):
    """pairs: (m, done) of the active queries 0, 2, 4, ..  -> exhausted, longest open set, open queries"""
    exhausted, nxt, open_m = 0, [], 0
    for i, (m, d) in enumerate(pairs):
        if m <= kp:
            exhausted += 1
        elif not d:
            nxt.append(2 * i)
            open_m = max(open_m, m)
    return exhausted, open_m, nxt


# ---- the cases ----------------------------------------------------------------------------------------------------------------------------
def _cases():
    cases = []
    for k, ov, m in ((10, 4, 3000), (10, 1, 3000), (10, 16, 3000), (1, 4, 1), (1, 4, 0), (100, 4, 399), (100, 4, 400), (100, 4, 401),
                     (7, 0, 1000), (1, 1, 1 << 32), (1 << 31, 16, 1 << 40), (U64, U64, U64), (3, 4, 12), (3, 4, 13), (400, 4, 3000)):
        cases.append(("K", k, ov, m))
    per = 1000 * PAIR
    for nq, kp, budget in ((100, 1000, BUDGET), (100000, 1000, BUDGET), (50, 1000, 10 * per), (50, 1000, 10 * per - 1), (50, 1000, 10 * per + 1),
                           (5, 1 << 30, BUDGET), (5, 0, BUDGET), (1, 1, 1), (0, 10, BUDGET), (7, U64, BUDGET), (22, 1000000, BUDGET),
                           (23, 1000000, BUDGET)):
        cases.append(("S", nq, kp, budget))
    for k, ld in ((1, 1), (10, 40), (10, 5), (0, 0), (64, 1000), (65, 1000), (960, 5000), (1984, 5000), (1985, 5000), (3000, 5000),
                  ((1 << 30) - 64, 1 << 31)):
        cases.append(("T", k, ld))
    for label in (0, 1, 2, 127, 128, 0xFFFFFFFE, 0x80000000, 123456789):
        for lg in (7, 12, 13, 31):
            cases.append(("H", label, lg))
    cases.append(("C", 40, []))
    cases.append(("C", 40, [(100, 1)] * 5))                                   # none unfinished
    cases.append(("C", 40, [(100, 0)] * 5))                                   # all unfinished
    cases.append(("C", 40, [(100 + i, i % 2) for i in range(9)]))             # alternating
    cases.append(("C", 40, [(100 + i, (i + 1) % 2) for i in range(9)]))
    cases.append(("C", 40, [(40, 0), (41, 0), (39, 1), (0, 0), (3000, 1), (3000, 0)]))  # whole sets end a query, done or not
    return cases


def _line(c):
    if c[0] == "C":
        return "C %d %d %s" % (c[1], len(c[2]), " ".join("%d %d" % p for p in c[2]))
    return " ".join(str(x) for x in c)


def _expected(c):
    if c[0] == "K":
        return "K " + " ".join(str(x) for x in k_sequence(*c[1:]))
    if c[0] == "S":
        return "S %d" % sub_chunk(*c[1:])
    if c[0] == "T":
        return "T %d" % table_lg(*c[1:])
    if c[0] == "H":
        return "H %d" % hash_of(*c[1:])
    ex, open_m, nxt = compact(c[1], c[2])
    return " ".join(["C", str(ex), str(open_m)] + [str(q) for q in nxt])


def test_restatement_properties():
    """what the driver relies on, checked on the restatement the header is compared with"""
    for k, ov, m in ((10, 4, 3000), (10, 1, 3000), (1, 16, 5), (100, 4, 401)):
        seq = k_sequence(k, ov, m)
        assert seq[0] == min(m, k * ov) and seq[-1] == m and all(b == min(4 * a, m) for a, b in zip(seq, seq[1:]))
    assert k_sequence(10, 4, 3000) == [40, 160, 640, 2560, 3000]
    assert sub_chunk(50, 1000, 10 * 12000) == 10 and sub_chunk(50, 1000, 10 * 12000 - 1) == 9
    assert sub_chunk(22, 1000000, BUDGET) * 1000000 * PAIR <= BUDGET < (sub_chunk(23, 1000000, BUDGET) + 1) * 1000000 * PAIR
    assert table_lg(1984, 5000) == 12 and table_lg(1985, 5000) == 13  # the last k whose table lives in LDS


def test_grouped_plan_under_asan_ubsan(tmp_path):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "grouped_plan_asan")
    cmd = [gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-static-libasan", "-static-libubsan", "-fno-sanitize-recover=all", "-Wall", "-Werror",
           "-I", os.path.join(ROOT, "lab_1806_vec_db_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "grouped_plan_asan.cpp"), "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True)
    assert b.returncode == 0, b.stderr
    cases = _cases()
    path = tmp_path / "cases.txt"
    path.write_text("\n".join(_line(c) for c in cases) + "\n")
    r = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout, r.stderr)
    assert "runtime error" not in r.stderr, r.stderr
    lines = r.stdout.strip().split("\n")
    assert lines[-1] == "grouped_plan ok" and len(lines) == len(cases) + 1
    for c, got in zip(cases, lines):
        assert got == _expected(c), (c, got, _expected(c))
