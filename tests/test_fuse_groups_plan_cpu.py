"""CPU: csrc/fuse_groups_plan.hpp -- the host arithmetic of the document-level fused search (vdb_flat_knn_fused_groups /
vdb_fuse_groups_device: the argument check with a code per refusal, the size and the place of the kernel's table, its scratch bytes, the
sub-chunks of fused queries under the memory budget) -- against a restatement in Python, under AddressSanitizer + UBSan.
tests/cpp/fuse_groups_plan_asan.cpp (its own main, the plan header alone, no HIP) reads the cases this file writes and prints what the
header computes; the restatement below must give the same lines.  The program is compiled with g++ -fsanitize=address,undefined and run
as a child process in the environment it inherits; nothing is loaded into this interpreter.  The exported vdb_fuse_groups_plan (no GPU
needed) is held against the same restatement."""
import math
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUDGET = 256 << 20
PAIR = 12
MAX_LISTS, MAX_FETCH, MAX_ENTRIES, MAX_SUBQ = 32, 4096, 16384, 16384
MIN_LG, SLOT, COLUMNS = 6, 28, 16
LDS_BYTES = 160 << 10       # LDS of a gfx950 CU
LDS_MAX_LG = 12             # the largest power of two of 28-byte slots under it
U64 = (1 << 64) - 1
RRF, MIN, SUM = 0, 1, 2


def fbits(x):
    return struct.unpack("<I", struct.pack("<f", x))[0]


# ---- the restatement ----------------------------------------------------------------------------------------------------------------------
def check_args(mode, list_form, nq, k, fetch_k, c, column, lims, weights):
    """-> (code, s_max): 0 accepted, else the first of 1 mode, 3 start, 4 descent, 5 no list, 6 too many lists, 7 fetch_k < k, 8 fetch_k
    above 4096, 9 entries above 16384, 10 weights with MIN, 13 weights with SUM, 11 a bad weight, 12 a bad c, 14 the column  (2, NULL
    limits, has no case line)"""
    if mode not in (RRF, MIN, SUM):
        return 1, None
    if lims[0] != 0:
        return 3, None
    if any(b < a for a, b in zip(lims, lims[1:])):
        return 4, None
    sizes = [b - a for a, b in zip(lims, lims[1:])]
    for s in sizes:
        if s == 0:
            return 5, None
        if s > MAX_LISTS:
            return 6, None
    s_max = max(sizes, default=0)
    if not list_form and fetch_k < k:
        return 7, None
    if fetch_k > MAX_FETCH:
        return 8, None
    if s_max * fetch_k > MAX_ENTRIES:
        return 9, None
    if weights is not None:
        if mode == MIN:
            return 10, None
        if mode == SUM:
            return 13, None
        if any(not (w > 0.0) or math.isinf(w) for w in weights):
            return 11, None
    if not (c >= 0.0) or math.isinf(c):
        return 12, None
    if column >= COLUMNS:
        return 14, None
    return 0, s_max


def table_lg(s_max, ld):
    lg = MIN_LG
    while (1 << lg) < 2 * min(s_max * ld, MAX_ENTRIES):
        lg += 1
    return lg


def scratch_bytes(nq, lg):
    return 0 if lg <= LDS_MAX_LG else nq * (SLOT << lg)


def sub_chunk(nq, s_max, kp, search, budget):
    if nq == 0:
        return 0
    sm, kk = min(max(s_max, 1), MAX_LISTS), min(max(kp, 1), MAX_FETCH)
    fit = nq
    if search:
        fit = min(fit, budget // (sm * kk * PAIR), MAX_SUBQ // sm)
    lg = table_lg(sm, kk)
    if lg > LDS_MAX_LG:
        fit = min(fit, budget // (SLOT << lg))
    return max(1, fit)


def group_hash(key_low, lg):
    return ((key_low * 2654435761) & 0xFFFFFFFF) >> (32 - lg)


# ---- the cases ----------------------------------------------------------------------------------------------------------------------------
def _check_cases():
    """(mode, list_form, k, fetch_k, c, column, lims, weights)"""
    nan, inf = float("nan"), float("inf")
    ok = [0, 2, 5]
    out = [
        (RRF, 0, 10, 40, 60.0, 0, ok, None), (MIN, 0, 10, 40, 60.0, 3, ok, None), (SUM, 0, 10, 40, 60.0, 15, ok, None),
        (RRF, 0, 10, 40, 0.0, 0, ok, [1.0, 2.0, 1e-3, 1e3, 0.5]),
        (3, 0, 10, 40, 60.0, 0, ok, None), (-1, 0, 10, 40, 60.0, 0, ok, None), (3, 0, 10, 40, 60.0, 99, [1, 2], None),   # a bad mode comes first
        (SUM, 0, 10, 40, 60.0, 0, [1, 2], None), (SUM, 0, 10, 40, 60.0, 0, [0, 3, 2, 4], None),                          # the limits
        (SUM, 0, 10, 40, 60.0, 0, [0, 2, 2, 5], None),                                                                   # a fused query without a sub-query
        (SUM, 0, 10, 40, 60.0, 0, [0, 32], None), (SUM, 0, 10, 40, 60.0, 0, [0, 33], None),                              # S = 32 / 33
        (RRF, 0, 10, 40, 60.0, 0, [0, U64], None), (RRF, 0, 10, 40, 60.0, 0, [0, 5, U64], None),                         # (no overflow in the lengths)
        (SUM, 0, 10, 10, 60.0, 0, ok, None), (SUM, 0, 10, 9, 60.0, 0, ok, None), (SUM, 1, 10, 9, 60.0, 0, ok, None),     # fetch_k = k, below it; the list form
        (RRF, 0, 0, 0, 60.0, 0, ok, None),
        (MIN, 0, 10, 4096, 60.0, 0, [0, 4], None), (MIN, 0, 10, 4097, 60.0, 0, [0, 1], None), (MIN, 1, 10, 4097, 60.0, 0, [0, 1], None),
        (SUM, 0, 10, 512, 60.0, 0, [0, 32], None), (SUM, 0, 10, 513, 60.0, 0, [0, 32], None),                            # S x F = 16384 / 16416
        (RRF, 0, 10, 1024, 60.0, 0, [0, 16, 17], None), (RRF, 0, 10, 1024, 60.0, 0, [0, 1, 18], None),
        (MIN, 0, 10, 40, 60.0, 0, ok, [1.0] * 5), (SUM, 0, 10, 40, 60.0, 0, ok, [1.0] * 5),                              # weights with MIN, with SUM
        (SUM, 0, 10, 40, 60.0, 0, ok, [nan] * 5), (SUM, 0, 10, 40, nan, 99, ok, [1.0] * 5),                              # ... reported before weights, c, column
        (SUM, 0, 10, 513, 60.0, 0, [0, 32], [1.0] * 32),                                                                 # ... and behind the entries
    ]
    for bad in (0.0, -0.0, -1.0, nan, inf, -inf):
        out.append((RRF, 0, 10, 40, 60.0, 0, ok, [1.0, 1.0, 1.0, 1.0, bad]))
    out.append((RRF, 0, 10, 40, nan, 99, ok, [1.0, 1.0, 1.0, 1.0, nan]))                                                  # a bad weight before a bad c
    for c in (0.0, -0.0, 1e-45, 3e38, -1e-45, -1.0, nan, inf, -inf):
        out.append((RRF, 0, 10, 40, c, 0, ok, None))
    out.append((SUM, 0, 10, 40, nan, 99, ok, None))                                                                       # c is checked under SUM too, before the column
    for col in (15, 16, 17, 0xFFFFFFFF):
        out.append((SUM, 0, 10, 40, 60.0, col, ok, None))
    out.append((MIN, 1, 10, 40, 60.0, 16, ok, None))
    out.append((RRF, 0, 10, 40, 60.0, 0, [0], None))                                                                      # nq = 0
    out.append((RRF, 0, 10, 40, 60.0, 16, [0], None))
    out.append((RRF, 0, 10, 40, 60.0, 0, [7], None))
    return out


def _cases():
    cases = []
    for mode, lf, k, f, c, col, lims, w in _check_cases():
        cases.append(("C", mode, lf, len(lims) - 1, k, f, "%x" % fbits(c), col, int(w is not None), *lims, *("%x" % fbits(x) for x in (w or []))))
    cases.append(("N",))
    for s_max, ld in ((1, 1), (1, 32), (1, 33), (2, 16), (3, 40), (8, 64), (2, 1024), (2, 1025), (4, 512), (4, 513), (4, 1024), (5, 1024), (8, 512),
                      (1, 2048), (1, 2049), (1, 4096), (2, 4096), (16, 1024), (32, 512), (0, 0), (32, 4096)):
        cases.append(("T", s_max, ld))
    per = 4 * 40 * PAIR
    for nq, s_max, kp, search, budget in (
            (1000, 4, 40, 1, BUDGET), (50, 4, 40, 1, 10 * per), (50, 4, 40, 1, 10 * per - 1), (50, 4, 40, 1, 10 * per + 1),  # the list budget +- 1
            (100000, 8, 20, 1, BUDGET), (100000, 32, 20, 1, BUDGET), (100000, 1, 20, 1, BUDGET), (100000, 3, 20, 1, BUDGET),  # the sub-query cap
            (1000, 16, 1024, 1, BUDGET), (1000, 16, 1024, 0, BUDGET),                                                        # the scratch under the budget
            (1000, 16, 1024, 0, 10 * (SLOT << 15)), (1000, 16, 1024, 0, 10 * (SLOT << 15) - 1), (1000, 16, 1024, 0, 10 * (SLOT << 15) + 1),
            (1000, 4, 1024, 0, 10 * (SLOT << 13)), (1000, 4, 1024, 0, 10 * (SLOT << 13) - 1),                                # 2^13 slots: scratch here
            (1000, 2, 1024, 0, 1), (1000, 4, 512, 0, 1),                                                                     # in LDS: no scratch to bound
            (0, 4, 40, 1, BUDGET), (0, 0, 0, 0, 0), (7, 4, 40, 1, 0), (5, 0, 0, 1, BUDGET), (5, U64, U64, 1, BUDGET), (U64, 1, 1, 0, U64)):
        cases.append(("S", nq, s_max, kp, search, budget))
    for key, lg in ((0, 6), (1, 6), (1499, 6), (0xFFFFFFFE, 15), (12345, 12), (7, 15)):
        cases.append(("H", key, lg))
    return cases


def _expected(c, spec=None):
    if c[0] == "C":
        mode, lf, k, f, cc, col, lims, w = spec
        cc32 = struct.unpack("<f", struct.pack("<I", fbits(cc)))[0]
        w32 = None if w is None else [struct.unpack("<f", struct.pack("<f", x))[0] for x in w]
        code, s_max = check_args(mode, lf, len(lims) - 1, k, f, cc32, col, lims, w32)
        return "C %d" % code if code else "C 0 %d" % s_max
    if c[0] == "N":
        return "N 2"
    if c[0] == "T":
        lg = table_lg(c[1], c[2])
        return "T %d %d %d %d" % (lg, int(lg <= LDS_MAX_LG), scratch_bytes(3, lg), SLOT << lg)
    if c[0] == "S":
        return "S %d" % sub_chunk(*c[1:])
    return "H %d" % group_hash(*c[1:])


def test_restatement_properties():
    """what the driver and the kernel rely on, checked on the restatement the header is compared with"""
    ok = [0, 2, 5]
    assert check_args(SUM, 0, 2, 10, 40, 60.0, 0, ok, None) == (0, 3)
    assert check_args(SUM, 0, 2, 10, 40, 60.0, 0, ok, [1.0] * 5)[0] == 13 and check_args(MIN, 0, 2, 10, 40, 60.0, 0, ok, [1.0] * 5)[0] == 10
    assert [check_args(RRF, 0, 2, 10, 40, 60.0, col, ok, None)[0] for col in (15, 16)] == [0, 14]
    # the slot: an 8-byte key, accumulator, stamp, representative, its distance, half a u64 sort key; the LDS limit is the largest power of
    # two of slots that fits the 160 KiB of a CU beside the kernel's few static words -- lower than the 2^13 of the 16-byte row-level slot
    assert SLOT == 8 + 4 + 4 + 4 + 4 + 8 // 2
    assert (SLOT << LDS_MAX_LG) + 64 <= LDS_BYTES < (SLOT << (LDS_MAX_LG + 1)) and LDS_MAX_LG < 13
    # load at most one half: an entry opens at most one group
    for s_max, ld in ((1, 1), (3, 40), (2, 1024), (4, 1024), (16, 1024), (32, 512)):
        assert (1 << table_lg(s_max, ld)) >= 2 * s_max * ld
    assert table_lg(2, 1024) == 12 and scratch_bytes(3, 12) == 0 and table_lg(2, 1025) == 13 and scratch_bytes(3, 13) == 3 * 28 * 8192
    assert table_lg(32, 512) == 15
    per = 4 * 40 * PAIR
    assert [sub_chunk(50, 4, 40, 1, 10 * per + d) for d in (-1, 0, 1)] == [9, 10, 10]
    assert sub_chunk(1000, 16, 1024, 0, BUDGET) == BUDGET // (28 << 15) == 292 and sub_chunk(0, 4, 40, 1, BUDGET) == 0


def test_fuse_groups_plan_under_asan_ubsan(tmp_path):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "fuse_groups_plan_asan")
    cmd = [gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-static-libasan", "-static-libubsan", "-fno-sanitize-recover=all", "-Wall", "-Werror",
           "-I", os.path.join(ROOT, "lab_1806_vec_db_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "fuse_groups_plan_asan.cpp"), "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True)
    assert b.returncode == 0, b.stderr
    cases, specs = _cases(), _check_cases()
    path = tmp_path / "cases.txt"
    path.write_text("\n".join(" ".join(str(x) for x in c) for c in cases) + "\n")
    r = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout, r.stderr)
    assert "runtime error" not in r.stderr, r.stderr
    lines = r.stdout.strip().split("\n")
    assert lines[-1] == "fuse_groups_plan ok" and len(lines) == len(cases) + 1
    codes = []
    for i, (c, got) in enumerate(zip(cases, lines)):
        exp = _expected(c, specs[i] if c[0] == "C" else None)
        assert got == exp, (c, got, exp)
        if c[0] == "C":
            codes.append(int(got.split()[1]))
    assert set(codes) == set(range(15)) - {2}  # every refusal code has a case (2, NULL limits, is the N line)


def test_exported_plan_matches_the_restatement():
    from lab_1806_vec_db_amd import GpuIndex

    for mode, lf, k, f, c, col, lims, w in _check_cases():
        if lf:
            continue  # (the export plans the search forms)
        got = GpuIndex.fuse_groups_plan(lims, k, f, mode, w, c, col)
        c32 = float(np.float32(c))
        ecode, es = check_args(mode, 0, len(lims) - 1, k, f, c32, col, lims, None if w is None else [float(np.float32(x)) for x in w])
        assert got[0] == ecode, (mode, k, f, c, col, lims, w)
        if ecode == 0:
            elg = table_lg(es, f)
            assert got[1:] == (es, elg, int(elg <= LDS_MAX_LG), scratch_bytes(1, elg), sub_chunk(len(lims) - 1, es, f, 1, BUDGET))
    assert GpuIndex.fuse_groups_plan([0, 2], 10, 1024, "sum")[1:5] == (2, 12, 1, 0)
    assert GpuIndex.fuse_groups_plan([0, 4], 10, 1024, "sum")[1:5] == (4, 13, 0, 28 << 13)
    assert GpuIndex.fuse_groups_plan([0, 4], 10, 40, "rrf", budget=1)[5] == 1
    assert GpuIndex.fuse_groups_plan([0, 4], 10, 40, "nonsense")[0] == 1
