"""CPU: csrc/fuse_plan.hpp -- the host arithmetic of the fused multi-query search (vdb_flat_knn_fused / vdb_fuse_lists_device: the argument
check with a code per refusal, S_max, the size and the place of the kernel's table, its scratch bytes, the sub-chunks of fused queries
under the memory budget) -- against a restatement in Python, under AddressSanitizer + UBSan.  tests/cpp/fuse_plan_asan.cpp (its own main,
the one host-only header, no HIP) reads the cases this file writes and prints what the header computes; the restatement below must give
the same lines.  The program is compiled with g++ -fsanitize=address,undefined and run as a child process in the environment it
inherits; nothing is loaded into this interpreter.  The exported vdb_fuse_plan (no GPU needed) is held against the same restatement."""
import ctypes as C
import math
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUDGET = 256 << 20   # FUSE_LIST_BUDGET
PAIR = 12            # FUSE_PAIR_BYTES
MAX_LISTS, MAX_FETCH, MAX_ENTRIES, MAX_SUBQ = 32, 4096, 16384, 16384
MIN_LG, LDS_MAX_LG, SLOT = 6, 13, 16
U64 = (1 << 64) - 1
RRF, MIN = 0, 1


def fbits(x):
    return struct.unpack("<I", struct.pack("<f", x))[0]


# ---- the restatement ----------------------------------------------------------------------------------------------------------------------
def check_args(mode, list_form, nq, k, fetch_k, c, lims, weights):
    """-> (code, s_max): 0 accepted, else the first of 1 mode, 3 start, 4 descent, 5 no list, 6 too many lists, 7 fetch_k < k, 8 fetch_k
    above 4096, 9 entries above 16384, 10 weights with MIN, 11 a bad weight, 12 a bad c  (2, NULL limits, has no case line)"""
    if mode not in (RRF, MIN):
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
        if any(not (w > 0.0) or math.isinf(w) for w in weights):
            return 11, None
    if not (c >= 0.0) or math.isinf(c):
        return 12, None
    return 0, s_max


def table_lg(s_max, ld):
    lg = MIN_LG
    while (1 << lg) < 2 * min(s_max * ld, MAX_ENTRIES):
        lg += 1
    return lg


def scratch_bytes(nq, lg):
    return 0 if lg <= LDS_MAX_LG else nq * (SLOT << lg)


def list_len(fetch_k, max_m):
    return max(1, min(fetch_k, max_m))


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


def fuse_hash(row, lg):
    return ((row * 2654435761) & 0xFFFFFFFF) >> (32 - lg)


# ---- the cases ----------------------------------------------------------------------------------------------------------------------------
def _check_cases():
    """(mode, list_form, k, fetch_k, c, lims, weights)"""
    nan, inf = float("nan"), float("inf")
    ok = [0, 2, 5]
    out = [
        (RRF, 0, 10, 40, 60.0, ok, None), (MIN, 0, 10, 40, 60.0, ok, None), (RRF, 0, 10, 40, 0.0, ok, [1.0, 2.0, 1e-3, 1e3, 0.5]),
        (2, 0, 10, 40, 60.0, ok, None), (-1, 0, 10, 40, 60.0, ok, None),                         # a bad mode
        (RRF, 0, 10, 40, 60.0, [1, 2], None), (RRF, 0, 10, 40, 60.0, [0, 3, 2, 4], None),        # the limits
        (RRF, 0, 10, 40, 60.0, [0, 2, 2, 5], None),                                              # a fused query without a sub-query
        (RRF, 0, 10, 40, 60.0, [0, 32], None), (RRF, 0, 10, 40, 60.0, [0, 33], None),            # S = 32 / 33
        (RRF, 0, 10, 40, 60.0, [0, 1, 33, 34], None), (RRF, 0, 10, 40, 60.0, [0, 1, 34, 35], None),
        (RRF, 0, 10, 40, 60.0, [0, U64], None), (RRF, 0, 10, 40, 60.0, [0, 5, U64], None),       # (no overflow in the lengths)
        (RRF, 0, 10, 10, 60.0, ok, None), (RRF, 0, 10, 9, 60.0, ok, None), (RRF, 1, 10, 9, 60.0, ok, None),  # fetch_k = k, below it; the list form
        (RRF, 0, 0, 0, 60.0, ok, None),
        (RRF, 0, 10, 4096, 60.0, [0, 4], None), (RRF, 0, 10, 4097, 60.0, [0, 1], None), (RRF, 1, 10, 4097, 60.0, [0, 1], None),
        (RRF, 0, U64, U64, 60.0, [0, 1], None),
        (RRF, 0, 10, 4096, 60.0, [0, 5], None),                                                  # 5 x 4096 entries
        (RRF, 0, 10, 512, 60.0, [0, 32], None), (RRF, 0, 10, 513, 60.0, [0, 32], None),          # S x F = 16384 / 16416
        (RRF, 0, 10, 16384, 60.0, [0, 1], None),
        (RRF, 0, 10, 1024, 60.0, [0, 16, 17], None), (RRF, 0, 10, 1024, 60.0, [0, 1, 18], None), # ... 16 x 1024 / 17 x 1024 in any fused query
        (MIN, 0, 10, 40, 60.0, ok, [1.0] * 5),                                                   # weights with MIN
        (MIN, 0, 10, 40, 60.0, ok, [nan] * 5),                                                   # ... reported before the weights are read
    ]
    for bad in (0.0, -0.0, -1.0, nan, inf, -inf):
        out.append((RRF, 0, 10, 40, 60.0, ok, [1.0, 1.0, 1.0, 1.0, bad]))
    out.append((RRF, 0, 10, 40, 60.0, ok, [1e-45, 3e38, 1.0, 1.0, 1.0]))                         # the smallest and a huge finite weight
    for c in (0.0, -0.0, 1e-45, 3e38, -1e-45, -1.0, nan, inf, -inf):
        out.append((RRF, 0, 10, 40, c, ok, None))
    out.append((MIN, 0, 10, 40, nan, ok, None))                                                   # c is checked under MIN too
    out.append((RRF, 0, 10, 40, 60.0, [0], None))                                                 # nq = 0
    out.append((RRF, 0, 10, 40, 60.0, [7], None))
    out.append((RRF, 0, 10, 4097, 60.0, [0], None))
    return out


def _cases():
    cases = []
    for mode, lf, k, f, c, lims, w in _check_cases():
        cases.append(("C", mode, lf, len(lims) - 1, k, f, "%x" % fbits(c), int(w is not None), *lims, *("%x" % fbits(x) for x in (w or []))))
    cases.append(("N",))
    for s_max, ld in ((1, 1), (1, 32), (1, 33), (2, 16), (3, 40), (8, 64), (4, 1024), (4, 1025), (5, 1024), (8, 512), (8, 513), (2, 2048),
                      (1, 4096), (2, 4096), (16, 1024), (32, 512), (0, 0), (32, 4096)):
        cases.append(("T", s_max, ld))
    for f, m in ((40, 1000), (40, 40), (40, 39), (40, 0), (0, 5), (4096, U64)):
        cases.append(("K", f, m))
    per = 4 * 40 * PAIR
    for nq, s_max, kp, search, budget in (
            (1000, 4, 40, 1, BUDGET), (50, 4, 40, 1, 10 * per), (50, 4, 40, 1, 10 * per - 1), (50, 4, 40, 1, 10 * per + 1),  # the list budget +- 1
            (100000, 8, 20, 1, BUDGET), (100000, 32, 20, 1, BUDGET), (100000, 1, 20, 1, BUDGET), (100000, 3, 20, 1, BUDGET),  # the sub-query cap
            (1000, 16, 1024, 1, BUDGET), (1000, 16, 1024, 0, BUDGET),                                                        # the scratch under the budget
            (1000, 16, 1024, 0, 10 * (SLOT << 15)), (1000, 16, 1024, 0, 10 * (SLOT << 15) - 1), (1000, 16, 1024, 0, 10 * (SLOT << 15) + 1),
            (1000, 4, 1024, 0, 1), (1000, 5, 1024, 0, 1),                                                                    # in LDS: no scratch to bound
            (0, 4, 40, 1, BUDGET), (0, 0, 0, 0, 0), (7, 4, 40, 1, 0), (5, 0, 0, 1, BUDGET), (5, U64, U64, 1, BUDGET), (U64, 1, 1, 0, U64)):
        cases.append(("S", nq, s_max, kp, search, budget))
    for row, lg in ((0, 6), (1, 6), (1499, 6), (0xFFFFFFFE, 15), (12345, 13), (7, 15)):
        cases.append(("H", row, lg))
    return cases


def _expected(c, spec=None):
    if c[0] == "C":
        mode, lf, k, f, cc, lims, w = spec
        cc32 = struct.unpack("<f", struct.pack("<I", fbits(cc)))[0]
        w32 = None if w is None else [struct.unpack("<f", struct.pack("<f", x))[0] for x in w]
        code, s_max = check_args(mode, lf, len(lims) - 1, k, f, cc32, lims, w32)
        return "C %d" % code if code else "C 0 %d" % s_max
    if c[0] == "N":
        return "N 2"
    if c[0] == "T":
        lg = table_lg(c[1], c[2])
        return "T %d %d %d" % (lg, int(lg <= LDS_MAX_LG), scratch_bytes(3, lg))
    if c[0] == "K":
        return "K %d" % list_len(*c[1:])
    if c[0] == "S":
        return "S %d" % sub_chunk(*c[1:])
    return "H %d" % fuse_hash(*c[1:])


def test_restatement_properties():
    """what the driver and the kernel rely on, checked on the restatement the header is compared with"""
    ok = [0, 2, 5]
    assert check_args(RRF, 0, 2, 10, 40, 60.0, ok, None) == (0, 3)
    assert [check_args(RRF, 0, 1, 10, 40, 60.0, [0, s], None)[0] for s in (32, 33)] == [0, 6]
    assert [check_args(RRF, 0, 1, 10, f, 60.0, [0, 1], None)[0] for f in (4096, 4097)] == [0, 8]
    assert [check_args(RRF, 0, 1, 10, f, 60.0, [0, 32], None)[0] for f in (512, 513)] == [0, 9]
    assert check_args(RRF, 0, 1, 10, 9, 60.0, [0, 1], None)[0] == 7 and check_args(RRF, 1, 1, 10, 9, 60.0, [0, 1], None)[0] == 0
    # the table: load at most one half, LDS up to 2^13 slots = 4096 entries, one slot more and it is scratch
    for s_max, ld in ((1, 1), (3, 40), (4, 1024), (5, 1024), (16, 1024), (32, 512)):
        assert (1 << table_lg(s_max, ld)) >= 2 * s_max * ld and ((1 << table_lg(s_max, ld)) < 4 * s_max * ld or table_lg(s_max, ld) == MIN_LG)
    assert table_lg(4, 1024) == 13 and scratch_bytes(3, 13) == 0 and table_lg(4, 1025) == 14 and scratch_bytes(3, 14) == 3 * 16 * 16384
    assert table_lg(16, 1024) == 15 and SLOT << LDS_MAX_LG == 128 << 10
    # the sub-chunk: the lists under the budget, at most 16384 sub-queries in one list call, the scratch under the budget
    per = 4 * 40 * PAIR
    assert [sub_chunk(50, 4, 40, 1, 10 * per + d) for d in (-1, 0, 1)] == [9, 10, 10]
    assert sub_chunk(100000, 32, 20, 1, BUDGET) == 512 and sub_chunk(100000, 3, 20, 1, BUDGET) == 5461
    assert sub_chunk(1000, 16, 1024, 0, BUDGET) == 512 and sub_chunk(0, 4, 40, 1, BUDGET) == 0 and sub_chunk(7, 4, 40, 1, 0) == 1


def test_fuse_plan_under_asan_ubsan(tmp_path):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "fuse_plan_asan")
    cmd = [gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-static-libasan", "-static-libubsan", "-fno-sanitize-recover=all", "-Wall", "-Werror",
           "-I", os.path.join(ROOT, "lab_1806_vec_db_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "fuse_plan_asan.cpp"), "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True)
    assert b.returncode == 0, b.stderr
    cases, specs = _cases(), _check_cases()
    path = tmp_path / "cases.txt"
    path.write_text("\n".join(" ".join(str(x) for x in c) for c in cases) + "\n")
    r = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout, r.stderr)
    assert "runtime error" not in r.stderr, r.stderr
    lines = r.stdout.strip().split("\n")
    assert lines[-1] == "fuse_plan ok" and len(lines) == len(cases) + 1
    codes = set()
    for i, (c, got) in enumerate(zip(cases, lines)):
        exp = _expected(c, specs[i] if c[0] == "C" else None)
        assert got == exp, (c, got, exp)
        if c[0] == "C":
            codes.add(int(got.split()[1]))
    assert codes == set(range(13)) - {2}  # every refusal code has a case (2, NULL limits, is the N line)


def test_exported_plan_matches_the_restatement():
    from lab_1806_vec_db_amd import _lib as L

    so = L.load()
    for mode, lf, k, f, c, lims, w in _check_cases():
        if lf:
            continue  # (the export plans the search forms)
        lm = np.asarray(lims, dtype=np.uint64)
        wa = None if w is None else np.asarray(w, dtype=np.float32)
        code, in_lds, lg = C.c_int(-1), C.c_int(-1), C.c_uint32(99)
        s_max, scratch, sub = C.c_uint64(U64), C.c_uint64(U64), C.c_uint64(U64)
        st = so.vdb_fuse_plan(mode, lm.ctypes.data_as(L.u64p), len(lims) - 1, k, f, None if wa is None else wa.ctypes.data_as(L.f32p), c, 0,
                              C.byref(code), C.byref(s_max), C.byref(lg), C.byref(in_lds), C.byref(scratch), C.byref(sub))
        assert st == 0
        c32 = float(np.float32(c))
        ecode, es = check_args(mode, 0, len(lims) - 1, k, f, c32, lims, None if wa is None else [float(x) for x in wa])
        assert code.value == ecode, (mode, k, f, c, lims, w)
        if ecode:
            assert (s_max.value, lg.value, in_lds.value) == (U64, 99, -1)  # nothing else is written
        else:
            elg = table_lg(es, f)
            assert (s_max.value, lg.value, in_lds.value, scratch.value) == (es, elg, int(elg <= LDS_MAX_LG), scratch_bytes(1, elg))
            assert sub.value == sub_chunk(len(lims) - 1, es, f, 1, BUDGET)
    code = C.c_int(-1)
    assert so.vdb_fuse_plan(0, None, 3, 1, 1, None, 60.0, 0, C.byref(code), None, None, None, None, None) == 0 and code.value == 2
    lm = np.asarray([0, 4] * 1, dtype=np.uint64)
    sub = C.c_uint64(0)
    assert so.vdb_fuse_plan(0, lm.ctypes.data_as(L.u64p), 1, 10, 40, None, 60.0, 1, C.byref(code), None, None, None, None, C.byref(sub)) == 0
    assert code.value == 0 and sub.value == 1
    assert so.vdb_fuse_plan(0, lm.ctypes.data_as(L.u64p), 1, 10, 40, None, 60.0, 0, None, None, None, None, None, None) == 1  # no out_code
