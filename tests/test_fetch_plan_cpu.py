"""CPU: vdb_fetch_plan (host utility, no GPU) against a Python restatement.

A bulk fetch of the rows R is carried out DIRECT (one copy out of the table) when R is one ascending run of consecutive rows, and
GATHER otherwise, in chunks of max(1, chunk_bytes // out_row_bytes) output rows.  Checked: the routes of runs and of runs with one swap,
one duplicate or one gap, m = 0 and m = 1; the chunk counts for chunk_bytes in {1, row, row + 1, 7 rows, huge} with m around the
multiples of chunk_rows; refused lists (a row at n, an empty table, a null list) leave the outputs untouched."""
import ctypes as C

import numpy as np
import pytest

GATHER, DIRECT = 0, 1
FILL = 2**63


@pytest.fixture(scope="module")
def lib():
    from lab_1806_vec_db_amd import _lib as L

    return L, L.load()


def _plan(lib, n, rows, row_bytes, chunk_bytes):
    L, so = lib
    r = np.ascontiguousarray(rows, dtype=np.uint64)
    route, cr, nc = C.c_int(77), C.c_uint64(FILL), C.c_uint64(FILL)
    st = so.vdb_fetch_plan(n, r.ctypes.data_as(L.u64p) if r.size else None, r.size, row_bytes, chunk_bytes, C.byref(route), C.byref(cr), C.byref(nc))
    assert st == 0, so.vdb_last_error()
    assert so.vdb_fetch_plan(n, r.ctypes.data_as(L.u64p) if r.size else None, r.size, row_bytes, chunk_bytes, None, None, None) == 0  # nothing asked for
    return route.value, cr.value, nc.value


def _want(rows, row_bytes, chunk_bytes):
    rows = [int(x) for x in rows]
    m = len(rows)
    run = m >= 1 and all(rows[j] == rows[0] + j for j in range(m))
    cr = max(1, chunk_bytes // row_bytes)
    return (DIRECT if run else GATHER), cr, -(-m // cr)


def test_routes(lib):
    n = 1003
    run = np.arange(17, 400)
    swap = run.copy()
    swap[[100, 101]] = swap[[101, 100]]
    dup = run.copy()
    dup[200] = dup[199]
    gap = np.concatenate([run[:50], run[51:]])
    cases = {"all": np.arange(n), "run": run, "last": [n - 1], "first": [0], "empty": [], "swap": swap, "dup": dup, "gap": gap,
             "reversed": np.arange(n)[::-1], "two_down": [5, 4], "two_same": [5, 5], "two_up": [5, 6], "wrap": [5, 0, 1, 2]}
    want_route = {"all": DIRECT, "run": DIRECT, "last": DIRECT, "first": DIRECT, "empty": GATHER, "swap": GATHER, "dup": GATHER, "gap": GATHER,
                  "reversed": GATHER, "two_down": GATHER, "two_same": GATHER, "two_up": DIRECT, "wrap": GATHER}
    for name, rows in cases.items():
        got = _plan(lib, n, rows, 512, 1 << 20)
        assert got == _want(rows, 512, 1 << 20), name
        assert got[0] == want_route[name], name


def test_random_lists_against_the_restatement(lib):
    rng = np.random.default_rng(1806)
    for it in range(600):
        n = int(rng.integers(1, 301))
        m = int(rng.integers(0, 2 * n))
        kind = it % 3
        if kind == 0:
            rows = rng.integers(0, n, size=m)
        elif kind == 1:
            a = int(rng.integers(0, n))
            rows = np.arange(a, a + int(rng.integers(0, n - a + 1)))
        else:  # a run with one element disturbed
            a = int(rng.integers(0, n))
            rows = np.arange(a, n)
            if rows.size > 1:
                rows[int(rng.integers(1, rows.size))] = int(rng.integers(0, n))
        rb = int(rng.integers(1, 5000))
        cb = int(rng.integers(1, 20000))
        assert _plan(lib, n, rows, rb, cb) == _want(rows, rb, cb), (n, rows, rb, cb)


@pytest.mark.parametrize("row_bytes", [1, 12, 3840])
def test_chunk_counts(lib, row_bytes):
    n = 100000
    for chunk_bytes, cr in ((1, 1), (row_bytes, 1), (row_bytes + 1, 1 if row_bytes > 1 else 2), (7 * row_bytes, 7), (1 << 62, (1 << 62) // row_bytes)):
        for mult in (0, 1, 2, 5):
            for d in (-1, 0, 1):
                m = min(cr, 3000) * mult + d
                if m < 0 or m > 20000:
                    continue
                rows = (np.arange(m) * 7919) % n  # (no run: m >= 2 rows 7919 apart)
                got = _plan(lib, n, rows, row_bytes, chunk_bytes)
                assert got[1] == cr and got == _want(rows, row_bytes, chunk_bytes), (row_bytes, chunk_bytes, m)
                assert got[2] == (m + cr - 1) // cr
    assert _plan(lib, n, np.arange(50) * 2, row_bytes, 1)[1:] == (1, 50)  # fetch_chunk_bytes = 1: one row per chunk
    assert _plan(lib, n, np.arange(50) * 2, row_bytes, 7 * row_bytes)[1:] == (7, 8)  # 7 rows per chunk, a ragged last chunk


@pytest.mark.parametrize("n,rows,m", [(8, [1, 8], 2), (8, [8], 1), (0, [0], 1), (8, None, 3), (5, [0, 1, 2, 3, 4, 5], 6)],
                         ids=["row_at_n", "only_row_at_n", "empty_table", "null_rows", "run_past_the_end"])
def test_invalid_lists_are_refused_and_write_nothing(lib, n, rows, m):
    L, so = lib
    r = None if rows is None else np.asarray(rows, dtype=np.uint64)
    rp = None if rows is None else r.ctypes.data_as(L.u64p)
    route, cr, nc = C.c_int(77), C.c_uint64(FILL), C.c_uint64(FILL)
    st = so.vdb_fetch_plan(n, rp, m, 16, 64, C.byref(route), C.byref(cr), C.byref(nc))
    assert st == 1 and so.vdb_last_error()  # VDB_ERR_INVALID, with a message
    assert route.value == 77 and cr.value == FILL and nc.value == FILL


def test_sizes_that_do_not_fit_and_zero_arguments(lib):
    L, so = lib
    r = np.zeros(4, dtype=np.uint64)
    rp = r.ctypes.data_as(L.u64p)
    nc = C.c_uint64(FILL)
    assert so.vdb_fetch_plan(8, rp, 4, 0, 64, None, None, C.byref(nc)) == 1  # out_row_bytes = 0
    assert so.vdb_fetch_plan(8, rp, 4, 16, 0, None, None, C.byref(nc)) == 1  # chunk_bytes = 0
    assert so.vdb_fetch_plan(8, rp, 4, 2**62, 64, None, None, C.byref(nc)) == 1  # m x row bytes overflows
    assert nc.value == FILL
    assert so.vdb_fetch_plan(8, rp, 4, 2**61, 64, None, None, C.byref(nc)) == 0 and nc.value == 4  # ... and just fits
    assert so.vdb_fetch_plan(0, None, 0, 16, 64, None, None, C.byref(nc)) == 0 and nc.value == 0  # an empty list over an empty table
