"""CPU: vdb_update_plan (host utility, no GPU) against np.unique(rows // 16).

An in-place update of the rows R moves nothing; its plan is the set of 16-row mirror tiles that hold a row of R, ascending and distinct.
Checked: random lists in shuffled order, one row, every row, rows that straddle tile boundaries, tables whose size is no multiple of
16; the count-only form; refused lists (null rows, a row at n, duplicates) leave the outputs untouched."""
import ctypes as C

import numpy as np
import pytest

FILL = 0xDEADBEEF


@pytest.fixture(scope="module")
def lib():
    from lab_1806_vec_db_amd import _lib as L

    return L, L.load()


def _plan(lib, n, rows):
    L, so = lib
    r = np.ascontiguousarray(rows, dtype=np.uint64)
    tiles = np.full(len(r) + 1, FILL, dtype=np.uint32)
    nt, count = C.c_uint64(2**63), C.c_uint64(2**63)
    st = so.vdb_update_plan(n, r.ctypes.data_as(L.u64p), len(r), tiles.ctypes.data_as(L.u32p), C.byref(nt))
    assert st == 0, so.vdb_last_error()
    assert so.vdb_update_plan(n, r.ctypes.data_as(L.u64p), len(r), None, C.byref(count)) == 0
    assert count.value == nt.value  # out_tiles NULL: the count alone
    assert (tiles[nt.value:] == FILL).all()
    return tiles[: nt.value]


def _check(lib, n, rows):
    rows = np.asarray(rows, dtype=np.uint64)
    got = _plan(lib, n, rows)
    want = np.unique(rows // np.uint64(16))
    assert got.dtype == np.uint32 and np.array_equal(got.astype(np.uint64), want), (n, rows)


def test_random_lists_and_edge_shapes(lib):
    rng = np.random.default_rng(1806)
    shapes = {"random": 0, "empty": 0, "all": 0, "one": 0, "boundary": 0, "block": 0}
    for it in range(1800):
        n = int(rng.integers(1, 301))
        kind = list(shapes)[it % 6]
        if kind == "random":
            rows = rng.permutation(n)[: int(rng.integers(0, n + 1))]
        elif kind == "empty":
            rows = []
        elif kind == "all":
            rows = rng.permutation(n)
        elif kind == "one":
            rows = [int(rng.integers(0, n))]
        elif kind == "boundary":  # the rows around every tile boundary of the table
            rows = rng.permutation([r for r in range(n) if r % 16 in (15, 0, 1)])
        else:  # one contiguous block, shuffled
            a = int(rng.integers(0, n))
            rows = rng.permutation(np.arange(a, a + int(rng.integers(0, n - a + 1))))
        shapes[kind] += 1
        _check(lib, n, rows)
    assert all(v == 300 for v in shapes.values()), shapes


@pytest.mark.parametrize("n", [18, 33, 1003, 22037])
def test_straddling_rows_and_ragged_tables(lib, n):
    assert n % 16
    _check(lib, n, [17, 15, 16])  # two tiles, three rows, any order
    _check(lib, n, [n - 1])  # the ragged last tile
    _check(lib, n, [n - 1, 0])
    _check(lib, n, np.arange(n)[::-1])  # every row, descending
    assert _plan(lib, n, [17, 15, 16]).tolist() == [0, 1]
    assert _plan(lib, n, [n - 1]).tolist() == [(n - 1) // 16]


def test_empty_list_and_empty_table(lib):
    L, so = lib
    nt = C.c_uint64(5)
    assert so.vdb_update_plan(0, None, 0, None, C.byref(nt)) == 0 and nt.value == 0
    assert so.vdb_update_plan(100, None, 0, None, None) == 0  # nothing asked for, nothing written
    assert len(_plan(lib, 100, [])) == 0


@pytest.mark.parametrize("n,rows", [(8, [2, 2]), (40, [3, 17, 3]), (8, [1, 8]), (0, [0]), (5, [0, 1, 2, 3, 4, 4]), (8, None)],
                         ids=["duplicate", "duplicate_apart", "row_at_n", "empty_table", "more_rows_than_table", "null_rows"])
def test_invalid_lists_are_refused_and_write_nothing(lib, n, rows):
    L, so = lib
    r = None if rows is None else np.asarray(rows, dtype=np.uint64)
    m = 3 if rows is None else len(r)
    rp = None if rows is None else r.ctypes.data_as(L.u64p)
    tiles = np.full(m, FILL, dtype=np.uint32)
    nt = C.c_uint64(2**63)
    st = so.vdb_update_plan(n, rp, m, tiles.ctypes.data_as(L.u32p), C.byref(nt))
    assert st == 1 and so.vdb_last_error()  # VDB_ERR_INVALID, with a message
    assert (tiles == FILL).all() and nt.value == 2**63
    assert so.vdb_update_plan(n, rp, m, None, C.byref(nt)) == 1 and nt.value == 2**63
