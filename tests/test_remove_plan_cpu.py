"""CPU: vdb_remove_plan (host utility, no GPU) against the naive replay of swap_remove in descending order.

Removing the rows R from a table of n rows is DEFINED as VecSet::swap_remove on them in descending order (MetadataVecTable::delete);
the plan is that sequence's net effect as moves (dst, src).  Checked: the state the moves produce equals the replay's for every
subset of n <= 8 and a few thousand random (n, R) with n <= 300 (the edge shapes named below included); src >= n' > dst, src not in
R, move count = |R below n'|, dst descending; refused lists leave the outputs untouched."""
import ctypes as C
import itertools

import numpy as np
import pytest


@pytest.fixture(scope="module")
def lib():
    from lab_1806_vec_db_amd import _lib as L

    return L, L.load()


def _naive(n, rows):
    cur = list(range(n))
    for i in sorted(rows, reverse=True):
        cur[i] = cur[-1]
        cur.pop()
    return cur


def _plan(lib, n, rows, fill=2**63):
    L, so = lib
    r = np.asarray(sorted(rows), dtype=np.uint64)
    dst = np.full(max(len(r), 1), fill, dtype=np.uint64)
    src = np.full(max(len(r), 1), fill, dtype=np.uint64)
    moves, count = C.c_uint64(fill), C.c_uint64(fill)
    st = so.vdb_remove_plan(n, r.ctypes.data_as(L.u64p), len(r), dst.ctypes.data_as(L.u64p), src.ctypes.data_as(L.u64p), C.byref(moves))
    assert st == 0, so.vdb_last_error()
    assert so.vdb_remove_plan(n, r.ctypes.data_as(L.u64p), len(r), None, None, C.byref(count)) == 0
    assert count.value == moves.value  # both outputs NULL: the count alone
    assert (dst[moves.value:] == fill).all() and (src[moves.value:] == fill).all()
    return dst[: moves.value].tolist(), src[: moves.value].tolist()


def _check(lib, n, rows):
    rows = sorted(rows)
    n1 = n - len(rows)
    dst, src = _plan(lib, n, rows)
    rs = set(rows)
    assert len(dst) == sum(1 for r in rows if r < n1), (n, rows)
    assert all(s >= n1 > d for d, s in zip(dst, src)), (n, rows, dst, src)
    assert all(s < n and s not in rs for s in src), (n, rows, src)
    assert dst == sorted(dst, reverse=True) and len(set(dst)) == len(dst) and len(set(src)) == len(src)
    cur = list(range(n))
    for d, s in zip(dst, src):
        cur[d] = s  # sources are never destinations: any order gives the same state
    assert cur[:n1] == _naive(n, rows), (n, rows)


def test_every_subset_of_small_tables(lib):
    for n in range(9):
        for m in range(n + 1):
            for rows in itertools.combinations(range(n), m):
                _check(lib, n, rows)


def test_random_tables_and_edge_shapes(lib):
    rng = np.random.default_rng(1806)
    shapes = {"random": 0, "empty": 0, "all": 0, "tail": 0, "below": 0, "block": 0}
    for it in range(3000):
        n = int(rng.integers(0, 301))
        kind = list(shapes)[it % 6]
        m = int(rng.integers(0, n + 1))
        if kind == "random":
            rows = rng.permutation(n)[:m].tolist()
        elif kind == "empty":
            rows = []
        elif kind == "all":
            rows = list(range(n))
        elif kind == "tail":  # entirely inside the old tail [n', n)
            rows = list(range(n - m // 2, n))
        elif kind == "below":  # entirely below n'
            m = min(m, n // 2)
            rows = rng.permutation(n - m)[:m].tolist()
        else:  # one contiguous block
            a = int(rng.integers(0, n + 1))
            rows = list(range(a, a + int(rng.integers(0, n - a + 1))))
        n1 = n - len(rows)
        if kind == "tail":
            assert all(r >= n1 for r in rows)
        if kind == "below":
            assert all(r < n1 for r in rows)
        shapes[kind] += 1
        _check(lib, n, rows)
    assert all(v >= 400 for v in shapes.values()), shapes


@pytest.mark.parametrize("n,rows", [(8, [3, 1]), (8, [2, 2]), (8, [1, 8]), (0, [0]), (5, [0, 1, 2, 3, 4, 4])],
                         ids=["unsorted", "duplicate", "out_of_range", "empty_table", "more_rows_than_table"])
def test_invalid_lists_are_refused_and_write_nothing(lib, n, rows):
    L, so = lib
    r = np.asarray(rows, dtype=np.uint64)
    fill = 2**63
    dst = np.full(len(r), fill, dtype=np.uint64)
    src = np.full(len(r), fill, dtype=np.uint64)
    moves = C.c_uint64(fill)
    st = so.vdb_remove_plan(n, r.ctypes.data_as(L.u64p), len(r), dst.ctypes.data_as(L.u64p), src.ctypes.data_as(L.u64p), C.byref(moves))
    assert st == 1 and so.vdb_last_error()  # VDB_ERR_INVALID, with a message
    assert (dst == fill).all() and (src == fill).all() and moves.value == fill
    assert so.vdb_remove_plan(n, r.ctypes.data_as(L.u64p), len(r), None, None, C.byref(moves)) == 1 and moves.value == fill


def test_python_wrapper(lib):
    import lab_1806_vec_db_amd as vdb

    dst, src = vdb.remove_plan(10, [1, 8])
    assert dst.tolist() == [1] and src.tolist() == [9] and dst.dtype == np.uint64
    with pytest.raises(vdb.VdbError):
        vdb.remove_plan(10, [8, 1])
