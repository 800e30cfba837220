"""CPU: vdb_labels_scatter_plan (host utility, no GPU) against numpy.

A scattered label write names m distinct rows below n and 1 .. 16 distinct columns below 16; the plan is that check plus the ids narrowed
to u32 for the upload.  Checked: random valid lists (ids equal to the rows, in their order), out_ids32 = NULL, n = 0, m = 0 with and
without columns, and every refusal -- a row at n, a duplicate row, a column at 16, a column named twice, no column with rows, 17 columns,
a NULL array with m > 0 -- with out_ids32 untouched behind a sentinel."""
import ctypes as C

import numpy as np
import pytest

FILL = 0xA5A5A5A5
COLS = 16


@pytest.fixture(scope="module")
def lib():
    from lab_1806_vec_db_amd import _lib as L

    return L, L.load()


def _call(lib, n, rows, columns, out="fill", m=None, n_cols=None):
    """(status, out array or None); rows / columns None: a NULL pointer"""
    L, so = lib
    r = None if rows is None else np.ascontiguousarray(rows, dtype=np.uint64)
    c = None if columns is None else np.ascontiguousarray(columns, dtype=np.uint32)
    m = (0 if r is None else r.size) if m is None else m
    n_cols = (0 if c is None else c.size) if n_cols is None else n_cols
    o = None if out is None else np.full(m + 3, FILL, dtype=np.uint32)
    st = so.vdb_labels_scatter_plan(n, None if r is None else r.ctypes.data_as(L.u64p), m, None if c is None else c.ctypes.data_as(L.u32p), n_cols,
                                    None if o is None else o.ctypes.data_as(L.u32p))
    return st, o


def test_random_lists_against_numpy(lib):
    rng = np.random.default_rng(1806)
    for it in range(400):
        n = int(rng.integers(1, 400))
        m = int(rng.integers(0, n + 1))
        rows = rng.permutation(n)[:m]
        cols = rng.permutation(COLS)[:int(rng.integers(1, COLS + 1))]
        st, o = _call(lib, n, rows, cols)
        assert st == 0, lib[1].vdb_last_error()
        assert np.array_equal(o[:m], rows.astype(np.uint32)) and (o[m:] == FILL).all(), (n, m)
        assert _call(lib, n, rows, cols, out=None)[0] == 0  # check only


def test_large_ids_are_narrowed_exactly(lib):
    n = 2 ** 32
    rows = np.array([2 ** 32 - 1, 0, 2 ** 31, 2 ** 31 - 1, 12345678901 % n], dtype=np.uint64)
    st, o = _call(lib, n, rows, [3])
    assert st == 0 and o[:5].tolist() == [int(x) for x in rows]
    assert _call(lib, 2 ** 32 + 1, rows, [3])[0] == 1  # more rows than a shard holds
    # (a short list over a large table: the row check sorts the list instead of marking a bitmap over the table)
    st, o = _call(lib, n, [2 ** 31, 7, 2 ** 31], [3])
    assert st == 1 and (o == FILL).all()
    st, o = _call(lib, n, [7, n], [3])
    assert st == 1 and (o == FILL).all()


def test_empty_calls(lib):
    assert _call(lib, 0, [], [0])[0] == 0  # an empty table, nothing listed
    assert _call(lib, 0, None, None)[0] == 0  # ... not even arrays
    assert _call(lib, 10, [], [])[0] == 0  # m == 0 needs no column
    assert _call(lib, 10, None, [5, 2], m=0)[0] == 0
    st, o = _call(lib, 0, [0], [0])  # any row of an empty table is out of bounds
    assert st == 1 and (o == FILL).all()


@pytest.mark.parametrize("n,rows,cols,kw", [
    (8, [1, 8], [0], {}),
    (8, [3, 5, 3], [0], {}),
    (8, [1, 2], [16], {}),
    (8, [1, 2], [0, 15, 16], {}),
    (8, [1, 2], [4, 7, 4], {}),
    (8, [1, 2], [], {}),
    (8, [1, 2], list(range(16)) + [0], {}),
    (8, [1, 2], np.arange(17) % 16, {}),
    (8, None, [0], {"m": 2}),
    (8, [1, 2], None, {"n_cols": 1}),
    (8, np.arange(9) % 8, [0], {}),
], ids=["row_at_n", "duplicate_row", "column_16", "column_16_last", "column_twice", "no_column", "17_columns", "17_columns_wrapped", "null_rows",
        "null_columns", "more_rows_than_n"])
def test_refusals_write_nothing(lib, n, rows, cols, kw):
    st, o = _call(lib, n, rows, cols, **kw)
    assert st == 1 and lib[1].vdb_last_error()  # VDB_ERR_INVALID, with a message
    assert (o == FILL).all()
    assert _call(lib, n, rows, cols, out=None, **kw)[0] == 1
