"""GPU: from a list of codes of ONE label column to rows (vdb_index_label_lookup; k_label_lookup / k_label_lookup_direct in
csrc/k_lookup.hip): per code the number of rows that carry it and the lowest such row.  The reference is numpy on the column array the
test keeps -- np.flatnonzero(col == c) gives first and count -- and every comparison is exact.  Every case runs on both routes: the
sorted one is forced by label_lookup_table_bytes = 0, the direct one by filling the list up with dense absent codes to more than 1024;
the routes must equal each other and numpy, and the counters must agree with vdb_label_lookup_plan."""
import ctypes as C
import threading

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NONE = 0xFFFFFFFF
ROW_NONE = 2**64 - 1
SORTED, DIRECT = 0, 1
MIB64 = 64 << 20
STATS = ("label_lookup_calls", "label_lookup_codes", "label_lookup_direct", "label_lookup_passes")


def _index(n, dim=4, seed=1, scalar="f32"):
    import lab_1806_vec_db_amd as vdb

    ix = vdb.GpuIndex(dim, "l2sqr", scalar=scalar)
    if n and scalar == "u8":
        ix.batch_add_u8(np.random.default_rng(seed).integers(0, 256, size=(n, dim)).astype(np.uint8))
    elif n:
        ix.batch_add(np.random.default_rng(seed).random((n, dim)).astype(np.float32))
    return ix


def _expect(col, codes):
    first = np.full(len(codes), ROW_NONE, dtype=np.uint64)
    counts = np.zeros(len(codes), dtype=np.uint64)
    for j, c in enumerate(codes):
        rows = np.flatnonzero(col == np.uint32(int(c)))
        if rows.size:
            first[j], counts[j] = rows[0], rows.size
    return first, counts


def _lookup(ix, column, col, codes, table_bytes, route, what):
    """one call under `table_bytes`: equal to numpy, on the route asked for, the counters moved as the plan says"""
    codes = [int(c) for c in codes]
    ix.set_param("label_lookup_table_bytes", table_bytes)
    plan = ix.label_lookup_plan(column, codes, table_bytes)
    assert plan[0] == route, (what, plan)
    before = [ix.get_stat(s) for s in STATS]
    first, counts = ix.label_lookup(column, codes)
    ran = bool(len(codes) and col.shape[0])
    assert [ix.get_stat(s) for s in STATS] == [before[0] + 1, before[1] + len(codes), before[2] + (ran and route == DIRECT), before[3] + (plan[3] if ran else 0)], what
    assert first.dtype == np.uint64 and counts.dtype == np.uint64
    want = _expect(col, codes)
    assert np.array_equal(counts, want[1]), what
    assert np.array_equal(first, want[0]), what
    return first, counts


def _both(ix, column, col, codes, what):
    """the sorted route over `codes`, then the direct route: the codes in clusters of a span the table cap allows, each filled up with dense
    absent codes to more than 1024 (LABEL_NONE rides with the first cluster); the answers per code must be the sorted route's"""
    codes = [int(c) for c in codes]
    want = dict(zip(codes, zip(*[a.tolist() for a in _lookup(ix, column, col, codes, 0, SORTED, (what, "sorted"))])))
    real = sorted(c for c in codes if c != NONE)
    clusters = []
    for c in real:
        if clusters and c - clusters[-1][0] < (1 << 20):
            clusters[-1].append(c)
        else:
            clusters.append([c])
    if not clusters:
        clusters = [[]]
    rng = np.random.default_rng(len(codes))
    for ci, cl in enumerate(clusters):
        taken = set(cl)
        lo = min(cl[0], 0xFFFFFFFE - 4000) if cl else 0
        fill = [c for c in range(lo, lo + 4000) if c not in taken][: max(1025 - len(cl), 0) + 1]
        lst = cl + fill + ([NONE] if ci == 0 and NONE in codes else [])
        lst = [lst[i] for i in rng.permutation(len(lst))]
        first, counts = _lookup(ix, column, col, lst, MIB64, DIRECT, (what, "direct", ci))
        for c, f, k in zip(lst, first.tolist(), counts.tolist()):
            if c in want:
                assert (f, k) == want[c], (what, c)


@pytest.mark.parametrize("n", (0, 1, 63, 64, 65, 255, 256, 257))
def test_row_counts(n):
    rng = np.random.default_rng(100 + n)
    col = rng.integers(0, 37, size=n).astype(np.uint32) * np.uint32(3)  # codes 0, 3, .., 108: sparse
    col[rng.random(n) < 0.1] = NONE
    ix = _index(n)
    try:
        if n:
            ix.set_labels(4, col)
        codes = [int(c) for c in np.unique(col) if c != NONE] + [NONE, 1]  # every present code, LABEL_NONE, one absent code
        rng.shuffle(codes)
        _both(ix, 4, col, codes, n)
        first, counts = ix.label_lookup(4, [])
        assert first.shape == (0,) and counts.shape == (0,)
    finally:
        ix.close()


def test_grid_stride_wraps():
    n = 4097  # 65 words over ONE workgroup of four waves: 17 trips, the last one a single partial word
    rng = np.random.default_rng(5)
    ix = _index(n)
    try:
        ix.set_param("label_lookup_max_blocks", 1)
        unique = rng.permutation(n).astype(np.uint32)
        ix.set_labels(0, unique)
        codes = rng.permutation(n + 3)  # every row's code and three absent ones
        _lookup(ix, 0, unique, codes, 0, SORTED, "unique, sorted")
        _lookup(ix, 0, unique, codes, MIB64, DIRECT, "unique, direct")
        few = (rng.integers(0, 5, size=n) * 1000).astype(np.uint32)
        ix.set_labels(1, few)
        _both(ix, 1, few, [4000, 0, 2000, NONE, 1000, 3000, 17], "five codes")
    finally:
        ix.close()


def test_hand_made_columns():
    n = 64 + 256 + 64 + 64 + 5
    ix = _index(n)
    try:
        # one code in every row: a wave makes one add and one min
        same = np.full(n, 7, dtype=np.uint32)
        ix.set_labels(0, same)
        _both(ix, 0, same, [7, 8, NONE], "one code")
        # 64 distinct codes in one wave | a workgroup of one code | rows without a value | first carriers at lane 63 and at lane 0 of the next word
        col = np.empty(n, dtype=np.uint32)
        col[:64] = np.arange(64, dtype=np.uint32)[::-1] + 1000
        col[64:320] = 7
        col[320:384] = np.where(np.arange(64) % 2 == 0, 7, NONE)
        col[384:448] = 7
        col[447] = 555          # lane 63 of word 6 is the first row of 555 ...
        col[448:] = (666, 555, 7, NONE, 666)  # ... and lane 0 of word 7 the first of 666
        ix.set_labels(1, col)
        first, counts = _lookup(ix, 1, col, [555, 666, 7, NONE, 1063, 1000], 0, SORTED, "hand-made")
        assert first.tolist() == [447, 448, 64, 321, 0, 63] and counts.tolist() == [2, 2, 256 + 32 + 63 + 1, 33, 1, 1]
        _both(ix, 1, col, [int(c) for c in np.unique(col)] + [5], "hand-made")
        # a column never written: every row is unlabelled, without a load
        never = np.full(n, NONE, dtype=np.uint32)
        first, counts = _lookup(ix, 9, never, [5, NONE], 0, SORTED, "never written")
        assert first.tolist() == [ROW_NONE, 0] and counts.tolist() == [0, n]
        _both(ix, 9, never, [5, NONE, 0], "never written")
        assert ix.get_stat("label_columns") == 2
    finally:
        ix.close()


def test_code_lists():
    n = 3000
    rng = np.random.default_rng(8)
    ix = _index(n)
    try:
        sparse = np.array([0, 7, 1 << 31, 0xFFFFFFFE], dtype=np.uint32)
        col = sparse[rng.integers(0, 4, size=n)]
        col[rng.random(n) < 0.1] = NONE
        ix.set_labels(2, col)
        _both(ix, 2, col, [0xFFFFFFFE, 0, NONE, 1 << 31, 7, 8, 0xFFFFFFFD], "sparse")
        many = rng.integers(0, 3500, size=n).astype(np.uint32)  # codes with one, several and no rows
        many[rng.random(n) < 0.05] = NONE
        ix.set_labels(3, many)
        for size in (1, 1023, 1024, 1025, 3000):
            codes = rng.permutation(4000)[:size].tolist()
            if size == 1024:
                codes[17] = NONE
            _both(ix, 3, many, codes, size)
        _lookup(ix, 3, many, rng.permutation(4000)[:3000], MIB64, DIRECT, "3000 codes, direct as they are")
        _lookup(ix, 3, many, rng.permutation(4000)[:3000], 4 * 3000, SORTED, "3000 codes under a small cap")
    finally:
        ix.close()


def test_u8_index_and_after_writes():
    n = 700
    rng = np.random.default_rng(9)
    ix = _index(n, scalar="u8")
    try:
        col = rng.integers(0, 50, size=n).astype(np.uint32)
        ix.set_labels(0, col)
        _both(ix, 0, col, list(range(52)) + [NONE], "u8")
    finally:
        ix.close()
    ix = _index(n)
    try:
        col = rng.permutation(n).astype(np.uint32)
        ix.set_labels(0, col)
        gone = rng.choice(n, size=90, replace=False)
        dst, src = ix.remove_rows(gone)
        col[dst.astype(np.int64)] = col[src.astype(np.int64)]
        col = col[: n - 90].copy()
        _both(ix, 0, col, rng.permutation(n), "after remove_rows")
        ix.batch_add(rng.random((133, 4)).astype(np.float32))  # the new rows are unlabelled
        col = np.concatenate([col, np.full(133, NONE, dtype=np.uint32)])
        _both(ix, 0, col, rng.permutation(n).tolist() + [NONE], "after batch_add")
        rows = rng.choice(col.shape[0], size=200, replace=False)
        new = rng.integers(0, 40, size=200).astype(np.uint32)  # now many rows share a code, and some codes lose their row
        ix.set_labels_rows(rows, [0], new)
        col[rows] = new
        _both(ix, 0, col, rng.permutation(n).tolist() + [NONE], "after set_labels_rows")
    finally:
        ix.close()


def test_refusals_change_nothing():
    import lab_1806_vec_db_amd._lib as L

    n = 300
    ix = _index(n)
    try:
        col = (np.arange(n) % 9).astype(np.uint32)
        ix.set_labels(0, col)
        ix.label_lookup(0, [1, 2])
        stats = STATS + ("label_count_calls", "label_columns", "mask_where_masks", "mask_partition_masks")
        before = [ix.get_stat(s) for s in stats]
        dense_dup = np.arange(2000, dtype=np.uint32)
        dense_dup[1999] = 3
        cases = [(16, np.array([1, 2], np.uint32), 2, True, True), (0, np.array([4, 4], np.uint32), 2, True, True),
                 (0, np.array([NONE, 1, NONE], np.uint32), 3, True, True), (0, dense_dup, 2000, True, True), (0, None, 3, True, True),
                 (0, np.array([1, 2, 3], np.uint32), 3, False, True), (0, np.array([1, 2, 3], np.uint32), 3, True, False)]
        for column, codes, m, with_first, with_counts in cases:
            first = np.full(m, 0xABCDEF, dtype=np.uint64)
            counts = np.full(m, 0xFEDCBA, dtype=np.uint64)
            st = ix._lib.vdb_index_label_lookup(ix._h, column, None if codes is None else codes.ctypes.data_as(L.u32p), m,
                                                first.ctypes.data_as(L.u64p) if with_first else None, counts.ctypes.data_as(L.u64p) if with_counts else None)
            assert st == 1, (column, m)
            assert (first == 0xABCDEF).all() and (counts == 0xFEDCBA).all(), (column, m)
            assert [ix.get_stat(s) for s in stats] == before, (column, m)
        with pytest.raises(L.VdbError, match="twice"):
            ix.label_lookup(0, [4, 4])
        # no codes: no pointer is needed, and the call counts
        assert ix._lib.vdb_index_label_lookup(ix._h, 0, None, 0, None, None) == 0
        assert ix.get_stat("label_lookup_calls") == before[0] + 1 and ix.get_stat("label_lookup_passes") == before[3]
    finally:
        ix.close()


def test_two_threads_on_one_handle():
    n = 5000
    rng = np.random.default_rng(11)
    ix = _index(n)
    try:
        col = rng.integers(0, 2000, size=n).astype(np.uint32)
        ix.set_labels(0, col)
        lists = [rng.permutation(2100)[:1500].tolist(), rng.permutation(2100)[:700].tolist() + [NONE]]  # one direct, one sorted
        assert [ix.label_lookup_plan(0, c)[0] for c in lists] == [DIRECT, SORTED]
        wants = [_expect(col, c) for c in lists]
        bad = []

        def work(t):
            try:
                for _ in range(8):
                    first, counts = ix.label_lookup(0, lists[t])
                    if not (np.array_equal(first, wants[t][0]) and np.array_equal(counts, wants[t][1])):
                        bad.append(t)
            except Exception as e:  # noqa: BLE001
                bad.append(repr(e))

        ts = [threading.Thread(target=work, args=(t,)) for t in range(2)]
        for t in ts:
            t.start()
        for t in ts:
            t.join()
        assert not bad
        assert ix.get_stat("label_lookup_calls") == 16 and ix.get_stat("label_lookup_direct") == 8 and ix.get_stat("label_lookup_passes") == 16
    finally:
        ix.close()
