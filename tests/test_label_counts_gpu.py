"""GPU: rows per value of one label column, over all rows or under a mask (vdb_index_label_counts, k_label_counts in
csrc/k_labels.hip).  The reference is numpy alone: np.count_nonzero / np.bincount over the label array (and the mask's bool array)."""
import threading

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NONE = 0xFFFFFFFF
SHAPES = (0, 1, 63, 64, 65, 255, 256, 257, 1000, 66000)  # word, workgroup and grid-stride boundaries


def _index(n, dim=4, seed=1):
    import lab_1806_vec_db_amd as vdb

    ix = vdb.GpuIndex(dim, "l2sqr")
    if n:
        ix.batch_add(np.random.default_rng(seed).random((n, dim)).astype(np.float32))
    return ix


def _want(col, codes, allow=None):
    keep = np.ones(col.shape[0], dtype=np.bool_) if allow is None else allow
    return np.array([np.count_nonzero((col == np.uint32(c)) & keep) for c in codes], dtype=np.uint64)


def _check(ix, column, col, codes, mask=None, allow=None, what=None):
    s0 = ix.get_stat("label_count_calls")
    got = ix.label_counts(column, codes, mask)
    assert got.dtype == np.uint64 and got.shape == (len(codes),)
    assert np.array_equal(got, _want(col, codes, allow)), (what, got, _want(col, codes, allow))
    assert ix.get_stat("label_count_calls") == s0 + 1


@pytest.mark.parametrize("n", SHAPES)
def test_count_shapes(n):
    rng = np.random.default_rng(300 + n)
    col = rng.integers(0, 23, size=n).astype(np.uint32) * np.uint32(5)
    col[rng.random(n) < 0.05] = NONE
    ix = _index(n)
    try:
        if n:
            ix.set_labels(6, col)
        codes = [int(c) for c in np.unique(col) if c != NONE] + [NONE, 3]  # every present code, LABEL_NONE, one absent code
        rng.shuffle(codes)
        _check(ix, 6, col, codes, what=(n, "no mask"))
        # the same total as a bincount over the dense codes
        if n:
            dense = np.bincount(col[col != NONE] // 5, minlength=23)
            got = ix.label_counts(6, [5 * v for v in range(23)])
            assert np.array_equal(got, dense.astype(np.uint64))
        # under a mask: host-built, device-built, and a combined NOT
        allow = rng.random(n) < 0.4
        hm = ix.make_mask(allow)
        _check(ix, 6, col, codes, hm, allow, (n, "host mask"))
        hm.close()
        dm = ix.make_mask_where([(6, 10)])
        _check(ix, 6, col, codes, dm, col == 10, (n, "device mask"))
        nm = ix.combine_masks("and", [dm], [True])
        _check(ix, 6, col, codes, nm, col != 10, (n, "NOT mask"))
        nm.close()
        dm.close()
        # a column never written: every row is unlabelled
        never = np.full(n, NONE, dtype=np.uint32)
        _check(ix, 11, never, [5, NONE], what=(n, "never written"))
        assert ix.label_counts(6, []).shape == (0,)
    finally:
        ix.close()


def test_1100_codes_u8_index_and_after_remove_rows():
    import lab_1806_vec_db_amd as vdb

    rng = np.random.default_rng(14)
    n = 5000
    ix = _index(n)
    try:
        col = rng.integers(0, 1100, size=n).astype(np.uint32)
        ix.set_labels(0, col)
        codes = [int(c) for c in rng.permutation(1100)]  # crosses the chunk of 1024 codes
        _check(ix, 0, col, codes, what="1100 codes")
        assert int(ix.label_counts(0, codes).sum()) == n
        allow = rng.random(n) < 0.5
        hm = ix.make_mask(allow)
        _check(ix, 0, col, codes, hm, allow, "1100 codes under a mask")
        hm.close()
        sparse = [0, 7, 1 << 31, 0xFFFFFFFE, NONE]
        col2 = np.array(sparse, dtype=np.uint32)[rng.integers(0, 5, size=n)]
        ix.set_labels(1, col2)
        _check(ix, 1, col2, sparse[::-1], what="sparse codes")
        gone = rng.choice(n, size=777, replace=False)
        dst, src = ix.remove_rows(gone)
        col[dst.astype(np.int64)] = col[src.astype(np.int64)]  # the labels move with the rows
        col = col[:n - 777].copy()
        _check(ix, 0, col, codes, what="after remove_rows")
    finally:
        ix.close()
    ux = vdb.GpuIndex(24, "l2sqr", scalar="u8")
    try:
        ux.batch_add_u8(rng.integers(0, 256, size=(700, 24), dtype=np.uint8))
        lab = rng.integers(0, 3, size=700).astype(np.uint32)
        ux.set_labels(15, lab)
        _check(ux, 15, lab, [2, NONE, 0, 1], what="u8")
        dm = ux.make_mask_where([(15, 1)])
        _check(ux, 15, lab, [2, NONE, 0, 1], dm, lab == 1, "u8 under a mask")
        dm.close()
    finally:
        ux.close()


def test_refused_calls_stale_and_foreign_masks():
    import lab_1806_vec_db_amd as vdb
    from lab_1806_vec_db_amd import _lib as L

    ix = _index(100)
    other = _index(100, seed=2)
    try:
        lab = (np.arange(100) % 4).astype(np.uint32)
        ix.set_labels(2, lab)
        s0 = ix.get_stat("label_count_calls")
        with pytest.raises(vdb.VdbError, match="error 1.*named twice"):
            ix.label_counts(2, [1, 2, 1])
        with pytest.raises(vdb.VdbError, match="error 1.*column 16"):
            ix.label_counts(16, [1])
        lib = L.load()
        out = np.full(3, 77, dtype=np.uint64)
        st = lib.vdb_index_label_counts(ix._h, 2, None, None, 3, out.ctypes.data_as(L.u64p))
        assert st == 1 and out.tolist() == [77, 77, 77]
        with pytest.raises(vdb.VdbError, match="null argument"):
            L.check(st)
        codes = np.array([1, 2, 3], dtype=np.uint32)
        st = lib.vdb_index_label_counts(ix._h, 2, None, codes.ctypes.data_as(L.u32p), 1 << 28, out.ctypes.data_as(L.u64p))
        assert st == 1 and out.tolist() == [77, 77, 77]
        with pytest.raises(vdb.VdbError, match="too many codes"):
            L.check(st)
        foreign = other.make_mask_where([])
        with pytest.raises(vdb.VdbError, match="error 1.*another index"):
            ix.label_counts(2, [1], foreign)
        foreign.close()
        mk = ix.make_mask_where([(2, 1)])
        assert ix.label_counts(2, [1, 0], mk).tolist() == [25, 0]
        s0 += 1
        ix.batch_add(np.ones((1, 4), dtype=np.float32))
        with pytest.raises(vdb.VdbError, match="error 3.*stale"):
            ix.label_counts(2, [1], mk)
        mk.close()
        assert ix.get_stat("label_count_calls") == s0
        assert ix.label_counts(2, [NONE, 3]).tolist() == [1, 25]  # the index still answers; the new row is unlabelled
    finally:
        other.close()
        ix.close()


def test_two_threads_count_at_once():
    n = 50000
    rng = np.random.default_rng(31)
    cols = {0: rng.integers(0, 200, size=n).astype(np.uint32), 1: rng.integers(0, 7, size=n).astype(np.uint32)}
    ix = _index(n)
    try:
        for c, a in cols.items():
            ix.set_labels(c, a)
        allow = rng.random(n) < 0.3
        hm = ix.make_mask(allow)
        errors = []

        def work(c):
            try:
                codes = [int(v) for v in np.unique(cols[c])] + [NONE]
                want, want_m = _want(cols[c], codes), _want(cols[c], codes, allow)
                for _ in range(10):
                    assert np.array_equal(ix.label_counts(c, codes), want)
                    assert np.array_equal(ix.label_counts(c, codes, hm), want_m)
            except BaseException as e:  # noqa: BLE001 -- reported by the main thread
                errors.append(e)

        ts = [threading.Thread(target=work, args=(c,)) for c in (0, 1, 0)]
        for t in ts:
            t.start()
        for t in ts:
            t.join()
        assert not errors, errors
        hm.close()
    finally:
        ix.close()
