"""GPU: the masks of many values of ONE label column from a single read of it (vdb_mask_create_partition, k_mask_partition in
csrc/k_labels.hip).  Every mask is read back (vdb_mask_rows) and compared EXACTLY -- bit words, ascending allow-list, count -- with the
mask numpy computes from the label array (np.packbits / np.flatnonzero of col == code) and with the mask vdb_mask_create_where_many
builds for the same term; the searches under a partition mask are compared with the same searches under the make_mask_where mask."""
import threading

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NONE = 0xFFFFFFFF
# the word (64 rows), workgroup (256 rows) and k_mask_scan iteration boundaries: 66 000 rows are 258 workgroups, more block counts
# than the 256 one iteration of the scan holds
SHAPES = (0, 1, 63, 64, 65, 255, 256, 257, 1000, 66000)


def _index(n, dim=4, dist="l2sqr", seed=1):
    import lab_1806_vec_db_amd as vdb

    ix = vdb.GpuIndex(dim, dist)
    if n:
        ix.batch_add(np.random.default_rng(seed).random((n, dim)).astype(np.float32))
    return ix


def _expect(col, code):
    """(words, ids) of the rows where col == code"""
    n = col.shape[0]
    ok = col == np.uint32(code)
    padded = np.zeros((n + 63) // 64 * 64, dtype=np.uint8)
    padded[:n] = ok
    return np.packbits(padded, bitorder="little").view(np.uint64), np.flatnonzero(ok).astype(np.uint32)


def _same(mk, want, what):
    words, ids = mk.rows()
    assert words.dtype == np.uint64 and ids.dtype == np.uint32
    assert np.array_equal(words, want[0]), what
    assert np.array_equal(ids, want[1]), what
    assert len(mk) == len(want[1]), what


def _close(masks):
    for mk in masks:
        mk.close()


def _check_partition(ix, column, col, codes, what):
    """the partition over `codes` equals numpy's masks and, bit for bit, make_masks_where's for the same terms"""
    s0, w0 = ix.get_stat("mask_partition_masks"), ix.get_stat("mask_where_masks")
    part = ix.make_masks_partition(column, codes)
    assert len(part) == len(codes)
    assert ix.get_stat("mask_partition_masks") == s0 + len(codes) and ix.get_stat("mask_where_masks") == w0
    where = ix.make_masks_where([[(column, int(c))] for c in codes])
    for c, pm, wm in zip(codes, part, where):
        _same(pm, _expect(col, c), (what, int(c)))
        pw, pi = pm.rows()
        ww, wi = wm.rows()
        assert np.array_equal(pw, ww) and np.array_equal(pi, wi) and len(pm) == len(wm), (what, int(c))
    _close(part)
    _close(where)


@pytest.mark.parametrize("n", SHAPES)
def test_partition_shapes(n):
    rng = np.random.default_rng(100 + n)
    G = 37
    col = rng.integers(0, G, size=n).astype(np.uint32) * np.uint32(3)  # codes 0, 3, .., 108: sparse
    col[rng.random(n) < 0.05] = NONE
    ix = _index(n)
    try:
        if n:
            ix.set_labels(4, col)
        codes = [int(c) for c in np.unique(col) if c != NONE] + [NONE, 1]  # every present code, LABEL_NONE, one absent code
        rng.shuffle(codes)
        _check_partition(ix, 4, col, codes, n)
        assert ix.make_masks_partition(4, []) == []
    finally:
        ix.close()


def test_hand_made_rows():
    n = 64 + 256 + 64 + 5  # a wave of 64 distinct codes | a workgroup of one code | a filler word | a last partial word
    col = np.empty(n, dtype=np.uint32)
    col[:64] = np.arange(64, dtype=np.uint32)[::-1] + 1000     # 64 rows, 64 distinct codes: the wave's loop runs 64 times
    col[64:320] = 7                                            # 256 rows of one code: four waves add to one block count
    col[320:384] = np.where(np.arange(64) % 2 == 0, 7, NONE)   # 7 again in another block, every other row unlabelled
    col[384:] = (7, 99999, 7, NONE, 99999)                     # code 99999 lives in the last partial word only
    ix = _index(n)
    try:
        ix.set_labels(0, col)
        codes = [int(c) for c in np.unique(col)]
        _check_partition(ix, 0, col, codes[::-1], "hand-made")
        (only,) = ix.make_masks_partition(0, [99999])
        assert only.rows()[1].tolist() == [385, 388] and int(only.rows()[0][-1]) == 0b10010
        only.close()
    finally:
        ix.close()


def test_code_lists():
    n = 3000
    rng = np.random.default_rng(8)
    ix = _index(n)
    try:
        # 1100 distinct codes in one call: crosses the chunk of 1024
        col = rng.permutation(np.arange(n, dtype=np.uint32) % 1100)
        ix.set_labels(1, col)
        codes = [int(c) for c in rng.permutation(1100)]
        _check_partition(ix, 1, col, codes, "1100 codes")
        # sparse codes
        sparse = np.array([0, 7, 1 << 31, 0xFFFFFFFE], dtype=np.uint32)
        col2 = sparse[rng.integers(0, 4, size=n)]
        col2[rng.random(n) < 0.1] = NONE
        ix.set_labels(2, col2)
        _check_partition(ix, 2, col2, [0xFFFFFFFE, 0, NONE, 1 << 31, 7, 8], "sparse")
        # a column never written: LABEL_NONE is every row, code 5 none
        never = np.full(n, NONE, dtype=np.uint32)
        _check_partition(ix, 9, never, [5, NONE], "never written")
        assert ix.get_stat("label_columns") == 2
    finally:
        ix.close()


def test_u8_index_and_columns_after_writes():
    import lab_1806_vec_db_amd as vdb

    rng = np.random.default_rng(6)
    n, dim = 700, 24
    rows = rng.integers(0, 256, size=(n, dim), dtype=np.uint8)
    ux = vdb.GpuIndex(dim, "l2sqr", scalar="u8")
    try:
        ux.batch_add_u8(rows)
        lab = rng.integers(0, 3, size=n).astype(np.uint32)
        ux.set_labels(15, lab)
        _check_partition(ux, 15, lab, [2, 0, NONE, 1], "u8")
        # the u8 range search under a partition mask returns what it returns under the make_mask_where mask
        qs = rng.integers(0, 256, size=(5, dim)).astype(np.float32)
        radius = np.float32(24 * 90.0 ** 2)
        pm = ux.make_masks_partition(15, [1, 2])[1]
        wm = ux.make_mask_where([(15, 2)])
        got, want = ux.range_search(qs, radius, mask=pm), ux.range_search(qs, radius, mask=wm)
        assert int(want[0][-1]) > 0
        for g, w in zip(got, want):
            assert np.array_equal(g, w)
        pm.close()
        wm.close()
    finally:
        ux.close()
    n = 1000
    ix = _index(n)
    try:
        col = rng.integers(0, 6, size=n).astype(np.uint32)
        ix.set_labels(3, col)
        gone = rng.choice(n, size=137, replace=False)
        dst, src = ix.remove_rows(gone)
        col[dst.astype(np.int64)] = col[src.astype(np.int64)]  # the labels move with the rows (every src lies above every dst)
        col = col[:n - 137].copy()
        assert np.array_equal(ix.get_labels(3), col)
        _check_partition(ix, 3, col, [0, 1, 2, 3, 4, 5, NONE], "after remove_rows")
        ix.batch_add(np.ones((70, 4), dtype=np.float32))  # the new rows are unlabelled
        col = np.concatenate([col, np.full(70, NONE, dtype=np.uint32)])
        assert np.array_equal(ix.get_labels(3), col)
        _check_partition(ix, 3, col, [NONE, 5, 0], "after batch_add")
    finally:
        ix.close()


def test_refused_calls():
    import lab_1806_vec_db_amd as vdb
    from lab_1806_vec_db_amd import _lib as L

    ix = _index(100)
    try:
        lab = (np.arange(100) % 4).astype(np.uint32)
        ix.set_labels(2, lab)
        s0 = ix.get_stat("mask_partition_masks")
        with pytest.raises(vdb.VdbError, match="error 1.*named twice"):
            ix.make_masks_partition(2, [1, 2, 1])
        with pytest.raises(vdb.VdbError, match="error 1.*named twice"):
            ix.make_masks_partition(2, list(range(1100)) + [3])  # the duplicate's two positions lie in different chunks
        with pytest.raises(vdb.VdbError, match="error 1.*column 16"):
            ix.make_masks_partition(16, [1])
        lib = L.load()
        codes = np.array([1, 2, 1], dtype=np.uint32)
        out = (L.vp * 3)()
        for args, msg in (((2, codes.ctypes.data_as(L.u32p), 3), "named twice"), ((16, codes.ctypes.data_as(L.u32p), 2), "column 16"),
                          ((2, None, 3), "null argument")):
            out[0] = out[1] = out[2] = 1  # (must come back NULL)
            st = lib.vdb_mask_create_partition(ix._h, args[0], args[1], args[2], out)
            assert st == 1 and all(out[j] is None for j in range(args[2])), msg
            with pytest.raises(vdb.VdbError, match=msg):
                L.check(st)
        st = lib.vdb_mask_create_partition(ix._h, 2, codes.ctypes.data_as(L.u32p), 1 << 28, out)  # refused before `out` is touched
        assert st == 1
        with pytest.raises(vdb.VdbError, match="too many codes"):
            L.check(st)
        assert lib.vdb_mask_create_partition(ix._h, 2, None, 0, None) == 0  # n_codes == 0 succeeds
        assert ix.get_stat("mask_partition_masks") == s0
        assert len(ix) == 100 and np.array_equal(ix.get_labels(2), lab)
        _check_partition(ix, 2, lab, [3, 0], "after the refused calls")  # the index still answers
    finally:
        ix.close()


def test_all_or_nothing_when_a_slab_cannot_be_allocated():
    import lab_1806_vec_db_amd as vdb
    from lab_1806_vec_db_amd import _lib as L

    n = 66000
    col = (np.arange(n) % 2).astype(np.uint32)
    ix = _index(n)
    try:
        ix.set_labels(0, col)
        _check_partition(ix, 0, col, [0, 1], "before")  # (the workspace of the call exists from here on)
        s0 = ix.get_stat("mask_partition_masks")
        lib = L.load()
        codes = np.array([0, 1], dtype=np.uint32)
        # two masks over 66 000 rows: the slab of the bit words is 2 x 8448 B, the slab of the allow-lists 264 000 B.  100 000: the words
        # are placed and the kernels have run when the lists' slab fails; 10 000: the first slab fails
        for limit in (100_000, 10_000):
            out = (L.vp * 2)()
            out[0] = out[1] = 1  # (must come back NULL)
            ix.set_param("debug_alloc_fail_over", limit)
            try:
                st = lib.vdb_mask_create_partition(ix._h, 0, codes.ctypes.data_as(L.u32p), 2, out)
            finally:
                ix.set_param("debug_alloc_fail_over", 0)
            assert st != 0 and out[0] is None and out[1] is None, limit
            with pytest.raises(vdb.VdbError, match="out of memory"):
                L.check(st)
            assert ix.get_stat("mask_partition_masks") == s0
        _check_partition(ix, 0, col, [1, 0, NONE], "after")
    finally:
        ix.close()


def test_lifetime_masks_of_one_call_die_in_any_order():
    import lab_1806_vec_db_amd as vdb

    n = 5000
    rng = np.random.default_rng(12)
    col = rng.integers(0, 40, size=n).astype(np.uint32)
    ix = _index(n)
    try:
        ix.set_labels(0, col)
        codes = list(range(40))
        masks = ix.make_masks_partition(0, codes)
        order = rng.permutation(40).tolist()
        survivor = order[-1]
        for j in order[:-1]:  # the slabs of the chunk live on with the survivor
            masks[j].close()
            _same(masks[survivor], _expect(col, codes[survivor]), ("survivor after", j))
        qs = np.zeros((2, 4), dtype=np.float32)
        ix.flat_knn_filtered(qs, 3, masks[survivor])
        ix.batch_add(np.ones((1, 4), dtype=np.float32))
        with pytest.raises(vdb.VdbError, match="error 3.*stale"):
            ix.flat_knn_filtered(qs, 3, masks[survivor])
        masks[survivor].close()
        other = _index(n + 1, seed=2)
        (mk,) = other.make_masks_partition(0, [NONE])
        assert len(mk) == n + 1
        with pytest.raises(vdb.VdbError, match="error 1.*another index"):
            ix.flat_knn_filtered(qs, 3, mk)
        mk.close()
        other.close()
    finally:
        ix.close()


def _same_knn(a, b, what):
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32)) and np.array_equal(a[2], b[2]), what


def test_search_under_a_partition_mask_direct_path_and_combine():
    n = 1000
    rng = np.random.default_rng(5)
    col = rng.integers(0, 5, size=n).astype(np.uint32)
    col[rng.random(n) < 0.1] = NONE
    ix = _index(n)
    try:
        ix.set_labels(2, col)
        qs = np.random.default_rng(3).random((9, 4)).astype(np.float32)
        codes = [3, 1, NONE, 9]
        part = ix.make_masks_partition(2, codes)
        for c, pm in zip(codes, part):
            wm = ix.make_mask_where([(2, c)])
            for k in (1, 10, 300):
                _same_knn(ix.flat_knn_filtered(qs, k, pm), ix.flat_knn_filtered(qs, k, wm), (c, k))
            for got, want in zip(ix.range_search(qs, 0.3, mask=pm), ix.range_search(qs, 0.3, mask=wm)):
                assert np.array_equal(got, want), c
            wm.close()
        both = ix.combine_masks("or", [part[0], part[2]])
        ok = (col == 3) | (col == NONE)
        assert np.array_equal(both.rows()[1], np.flatnonzero(ok).astype(np.uint32)) and len(both) == int(ok.sum())
        padded = np.zeros((n + 63) // 64 * 64, dtype=np.uint8)
        padded[:n] = ok
        assert np.array_equal(both.rows()[0], np.packbits(padded, bitorder="little").view(np.uint64))
        both.close()
        _close(part)
    finally:
        ix.close()


def test_search_under_a_partition_mask_8bit_tier():
    """the 8-bit tier reads the mask's bit words (through the lazily built masked row constants) where the direct path reads its list"""
    from conftest import gist_like

    n, dim = 20000, 128
    base = gist_like(n, dim=dim, seed=77)
    ix = _index(0, dim=dim)
    try:
        ix.batch_add(base)
        half = (np.random.default_rng(4).random(n) < 0.5).astype(np.uint32)  # about half the rows: past flat_filtered_direct_max
        ix.set_labels(0, half)
        ix.set_flat_mode(2)
        qs = gist_like(40, dim=dim, seed=78)
        pm = ix.make_masks_partition(0, [0, 1])[1]
        wm = ix.make_mask_where([(0, 1)])
        assert len(pm) == len(wm) == int(half.sum()) > 8192
        s0 = ix.get_stat("flat_filtered_i8_queries")
        got = ix.flat_knn_filtered(qs, 10, pm)
        assert ix.get_stat("flat_filtered_i8_queries") == s0 + len(qs)
        _same_knn(got, ix.flat_knn_filtered(qs, 10, wm), "8-bit tier")
        assert bool((half[got[0].astype(np.int64)] == 1).all())
        pm.close()
        wm.close()
    finally:
        ix.close()


def test_two_threads_partition_different_columns():
    n = 20000
    rng = np.random.default_rng(21)
    cols = {0: rng.integers(0, 50, size=n).astype(np.uint32), 1: rng.integers(0, 9, size=n).astype(np.uint32)}
    ix = _index(n)
    try:
        for c, a in cols.items():
            ix.set_labels(c, a)
        s0 = ix.get_stat("mask_partition_masks")
        errors = []

        def work(c):
            try:
                codes = [int(v) for v in np.unique(cols[c])] + [NONE]
                for _ in range(5):
                    part = ix.make_masks_partition(c, codes)
                    for code, mk in zip(codes, part):
                        _same(mk, _expect(cols[c], code), (c, code))
                    _close(part)
            except BaseException as e:  # noqa: BLE001 -- reported by the main thread
                errors.append(e)

        ts = [threading.Thread(target=work, args=(c,)) for c in cols]
        for t in ts:
            t.start()
        for t in ts:
            t.join()
        assert not errors, errors
        assert ix.get_stat("mask_partition_masks") == s0 + 5 * (51 + 10)
    finally:
        ix.close()
