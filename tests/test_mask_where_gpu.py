"""GPU: row masks built on the device from label columns (vdb_mask_create_where / _many, csrc/k_labels.hip).  Every mask is read back
(vdb_mask_rows) and compared EXACTLY -- bit words and ascending allow-list -- with the mask numpy computes from the label arrays; the
searches under a device-built mask are compared with the same searches under vdb_mask_create's mask of the same rows."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NONE = 0xFFFFFFFF
# 300 001 rows: 4688 words in 1172 workgroups -- more block counts than one iteration of the scan holds (256) and a ragged last word (33
# rows); 300 101 rows add a ragged last workgroup (2 of its 4 words).  65 and 257 rows: a second word / a second workgroup of one word.
SHAPES = (0, 1, 63, 64, 65, 255, 256, 257, 1000, 300001, 300101)


def _labels(n, seed=5):
    """two columns: about 5 and about 3 distinct codes, some rows unlabelled"""
    rng = np.random.default_rng(seed + n)
    a = rng.integers(0, 5, size=n).astype(np.uint32)
    b = rng.integers(0, 3, size=n).astype(np.uint32)
    a[rng.random(n) < 0.1] = NONE
    b[rng.random(n) < 0.2] = NONE
    return a, b


def _expect(n, cols, terms):
    """(words, ids) of the rows where cols[c] == code for every term; a column the dict lacks reads NONE"""
    ok = np.ones(n, dtype=np.bool_)
    for c, code in terms:
        ok &= cols.get(c, np.full(n, NONE, dtype=np.uint32)) == np.uint32(code)
    padded = np.zeros((n + 63) // 64 * 64, dtype=np.uint8)
    padded[:n] = ok
    return np.packbits(padded, bitorder="little").view(np.uint64), np.flatnonzero(ok).astype(np.uint32)


def _index(n, dim=4, dist="l2sqr", seed=1):
    import lab_1806_vec_db_amd as vdb

    ix = vdb.GpuIndex(dim, dist)
    if n:
        ix.batch_add(np.random.default_rng(seed).random((n, dim)).astype(np.float32))
    return ix


def _labelled(n):
    """an index of n rows with columns 2 and 7 written (5 never), and the numpy twin of the columns"""
    ix = _index(n)
    a, b = _labels(n)
    if n:
        ix.set_labels(2, a)
        ix.set_labels(7, b)
    return ix, {2: a, 7: b}


def _same(mk, want, what):
    words, ids = mk.rows()
    assert words.dtype == np.uint64 and ids.dtype == np.uint32
    assert np.array_equal(words, want[0]), what
    assert np.array_equal(ids, want[1]), what
    assert len(mk) == len(want[1]), what


TERM_LISTS = (
    [],                                   # every row
    [(2, 3)], [(7, 0)],                   # one term
    [(2, 1), (7, 2)], [(7, 1), (2, 4)],   # two terms
    [(2, NONE)], [(2, 0), (7, NONE)],     # unlabelled rows
    [(5, NONE)], [(5, 0)], [(2, 2), (5, NONE)],  # a column never written: NONE everywhere
    [(2, 1), (2, 3)],                     # conflicting terms on one column: empty
    [(2, 9)],                             # a code no row carries
    [(2, 1), (7, 2), (5, NONE), (2, 1), (7, 2), (5, NONE), (2, 1), (7, 2)],  # all 8 terms
)


@pytest.mark.parametrize("n", SHAPES)
def test_mask_shapes(n):
    ix, cols = _labelled(n)
    try:
        s0 = ix.get_stat("mask_where_masks")
        for terms in TERM_LISTS:
            mk = ix.make_mask_where(terms)
            _same(mk, _expect(n, cols, terms), (n, terms))
            mk.close()
        assert ix.get_stat("mask_where_masks") == s0 + len(TERM_LISTS)
        # the same object vdb_mask_create makes: its read-back goes through the same call
        allow = cols[2] == 3 if n else np.zeros(0, dtype=np.bool_)
        hm = ix.make_mask(allow)
        _same(hm, _expect(n, cols, [(2, 3)]), (n, "host mask"))
        hm.close()
    finally:
        ix.close()


def test_many_form_equals_the_singles():
    n = 1000
    ix, cols = _labelled(n)
    try:
        rng = np.random.default_rng(9)
        lists = []
        for g in range(1100):  # more than one chunk of 1024
            pick = g % 11
            if pick == 0:
                lists.append([])  # full
            elif pick == 1:
                lists.append([(2, 1), (2, 2)])  # empty
            elif pick == 2:
                lists.append([(2, 4), (7, 1)])  # duplicates of one another
            else:
                lists.append([(int(rng.choice((2, 5, 7))), int(rng.choice((0, 1, 2, 3, 4, NONE)))) for _ in range(int(rng.integers(1, 4)))])
        s0 = ix.get_stat("mask_where_masks")
        many = ix.make_masks_where(lists)
        assert len(many) == 1100 and ix.get_stat("mask_where_masks") == s0 + 1100
        singles = {}
        for g, (terms, mk) in enumerate(zip(lists, many)):
            _same(mk, _expect(n, cols, terms), (g, terms))
            key = tuple(terms)
            if key not in singles:  # the single form, once per distinct list
                one = ix.make_mask_where(terms)
                singles[key] = one.rows()
                one.close()
            w, i = mk.rows()
            assert np.array_equal(w, singles[key][0]) and np.array_equal(i, singles[key][1]), g
        for mk in many:
            mk.close()
        assert ix.make_masks_where([]) == []
    finally:
        ix.close()


def test_many_form_is_all_or_nothing():
    import lab_1806_vec_db_amd as vdb

    ix, cols = _labelled(1000)
    try:
        s0 = ix.get_stat("mask_where_masks")
        lists = [[(2, 1)]] * 1030 + [[(7, 0), (16, 0)]]  # the invalid column comes last, in the second chunk
        with pytest.raises(vdb.VdbError, match="error 1.*column 16"):
            ix.make_masks_where(lists)
        assert ix.get_stat("mask_where_masks") == s0
        assert len(ix) == 1000 and np.array_equal(ix.get_labels(2), cols[2])
        mk = ix.make_mask_where([(2, 1)])  # the index still answers
        _same(mk, _expect(1000, cols, [(2, 1)]), "after the refused call")
        mk.close()
    finally:
        ix.close()


def _same_knn(a, b, what):
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32)) and np.array_equal(a[2], b[2]), what


def test_search_under_a_device_built_mask_direct_path():
    n = 1000
    ix, cols = _labelled(n)
    try:
        qs = np.random.default_rng(3).random((9, 4)).astype(np.float32)
        for terms in ([(2, 3)], [(2, 1), (7, 2)], [], [(2, 9)]):
            dm = ix.make_mask_where(terms)
            hm = ix.make_mask(_expect(n, cols, terms)[1])
            for k in (1, 10, 300):
                _same_knn(ix.flat_knn_filtered(qs, k, dm), ix.flat_knn_filtered(qs, k, hm), (terms, k))
            for got, want in zip(ix.range_search(qs, 0.3, mask=dm), ix.range_search(qs, 0.3, mask=hm)):
                assert np.array_equal(got, want), terms
            dm.close()
            hm.close()
    finally:
        ix.close()


def test_search_under_a_device_built_mask_8bit_tier():
    """the 8-bit tier reads the mask's bit words (through the masked row constants) where the direct path reads its allow-list"""
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
        dm = ix.make_mask_where([(0, 1)])
        hm = ix.make_mask(half == 1)
        assert len(dm) == len(hm) == int(half.sum()) > 8192
        s0 = ix.get_stat("flat_filtered_i8_queries")
        got = ix.flat_knn_filtered(qs, 10, dm)
        assert ix.get_stat("flat_filtered_i8_queries") == s0 + len(qs)
        _same_knn(got, ix.flat_knn_filtered(qs, 10, hm), "8-bit tier")
        assert ix.get_stat("flat_filtered_i8_queries") == s0 + 2 * len(qs)
        assert bool((half[got[0].astype(np.int64)] == 1).all())
        dm.close()
        hm.close()
    finally:
        ix.close()


def test_range_search_under_a_device_built_mask_u8_index():
    import lab_1806_vec_db_amd as vdb

    n, dim = 700, 24
    rng = np.random.default_rng(6)
    rows = rng.integers(0, 256, size=(n, dim), dtype=np.uint8)
    ix = vdb.GpuIndex(dim, "l2sqr", scalar="u8")
    try:
        ix.batch_add_u8(rows)
        lab = rng.integers(0, 3, size=n).astype(np.uint32)
        ix.set_labels(15, lab)
        assert np.array_equal(ix.get_labels(15), lab)
        qs = rng.integers(0, 256, size=(5, dim)).astype(np.float32)
        radius = np.float32(24 * 90.0 ** 2)
        dm = ix.make_mask_where([(15, 2)])
        hm = ix.make_mask(lab == 2)
        got, want = ix.range_search(qs, radius, mask=dm), ix.range_search(qs, radius, mask=hm)
        assert int(want[0][-1]) > 0
        for g, w in zip(got, want):
            assert np.array_equal(g, w)
        assert bool((lab[got[1].astype(np.int64)] == 2).all())
        dm.close()
        hm.close()
    finally:
        ix.close()


def test_errors():
    import lab_1806_vec_db_amd as vdb
    from lab_1806_vec_db_amd import _lib as L

    ix, cols = _labelled(100)
    try:
        with pytest.raises(vdb.VdbError, match="error 1.*column 16"):
            ix.make_mask_where([(16, 0)])
        with pytest.raises(vdb.VdbError, match="error 1.*9 terms"):
            ix.make_mask_where([(2, 0)] * 9)
        with pytest.raises(vdb.VdbError, match="error 1.*9 terms"):
            ix.make_masks_where([[(2, 0)], [(2, 0)] * 9])
        with pytest.raises(vdb.VdbError, match="error 1.*column 16"):
            ix.set_labels(16, np.zeros(3, dtype=np.uint32))
        with pytest.raises(vdb.VdbError, match="error 1.*pass the 100 rows"):
            ix.set_labels(2, np.zeros(3, dtype=np.uint32), first_row=98)
        with pytest.raises(vdb.VdbError, match="error 1.*pass the 100 rows"):
            ix.get_labels(2, first_row=101, count=0)
        with pytest.raises(vdb.VdbError, match="error 1.*pass the 100 rows"):
            ix.get_labels(5, first_row=50, count=51)
        with pytest.raises(vdb.VdbError, match="error 1.*column 16"):
            ix.get_labels(16)
        assert np.array_equal(ix.get_labels(2), cols[2])  # nothing was written by the refused calls
        ix.set_labels(9, np.zeros(0, dtype=np.uint32), first_row=100)  # count == 0 is fine and allocates nothing
        assert ix.get_stat("label_columns") == 2 and ix.get_labels(2, first_row=100).size == 0
        # term_lims that do not start at 0 / that decrease, straight through the C ABI
        lib = L.load()
        col = np.array([2, 2], dtype=np.uint32)
        code = np.array([0, 1], dtype=np.uint32)
        for lims, msg in (((1, 2, 2), "term_lims.0. must be 0"), ((0, 2, 1), "must not decrease")):
            out = (L.vp * 2)()
            out[0] = out[1] = 1  # (must come back NULL)
            lm = np.array(lims, dtype=np.uint64)
            st = lib.vdb_mask_create_where_many(ix._h, lm.ctypes.data_as(L.u64p), col.ctypes.data_as(L.u32p), code.ctypes.data_as(L.u32p), 2, out)
            assert st == 1 and out[0] is None and out[1] is None
            with pytest.raises(vdb.VdbError, match=msg):
                L.check(st)
    finally:
        ix.close()


def test_a_device_built_mask_goes_stale_like_any_other():
    import lab_1806_vec_db_amd as vdb

    ix, cols = _labelled(300)
    try:
        qs = np.zeros((2, 4), dtype=np.float32)
        mk = ix.make_mask_where([(2, 1)])
        ix.flat_knn_filtered(qs, 3, mk)
        ix.set_labels(2, np.full(10, 1, dtype=np.uint32))  # writing labels leaves masks valid: a mask is a set of rows
        ix.flat_knn_filtered(qs, 3, mk)
        ix.batch_add(np.ones((1, 4), dtype=np.float32))
        with pytest.raises(vdb.VdbError, match="error 3.*stale"):
            ix.flat_knn_filtered(qs, 3, mk)
        mk.close()
        other = _index(301, seed=2)
        mk = other.make_mask_where([])
        with pytest.raises(vdb.VdbError, match="error 1.*another index"):
            ix.flat_knn_filtered(qs, 3, mk)
        mk.close()
        other.close()
    finally:
        ix.close()
