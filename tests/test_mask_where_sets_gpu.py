"""GPU: row masks built on the device from SET and RANGE terms over label columns (vdb_mask_create_where_sets / _many,
k_mask_rows<MaskAll> in csrc/k_labels.hip).  Every mask is read back (vdb_mask_rows) and compared EXACTLY -- bit words and ascending
allow-list -- with the mask numpy computes from the label arrays by the rule the header states; the two documented equivalences with the
equality terms of vdb_mask_create_where give identical masks; searches under a set mask are compared with the same searches under
vdb_mask_create's mask of the same rows."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NONE = 0xFFFFFFFF
NEGATE, NONE_FLAG = 1, 2
# the shapes of test_mask_where_gpu: 300 001 rows are 4688 words in 1172 workgroups -- more block counts than one iteration of the scan
# holds (256) and a ragged last word; 65 and 257 rows: a second word / a second workgroup of one word
SHAPES = (0, 1, 63, 64, 65, 255, 256, 257, 1000, 300001)


def _labels(n, seed=11):
    """column 2: about 200 distinct codes (63, 64, 127 and 128 -- the word edges of a bitmap from 0 -- among them), 10 % unlabelled;
    column 7: 3 codes"""
    rng = np.random.default_rng(seed + n)
    a = rng.integers(0, 200, size=n).astype(np.uint32)
    a[rng.random(n) < 0.1] = NONE
    if n >= 8:
        a[rng.permutation(n)[:4]] = (63, 64, 127, 128)
    b = rng.integers(0, 3, size=n).astype(np.uint32)
    b[rng.random(n) < 0.2] = NONE
    return a, b


def T(col, lo=None, hi=None, neg=False, none=False, codes=None):
    from lab_1806_vec_db_amd.labels import LabelTerm

    return LabelTerm(col, lo, hi, negate=neg, none=none, codes=codes)


def _allowed(n, cols, terms):
    """the rule of include/vdbhip.h, written out: an unlabelled row matches a term iff it has NONE; a labelled one when
    (lo <= v <= hi and, with a set, v in the set) != NEGATE; a column the dict lacks reads NONE everywhere"""
    ok = np.ones(n, dtype=np.bool_)
    for t in terms:
        v = cols.get(t.column, np.full(n, NONE, dtype=np.uint32)).astype(np.int64)
        inside = (v >= t.lo) & (v <= t.hi)
        if t.codes is not None:
            inside &= np.isin(v, np.array(t.codes, dtype=np.int64))
        ok &= np.where(v == NONE, t.none, inside != t.negate)
    return ok


def _expect(n, cols, terms):
    ok = _allowed(n, cols, terms)
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


def _term_lists():
    scattered = [3, 63, 64, 127, 128, 150]
    return (
        [],                                                        # zero terms: every row
        [T(2, 10, 50)],                                            # a pure range
        [T(2, 1, 0)], [T(2, 1, 0, neg=True)],                      # the empty range: nothing / every labelled row
        [T(2, codes=[64])], [T(2, 0, 199, codes=[64])],            # a single-code bitmap, tight and inside a wide span
        [T(2, 0, 199, codes=[0, 199])], [T(2, 63, 128, codes=[63, 128])],  # only the first and the last bit set
        [T(2, codes=scattered)],
        [T(2, codes=scattered, neg=True)],                         # NEGATE
        [T(2, 10, 50, none=True)], [T(2, codes=scattered, none=True)],  # NONE
        [T(2, codes=scattered, neg=True, none=True)], [T(2, 10, 50, neg=True, none=True)],  # NEGATE | NONE
        [T(2, 100, 0xFFFFFFFF)], [T(2, 100, 0xFFFFFFFF, neg=True)],     # hi = 0xFFFFFFFF
        [T(5, 0, 10)], [T(5, 0, 10, none=True)], [T(5, 1, 0, neg=True)], [T(5, codes=[1, 70], neg=True, none=True)],  # never written
        [T(2, 10, 150), T(2, codes=[5, 64, 149, 150, 151], neg=True)],  # two terms on one column
        [T(7, codes=[0, 2]), T(2, 64, 199, none=True)],
        [T(2, 0, 180), T(7, 0, 1, none=True), T(5, 1, 0, none=True), T(2, codes=scattered, neg=True), T(7, codes=[1], neg=True, none=True),
         T(5, 3, 9, neg=True, none=True), T(2, 1, 0xFFFFFFFF, none=True), T(7, 1, 0, neg=True, none=True)],  # all 8 terms
    )


@pytest.mark.parametrize("n", SHAPES)
def test_mask_shapes(n):
    ix, cols = _labelled(n)
    try:
        lists = _term_lists()
        s0, e0 = ix.get_stat("mask_where_set_masks"), ix.get_stat("mask_where_masks")
        for terms in lists:
            mk = ix.make_mask_where_sets(terms)
            _same(mk, _expect(n, cols, terms), (n, terms))
            mk.close()
        assert ix.get_stat("mask_where_set_masks") == s0 + len(lists) and ix.get_stat("mask_where_masks") == e0
        if n == 1000:  # the lists are not degenerate at a size where every code occurs
            sizes = [int(_allowed(n, cols, t).sum()) for t in lists]
            assert sizes[0] == n and sizes[2] == 0 and all(0 < m < n for m in sizes[4:16]), sizes
    finally:
        ix.close()


def test_equality_equivalences_give_the_masks_of_make_mask_where():
    ix, cols = _labelled(1000)
    try:
        for c in (2, 7, 5):
            for code in (0, 2, 64, 128, 9999, NONE):
                eq = ix.make_mask_where([(c, code)])
                st = ix.make_mask_where_sets([T(c, 1, 0, none=True) if code == NONE else T(c, code, code)])
                for a, b in zip(eq.rows(), st.rows()):
                    assert np.array_equal(a, b), (c, code)
                assert len(eq) == len(st)
                eq.close()
                st.close()
    finally:
        ix.close()


def _random_terms(rng):
    out = []
    for _ in range(int(rng.integers(0, 4))):
        col = int(rng.choice((2, 5, 7)))
        top = 3 if col == 7 else 210
        neg, none = bool(rng.integers(0, 2)), bool(rng.integers(0, 2))
        kind = int(rng.integers(0, 4))
        if kind == 0:
            lo, hi = sorted(int(x) for x in rng.integers(0, top, size=2))
            out.append(T(col, lo, hi, neg, none))
        elif kind == 1:
            out.append(T(col, 1, 0, neg, none))
        elif kind == 2:
            out.append(T(col, int(rng.integers(0, top)), 0xFFFFFFFF, neg, none))
        else:
            out.append(T(col, neg=neg, none=none, codes=rng.integers(0, top, size=int(rng.integers(1, 40))).tolist()))
    return out


def test_many_form_across_the_chunk_boundary():
    n = 1000
    ix, cols = _labelled(n)
    try:
        rng = np.random.default_rng(19)
        lists = [_random_terms(rng) for _ in range(1100)]  # more than one chunk of 1024
        s0 = ix.get_stat("mask_where_set_masks")
        many = ix.make_masks_where_sets(lists)
        assert len(many) == 1100 and ix.get_stat("mask_where_set_masks") == s0 + 1100
        sizes = set()
        for g, (terms, mk) in enumerate(zip(lists, many)):
            want = _expect(n, cols, terms)
            _same(mk, want, (g, terms))
            sizes.add(len(want[1]))
            mk.close()
        assert len(sizes) > 100  # (the random lists select many different row sets)
        assert ix.make_masks_where_sets([]) == []
    finally:
        ix.close()


def _raw_many(ix, tlims, cols, lo, hi, flags, slims, words, n_masks):
    """the C call with arrays exactly as given; (status, the out array)"""
    from lab_1806_vec_db_amd import _lib as L

    u32 = lambda a: np.array(a, dtype=np.uint32)  # noqa: E731
    u64 = lambda a: np.array(a, dtype=np.uint64)  # noqa: E731
    a_t, a_c, a_l, a_h, a_f = u64(tlims), u32(cols), u32(lo), u32(hi), u32(flags)
    a_s = None if slims is None else u64(slims)
    a_w = words if isinstance(words, np.ndarray) else u64(words)
    out = (L.vp * max(n_masks, 1))()
    for g in range(n_masks):
        out[g] = 1  # (must come back NULL)
    p = lambda a, t: None if a is None else a.ctypes.data_as(t)  # noqa: E731
    st = L.load().vdb_mask_create_where_sets_many(ix._h, p(a_t, L.u64p), p(a_c, L.u32p), p(a_l, L.u32p), p(a_h, L.u32p), p(a_f, L.u32p),
                                                  p(a_s, L.u64p), p(a_w, L.u64p), n_masks, out)
    return st, out


def test_invalid_calls_make_nothing():
    import lab_1806_vec_db_amd as vdb
    from lab_1806_vec_db_amd import _lib as L

    ix, cols = _labelled(1000)
    try:
        s0 = ix.get_stat("mask_where_set_masks")
        with pytest.raises(vdb.VdbError, match="error 1.*9 terms"):
            ix.make_mask_where_sets([T(2, 0, 5)] * 9)
        with pytest.raises(vdb.VdbError, match="error 1.*9 terms"):
            ix.make_masks_where_sets([[T(2, 0, 5)], [T(2, 0, 5)] * 9])
        with pytest.raises(vdb.VdbError, match="error 1.*column 16"):
            ix.make_masks_where_sets([[T(2, 0, 5)]] * 1030 + [[T(7, 0, 1), T(16, 0, 1)]])  # the invalid term comes last, in the second chunk
        big = np.zeros(9 << 18, dtype=np.uint64)  # 9 bitmaps of 2^24 codes each: more than VDB_MASK_MAX_SET_BITS in the call
        for args, msg in (
            (((0, 1, 2), (2, 2), (0, 0), (5, 5), (0, 4), (0, 0, 0), (), 2), "unknown flag bits"),
            (((0, 1, 2), (2, 2), (0, 0), (5, 5), (0, 0), (1, 1, 1), (0,), 2), "set_lims.0. must be 0"),
            (((0, 1, 2), (2, 2), (0, 0), (63, 63), (0, 0), (0, 1, 0), (1,), 2), "set_lims must not decrease"),
            (((0, 1, 2), (2, 2), (0, 0), (5, 64), (0, 0), (0, 0, 1), (1,), 2), "need 2"),          # 65 codes in one word
            (((0, 1, 2), (2, 2), (0, 0), (5, 63), (0, 0), (0, 0, 2), (1, 1), 2), "need 1"),        # 64 codes in two words
            (((0, 1, 2), (2, 2), (0, 9), (5, 8), (0, 0), (0, 0, 1), (1,), 2), "lo > hi"),           # a bitmap on an empty range
            (((0, 1, 2), (2, 2), (0, 0), (5, NONE), (0, 0), (0, 0, 1), (1,), 2), "need 67108864"),  # the full span: 2^26 words in 64-bit arithmetic
            ((tuple(range(10)), (2,) * 9, (0,) * 9, ((1 << 24) - 1,) * 9, (0,) * 9, tuple(g << 18 for g in range(10)), big, 9), "bitmap words in one call"),
            (((1, 1, 2), (2, 2), (0, 0), (5, 5), (0, 0), None, (), 2), "term_lims.0. must be 0"),
            (((0, 2, 1), (2, 2), (0, 0), (5, 5), (0, 0), None, (), 2), "term_lims must not decrease"),
        ):
            st, out = _raw_many(ix, *args)
            assert st == 1 and all(out[g] is None for g in range(args[-1])), msg
            with pytest.raises(vdb.VdbError, match=msg):
                L.check(st)
        assert ix.get_stat("mask_where_set_masks") == s0
        assert len(ix) == 1000 and np.array_equal(ix.get_labels(2), cols[2])
        # set_lims == NULL: no term has a bitmap; n_masks == 0 succeeds
        st, out = _raw_many(ix, (0, 1, 2), (2, 7), (10, 1), (50, 0), (0, NEGATE | NONE_FLAG), None, (), 2)
        assert st == 0
        for g, terms in enumerate(([T(2, 10, 50)], [T(7, 1, 0, neg=True, none=True)])):
            mk = vdb.RowMask.from_handle(ix, out[g])
            _same(mk, _expect(1000, cols, terms), "null set_lims")
            mk.close()
        assert _raw_many(ix, (0,), (), (), (), (), None, (), 0)[0] == 0
        assert ix.get_stat("mask_where_set_masks") == s0 + 2
    finally:
        ix.close()


def test_a_set_mask_goes_stale_like_any_other():
    import lab_1806_vec_db_amd as vdb

    ix, cols = _labelled(300)
    try:
        qs = np.zeros((2, 4), dtype=np.float32)
        mk = ix.make_mask_where_sets([T(2, codes=[1, 64, 90], neg=True)])
        ix.flat_knn_filtered(qs, 3, mk)
        ix.batch_add(np.ones((1, 4), dtype=np.float32))
        with pytest.raises(vdb.VdbError, match="error 3.*stale"):
            ix.flat_knn_filtered(qs, 3, mk)
        mk.close()
    finally:
        ix.close()


def _same_knn(a, b, what):
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32)) and np.array_equal(a[2], b[2]), what


def test_search_under_a_set_mask_direct_path():
    n = 1000
    ix, cols = _labelled(n)
    try:
        qs = np.random.default_rng(3).random((9, 4)).astype(np.float32)
        for terms in ([T(2, codes=[3, 63, 64, 127, 128, 150])], [T(2, 10, 150), T(7, codes=[0, 2], none=True)], [T(2, 1, 0)]):
            dm = ix.make_mask_where_sets(terms)
            hm = ix.make_mask(_expect(n, cols, terms)[1])
            for k in (1, 10, 300):
                _same_knn(ix.flat_knn_filtered(qs, k, dm), ix.flat_knn_filtered(qs, k, hm), (terms, k))
            for got, want in zip(ix.range_search(qs, 0.3, mask=dm), ix.range_search(qs, 0.3, mask=hm)):
                assert np.array_equal(got, want), terms
            dm.close()
            hm.close()
    finally:
        ix.close()


def test_search_under_a_set_mask_8bit_tier():
    """the 8-bit tier reads the mask's bit words (through the masked row constants): the smallest table that takes it by default
    (16 384 rows) under an allow-list past flat_filtered_direct_max (8192)"""
    from conftest import gist_like

    n, dim = 16384, 128
    ix = _index(0, dim=dim)
    try:
        ix.batch_add(gist_like(n, dim=dim, seed=77))
        lab = np.random.default_rng(4).integers(0, 130, size=n).astype(np.uint32)
        ix.set_labels(0, lab)
        qs = gist_like(40, dim=dim, seed=78)
        keep = [c for c in range(130) if c % 3]  # two thirds of the codes, over three bitmap words
        terms = [T(0, codes=keep)]
        dm = ix.make_mask_where_sets(terms)
        hm = ix.make_mask(np.isin(lab, keep))
        assert len(dm) == len(hm) == int(np.isin(lab, keep).sum()) > 8192
        s0 = ix.get_stat("flat_filtered_i8_queries")
        got = ix.flat_knn_filtered(qs, 10, dm)
        assert ix.get_stat("flat_filtered_i8_queries") == s0 + len(qs)
        _same_knn(got, ix.flat_knn_filtered(qs, 10, hm), "8-bit tier")
        assert bool(np.isin(lab[got[0].astype(np.int64)], keep).all())
        dm.close()
        hm.close()
    finally:
        ix.close()


def test_range_search_under_a_set_mask_u8_index():
    import lab_1806_vec_db_amd as vdb

    n, dim = 700, 24
    rng = np.random.default_rng(6)
    rows = rng.integers(0, 256, size=(n, dim), dtype=np.uint8)
    ix = vdb.GpuIndex(dim, "l2sqr", scalar="u8")
    try:
        ix.batch_add_u8(rows)
        lab = rng.integers(0, 100, size=n).astype(np.uint32)
        lab[::9] = NONE
        ix.set_labels(15, lab)
        qs = rng.integers(0, 256, size=(5, dim)).astype(np.float32)
        radius = np.float32(24 * 90.0 ** 2)
        terms = [T(15, codes=list(range(0, 100, 2)), neg=True, none=True)]  # the odd codes and the unlabelled rows
        dm = ix.make_mask_where_sets(terms)
        allow = _allowed(n, {15: lab}, terms)
        hm = ix.make_mask(allow)
        got, want = ix.range_search(qs, radius, mask=dm), ix.range_search(qs, radius, mask=hm)
        assert int(want[0][-1]) > 0
        for g, w in zip(got, want):
            assert np.array_equal(g, w)
        assert bool(allow[got[1].astype(np.int64)].all())
        dm.close()
        hm.close()
    finally:
        ix.close()
