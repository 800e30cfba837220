"""GPU: row masks built on the device from an OR of conjunctions of set / range terms over label columns (vdb_mask_create_where_any /
_many, k_mask_rows<MaskAny> in csrc/k_labels.hip) and the AND / OR / NOT of finished masks (vdb_mask_combine, k_mask_combine).  Every mask
is read back (vdb_mask_rows) and compared EXACTLY -- bit words and ascending allow-list -- with the mask numpy computes from the label
arrays by the rule the header states; a mask of one clause is the vdb_mask_create_where_sets mask of its terms; searches under a
device-built OR mask are compared with the reference's order restricted to the same rows and with the same searches under
vdb_mask_create's mask."""
import itertools
import threading

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NONE = 0xFFFFFFFF
# 65 / 257 rows: a second word / a second workgroup of one word; 70 001 rows are 1094 words in 274 workgroups -- more block counts than one
# iteration of the scan holds (256) and a ragged last word
SHAPES = (0, 1, 63, 64, 65, 255, 256, 257, 1000, 70001)
SCATTERED = [3, 63, 64, 127, 128, 150]


def T(col, lo=None, hi=None, neg=False, none=False, codes=None):
    from lab_1806_vec_db_amd.labels import LabelTerm

    return LabelTerm(col, lo, hi, negate=neg, none=none, codes=codes)


def _labels(n, seed=23):
    """column 2: about 200 distinct codes (the word edges of a bitmap from 0 among them), 10 % unlabelled; column 7: 3 codes, 20 %
    unlabelled"""
    rng = np.random.default_rng(seed + n)
    a = rng.integers(0, 200, size=n).astype(np.uint32)
    a[rng.random(n) < 0.1] = NONE
    if n >= 8:
        a[rng.permutation(n)[:4]] = (63, 64, 127, 128)
    b = rng.integers(0, 3, size=n).astype(np.uint32)
    b[rng.random(n) < 0.2] = NONE
    return a, b


def _labelled(n, scalar="f32"):
    """an index of n rows with columns 2 and 7 written (5 never), and the numpy twin of the columns"""
    import lab_1806_vec_db_amd as vdb

    ix = vdb.GpuIndex(4, "l2sqr", scalar=scalar)
    if n:
        rows = np.random.default_rng(1).integers(0, 256, size=(n, 4))
        ix.batch_add_u8(rows.astype(np.uint8)) if scalar == "u8" else ix.batch_add(rows.astype(np.float32))
    a, b = _labels(n)
    if n:
        ix.set_labels(2, a)
        ix.set_labels(7, b)
    return ix, {2: a, 7: b}


def _term(n, cols, t):
    """the rule of include/vdbhip.h for one term: an unlabelled row matches iff the term has NONE; a labelled one when
    (lo <= v <= hi and, with a set, v in the set) != NEGATE; a column the dict lacks reads NONE everywhere"""
    v = cols.get(t.column, np.full(n, NONE, dtype=np.uint32)).astype(np.int64)
    inside = (v >= t.lo) & (v <= t.hi)
    if t.codes is not None:
        inside &= np.isin(v, np.array(t.codes, dtype=np.int64))
    return np.where(v == NONE, t.none, inside != t.negate)


def _allowed(n, cols, clauses):
    any_ = np.zeros(n, dtype=np.bool_)
    for c in clauses:
        ok = np.ones(n, dtype=np.bool_)
        for t in c:
            ok &= _term(n, cols, t)
        any_ |= ok
    return any_


def _pack(ok):
    n = len(ok)
    padded = np.zeros((n + 63) // 64 * 64, dtype=np.uint8)
    padded[:n] = ok
    return np.packbits(padded, bitorder="little").view(np.uint64), np.flatnonzero(ok).astype(np.uint32)


def _same(mk, want, what):
    words, ids = mk.rows()
    assert words.dtype == np.uint64 and ids.dtype == np.uint32
    assert np.array_equal(words, want[0]), what
    assert np.array_equal(ids, want[1]), what
    assert len(mk) == len(want[1]), what


def _conjunctions():
    """term lists: one clause each here, and what the many-clause masks below are put together from"""
    return (
        [T(2, 10, 50)], [T(2, 1, 0)], [T(2, 1, 0, neg=True)], [T(2, codes=[64])], [T(2, 0, 199, codes=[0, 199])], [T(2, codes=SCATTERED)],
        [T(2, 100, 0xFFFFFFFF)], [T(2, 100, 0xFFFFFFFF, neg=True, none=True)],                                     # hi = 0xFFFFFFFF
        [T(5, 0, 10)], [T(5, 0, 10, none=True)], [T(5, 1, 0, neg=True)], [T(5, codes=[1, 70], neg=True, none=True)],  # never written
        [T(7, codes=[0, 2]), T(2, 64, 199, none=True)],
        [T(2, 0, 180), T(7, 0, 1, none=True), T(5, 1, 0, none=True), T(2, codes=SCATTERED, neg=True), T(7, codes=[1], neg=True, none=True),
         T(5, 3, 9, neg=True, none=True), T(2, 1, 0xFFFFFFFF, none=True), T(7, 1, 0, neg=True, none=True)],        # all 8 terms
    )


def _flag_masks():
    """two clauses -- a bitmap term or a range term on column 2, a range term on column 7 -- under every combination of NEGATE and
    NONE on each"""
    out = []
    for neg, none, neg2, none2 in itertools.product((False, True), repeat=4):
        out.append([[T(2, codes=SCATTERED, neg=neg, none=none)], [T(7, 0, 0, neg=neg2, none=none2)]])
        out.append([[T(2, 20, 90, neg=neg, none=none), T(7, codes=[0, 2], neg=neg2, none=none2)], [T(2, 150, 0xFFFFFFFF, neg=none, none=neg)]])
    return out


def _clause_lists():
    cj = _conjunctions()
    sixty_four = [[T(2, 3 * i, 3 * i, none=(i == 5)), T(7, i % 3, 2, neg=bool(i & 1), none=bool(i & 2))] for i in range(64)]
    return [
        [],                                  # 0 clauses: the empty mask
        [[]],                                # one clause without terms: every row
        *[[c] for c in cj],                  # 1 clause
        [cj[0], cj[12]], [cj[8], cj[11]], [cj[1], cj[1]], [cj[3], []],     # 2 clauses; the last holds a clause without terms
        [cj[1], [], cj[0]], [cj[3], cj[6], cj[13]], [cj[5], cj[9], cj[2]],   # 3 clauses
        sixty_four, [[T(2, c, c)] for c in range(63)] + [cj[13]],           # 64 clauses
        *_flag_masks(),
    ]


@pytest.mark.parametrize("n", SHAPES)
def test_mask_shapes(n):
    ix, cols = _labelled(n)
    try:
        lists = _clause_lists()
        assert {len(c) for c in lists} >= {0, 1, 2, 3, 64}
        names = ("mask_where_any_masks", "mask_where_set_masks", "mask_where_masks", "mask_combine_masks")
        s0 = [ix.get_stat(s) for s in names]
        many = ix.make_masks_where_any(lists)
        assert [ix.get_stat(s) for s in names] == [s0[0] + len(lists)] + s0[1:]
        sizes = []
        for g, (clauses, mk) in enumerate(zip(lists, many)):
            ok = _allowed(n, cols, clauses)
            _same(mk, _pack(ok), (n, g, clauses))
            sizes.append(int(ok.sum()))
            mk.close()
        for g in (0, 1, 14, 18, 21, 23):  # the single form
            mk = ix.make_mask_where_any(lists[g])
            _same(mk, _pack(_allowed(n, cols, lists[g])), (n, g, "single"))
            mk.close()
        assert ix.get_stat("mask_where_any_masks") == s0[0] + len(lists) + 6
        assert sizes[0] == 0 and sizes[1] == n and sizes[19] == n and sizes[20] == n
        if n == 1000:  # the lists are not degenerate at a size where every code occurs
            assert 0 < sizes[23] < n and 0 < sizes[24] < n and len(set(sizes)) > 30, sizes
    finally:
        ix.close()


def test_one_clause_is_the_where_sets_mask():
    ix, cols = _labelled(1000)
    try:
        for terms in _conjunctions() + ([],):
            a = ix.make_mask_where_any([terms])
            b = ix.make_mask_where_sets(terms)
            for x, y in zip(a.rows(), b.rows()):
                assert np.array_equal(x, y), terms
            assert len(a) == len(b)
            a.close()
            b.close()
    finally:
        ix.close()


def test_u8_index():
    """a VecSet<u8> index builds the same masks"""
    n = 1000
    ix, cols = _labelled(n, scalar="u8")
    try:
        lists = _clause_lists()
        for g, mk in enumerate(ix.make_masks_where_any(lists)):
            _same(mk, _pack(_allowed(n, cols, lists[g])), g)
            mk.close()
    finally:
        ix.close()


def _random_term(rng):
    col = int(rng.choice((2, 5, 7)))
    top = 3 if col == 7 else 210
    neg, none = bool(rng.integers(0, 2)), bool(rng.integers(0, 2))
    kind = int(rng.integers(0, 4))
    if kind == 0:
        lo, hi = sorted(int(x) for x in rng.integers(0, top, size=2))
        return T(col, lo, hi, neg, none)
    if kind == 1:
        return T(col, 1, 0, neg, none)
    if kind == 2:
        return T(col, int(rng.integers(0, top)), 0xFFFFFFFF, neg, none)
    return T(col, neg=neg, none=none, codes=rng.integers(0, top, size=int(rng.integers(1, 40))).tolist())


def _random_clauses(rng):
    return [[_random_term(rng) for _ in range(int(rng.integers(0, 4)))] for _ in range(int(rng.integers(0, 5)))]


def test_many_form_across_the_chunk_boundary():
    n = 1000
    ix, cols = _labelled(n)
    try:
        rng = np.random.default_rng(29)
        lists = [_random_clauses(rng) for _ in range(1100)]  # more than one chunk of 1024
        s0 = ix.get_stat("mask_where_any_masks")
        many = ix.make_masks_where_any(lists)
        assert len(many) == 1100 and ix.get_stat("mask_where_any_masks") == s0 + 1100
        sizes = set()
        for g, (clauses, mk) in enumerate(zip(lists, many)):
            want = _pack(_allowed(n, cols, clauses))
            _same(mk, want, (g, clauses))
            sizes.add(len(want[1]))
            mk.close()
        assert len(sizes) > 100  # (the random lists select many different row sets)
        assert ix.make_masks_where_any([]) == []
    finally:
        ix.close()


def _raw_many(ix, mlims, clims, cols, lo, hi, flags, slims, words, n_masks):
    """the C call with arrays exactly as given; (status, the out array)"""
    from lab_1806_vec_db_amd import _lib as L

    u32 = lambda a: np.array(a, dtype=np.uint32)  # noqa: E731
    u64 = lambda a: np.array(a, dtype=np.uint64)  # noqa: E731
    a_m, a_c = u64(mlims), None if clims is None else u64(clims)
    a_col, a_l, a_h, a_f = u32(cols), u32(lo), u32(hi), u32(flags)
    a_s = None if slims is None else u64(slims)
    a_w = words if isinstance(words, np.ndarray) else u64(words)
    out = (L.vp * max(n_masks, 1))()
    for g in range(n_masks):
        out[g] = 1  # (must come back NULL)
    p = lambda a, t: None if a is None else a.ctypes.data_as(t)  # noqa: E731
    st = L.load().vdb_mask_create_where_any_many(ix._h, p(a_m, L.u64p), p(a_c, L.u64p), p(a_col, L.u32p), p(a_l, L.u32p), p(a_h, L.u32p),
                                                 p(a_f, L.u32p), p(a_s, L.u64p), p(a_w, L.u64p), n_masks, out)
    return st, out


def test_invalid_calls_make_nothing():
    import lab_1806_vec_db_amd as vdb
    from lab_1806_vec_db_amd import _lib as L

    ix, cols = _labelled(1000)
    try:
        names = ("mask_where_any_masks", "mask_where_set_masks", "mask_where_masks", "mask_combine_masks")
        s0 = [ix.get_stat(s) for s in names]
        with pytest.raises(vdb.VdbError, match="error 1.*65 clauses"):
            ix.make_mask_where_any([[T(2, 0, 5)]] * 65)
        with pytest.raises(vdb.VdbError, match="error 1.*mask 1 has 65 clauses"):
            ix.make_masks_where_any([[[T(2, 0, 5)]] * 64, [[T(2, 0, 5)]] * 65])
        with pytest.raises(vdb.VdbError, match="error 1.*9 terms"):
            ix.make_mask_where_any([[T(2, 0, 5)], [T(2, 0, 5)] * 9])
        with pytest.raises(vdb.VdbError, match="error 1.*column 16"):
            ix.make_masks_where_any([[[T(2, 0, 5)]]] * 1030 + [[[T(7, 0, 1)], [T(16, 0, 1)]]])  # the invalid term comes last, in the second chunk
        big = np.zeros(9 << 18, dtype=np.uint64)  # 9 bitmaps of 2^24 codes each: more than VDB_MASK_MAX_SET_BITS in the call
        two = ((0, 1, 2), (0, 1, 2))  # two masks of one clause of one term each
        for args, msg in (
            ((*two, (2, 2), (0, 0), (5, 5), (0, 4), (0, 0, 0), (), 2), "unknown flag bits"),
            ((*two, (2, 2), (0, 0), (5, 5), (0, 0), (1, 1, 1), (0,), 2), "set_lims.0. must be 0"),
            ((*two, (2, 2), (0, 0), (63, 63), (0, 0), (0, 1, 0), (1,), 2), "set_lims must not decrease"),
            ((*two, (2, 2), (0, 0), (5, 64), (0, 0), (0, 0, 1), (1,), 2), "need 2"),          # 65 codes in one word
            ((*two, (2, 2), (0, 0), (5, 63), (0, 0), (0, 0, 2), (1, 1), 2), "need 1"),        # 64 codes in two words
            ((*two, (2, 2), (0, 9), (5, 8), (0, 0), (0, 0, 1), (1,), 2), "lo > hi"),           # a bitmap on an empty range
            ((*two, (2, 2), (0, 0), (5, NONE), (0, 0), (0, 0, 1), (1,), 2), "need 67108864"),  # the full span: 2^26 words in 64-bit arithmetic
            (((0, 9), tuple(range(10)), (2,) * 9, (0,) * 9, ((1 << 24) - 1,) * 9, (0,) * 9, tuple(g << 18 for g in range(10)), big, 1), "bitmap words in one call"),
            (((1, 1, 2), (0, 1, 2), (2, 2), (0, 0), (5, 5), (0, 0), None, (), 2), "mask_lims.0. must be 0"),
            (((0, 2, 1), (0, 1, 2), (2, 2), (0, 0), (5, 5), (0, 0), None, (), 2), "mask_lims must not decrease"),
            (((0, 1, 2), (1, 1, 2), (2, 2), (0, 0), (5, 5), (0, 0), None, (), 2), "clause_lims.0. must be 0"),
            (((0, 1, 2), (0, 2, 1), (2, 2), (0, 0), (5, 5), (0, 0), None, (), 2), "clause_lims must not decrease"),
            (((0, 1, 2), None, (2, 2), (0, 0), (5, 5), (0, 0), None, (), 2), "null argument"),
            (((0, 65), tuple(range(66)), (2,) * 65, (0,) * 65, (5,) * 65, (0,) * 65, None, (), 1), "65 clauses"),
            (((0, 1), (0, 9), (2,) * 9, (0,) * 9, (5,) * 9, (0,) * 9, None, (), 1), "9 terms"),
        ):
            st, out = _raw_many(ix, *args)
            assert st == 1 and all(out[g] is None for g in range(args[-1])), msg
            with pytest.raises(vdb.VdbError, match=msg):
                L.check(st)
        assert [ix.get_stat(s) for s in names] == s0
        assert len(ix) == 1000 and np.array_equal(ix.get_labels(2), cols[2])
        # legal: set_lims == NULL (no term has a bitmap); a mask without clauses beside others; n_masks == 0; nothing but empty masks
        st, out = _raw_many(ix, (0, 2, 2, 3), (0, 1, 2, 2), (2, 7), (10, 1), (50, 0), (0, 3), None, (), 3)
        assert st == 0
        for g, clauses in enumerate(([[T(2, 10, 50)], [T(7, 1, 0, neg=True, none=True)]], [], [[]])):
            mk = vdb.RowMask.from_handle(ix, out[g])
            _same(mk, _pack(_allowed(1000, cols, clauses)), ("legal raw call", g))
            mk.close()
        assert _raw_many(ix, (0,), None, (), (), (), (), None, (), 0)[0] == 0
        st, out = _raw_many(ix, (0, 0, 0), None, (), (), (), (), None, (), 2)
        assert st == 0
        for g in range(2):
            mk = vdb.RowMask.from_handle(ix, out[g])
            assert len(mk) == 0 and not mk.rows()[0].any()
            mk.close()
        assert ix.get_stat("mask_where_any_masks") == s0[0] + 5
    finally:
        ix.close()


# ---- vdb_mask_combine -------------------------------------------------------------------------------------------------------------------
def _eight_masks(ix, cols, n):
    """eight masks of one index from all four constructors, and the bool array of each"""
    rng = np.random.default_rng(n)
    host = [rng.random(n) < p for p in (0.5, 0.9)]
    eq = [(2, int(cols[2][0])), (7, NONE)]
    sets = [[T(2, codes=SCATTERED, neg=True)], [T(7, 0, 1, none=True), T(2, 5, 150)]]
    anys = [[[T(2, 10, 50)], [T(7, 2, 2)]], [[T(2, 100, 0xFFFFFFFF)], [T(5, 1, 0, none=True), T(7, 0, 0)]]]
    masks = [ix.make_mask(host[0]), ix.make_mask_where([eq[0]]), ix.make_mask_where_sets(sets[0]), ix.make_mask_where_any(anys[0]),
             ix.make_mask_where_any(anys[1]), ix.make_mask_where_sets(sets[1]), ix.make_mask_where([eq[1]]), ix.make_mask(host[1])]
    bools = [host[0], cols[2] == eq[0][1], _allowed(n, cols, [sets[0]]), _allowed(n, cols, anys[0]), _allowed(n, cols, anys[1]),
             _allowed(n, cols, [sets[1]]), cols[7] == NONE, host[1]]
    for mk, b in zip(masks, bools):
        _same(mk, _pack(b), "combine input")
    return masks, bools


@pytest.mark.parametrize("n", (65, 257))
def test_combine_every_invert_pattern(n):
    ix, cols = _labelled(n)
    try:
        masks, bools = _eight_masks(ix, cols, n)
        s0, a0 = ix.get_stat("mask_combine_masks"), ix.get_stat("mask_where_any_masks")
        made = 0
        for n_in in (1, 2, 8):
            for first in ((0,) if n_in == 8 else (0, 3, 6)):  # (which inputs: constructors mixed)
                ms, bs = masks[first:first + n_in], bools[first:first + n_in]
                for op, fold in (("and", np.logical_and), ("or", np.logical_or)):
                    for inv in [None] + list(itertools.product((False, True), repeat=n_in)):
                        want = None
                        for b, v in zip(bs, inv or (False,) * n_in):
                            x = ~b if v else b
                            want = x if want is None else fold(want, x)
                        mk = ix.combine_masks(op, ms, inv)
                        _same(mk, _pack(want), (n, n_in, first, op, inv))  # (the words compare whole: tail bits clear under NOT)
                        mk.close()
                        made += 1
        assert made == 2 * (3 * 3 + 3 * 5 + 257)
        assert ix.get_stat("mask_combine_masks") == s0 + made and ix.get_stat("mask_where_any_masks") == a0
        nots = ix.combine_masks("or", [masks[7]], [True])
        assert len(nots) == n - len(masks[7])
        both = ix.combine_masks(0, [nots, masks[7]])  # the integer op codes; a combined mask as an input
        assert len(both) == 0 and not both.rows()[0].any()
        for mk in masks + [nots, both]:
            mk.close()
    finally:
        ix.close()


def test_combine_empty_index_and_larger_table():
    import lab_1806_vec_db_amd as vdb

    ex = vdb.GpuIndex(4, "l2sqr")
    try:
        a, b = ex.make_mask([]), ex.make_mask_where_any([[]])
        c = ex.combine_masks("or", [a, b], [True, False])
        assert len(c) == 0 and c.rows()[0].size == 0
        for mk in (a, b, c):
            mk.close()
    finally:
        ex.close()
    n = 70001  # 274 block counts: two iterations of the scan, a ragged last word
    ix, cols = _labelled(n)
    try:
        x, y = ix.make_mask_where_any([[T(2, 10, 50)], [T(7, 2, 2)]]), ix.make_mask(np.arange(n) % 3 == 0)
        bx, by = _allowed(n, cols, [[T(2, 10, 50)], [T(7, 2, 2)]]), np.arange(n) % 3 == 0
        for op, inv, want in (("and", (False, True), bx & ~by), ("or", (True, True), ~bx | ~by), ("or", None, bx | by)):
            mk = ix.combine_masks(op, [x, y], inv)
            _same(mk, _pack(want), (op, inv))
            mk.close()
        x.close()
        y.close()
    finally:
        ix.close()


def test_combine_errors():
    import ctypes as C

    import lab_1806_vec_db_amd as vdb
    from lab_1806_vec_db_amd import _lib as L

    ix, cols = _labelled(300)
    other, _ = _labelled(300)
    try:
        mine, theirs = ix.make_mask_where_any([[T(2, 10, 50)]]), other.make_mask_where_any([[T(2, 10, 50)]])
        s0 = ix.get_stat("mask_combine_masks")
        with pytest.raises(vdb.VdbError, match="error 1.*another index"):
            ix.combine_masks("and", [mine, theirs])
        with pytest.raises(vdb.VdbError, match="error 1.*0 inputs"):
            ix.combine_masks("and", [])
        with pytest.raises(vdb.VdbError, match="error 1.*9 inputs"):
            ix.combine_masks("or", [mine] * 9)
        with pytest.raises(vdb.VdbError, match="error 1.*unknown op"):
            ix.combine_masks(2, [mine])
        with pytest.raises(vdb.VdbError, match="error 1.*unknown op"):
            ix.combine_masks("xor", [mine])
        with pytest.raises(ValueError):
            ix.combine_masks("or", [mine, mine], [True])
        arr = (L.vp * 2)(mine._h, None)  # a NULL input, through the C call: *out comes back NULL
        out = L.vp(1)
        assert L.load().vdb_mask_combine(ix._h, 0, arr, None, 2, C.byref(out)) == 1 and out.value is None
        ok = ix.combine_masks("or", [mine, mine], [False, True])
        assert len(ok) == 300
        ix.batch_add(np.ones((1, 4), dtype=np.float32))
        with pytest.raises(vdb.VdbError, match="error 3.*stale"):
            ix.combine_masks("and", [mine])
        fresh = ix.make_mask_where_any([[]])
        with pytest.raises(vdb.VdbError, match="error 3.*stale"):
            ix.combine_masks("and", [fresh, ok])
        assert ix.get_stat("mask_combine_masks") == s0 + 1
        for mk in (mine, theirs, ok, fresh):
            mk.close()
    finally:
        ix.close()
        other.close()


# ---- searches under a device-built OR mask ------------------------------------------------------------------------------------------------
def _full_order(base, qs, kind=0):
    from oracle import oracle as O

    oi, od, oc = O.flat_knn_batch(base, qs, len(base), kind, nthreads=16)
    assert (oc == len(base)).all()
    return oi.astype(np.uint64), od


def _expect_knn(full, allow, k):
    oi, od = full
    nq = len(oi)
    idx, dist, cnt = np.zeros((nq, k), dtype=np.uint64), np.zeros((nq, k), dtype=np.float32), np.zeros(nq, dtype=np.uint64)
    for q in range(nq):
        keep = allow[oi[q].astype(np.int64)]
        c = min(k, int(keep.sum()))
        idx[q, :c], dist[q, :c], cnt[q] = oi[q][keep][:c], od[q][keep][:c], c
    return idx, dist, cnt


def _expect_range(full, allow, radii):
    oi, od = full
    lims, ids, ds = [0], [], []
    for q in range(len(oi)):
        keep = allow[oi[q].astype(np.int64)]
        fi, fd = oi[q][keep], od[q][keep]
        cut = int((fd <= np.float32(radii[q])).sum())
        ids.append(fi[:cut])
        ds.append(fd[:cut])
        lims.append(lims[-1] + cut)
    return np.array(lims, dtype=np.uint64), np.concatenate(ids), np.concatenate(ds)


def _same_knn(a, b, what):
    assert np.array_equal(a[2], b[2]) and np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32)), what


def _same_range(a, b, what):
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[2].view(np.uint32), b[2].astype(np.float32).view(np.uint32)), what


def _search_table(n, dim, codes0, seed):
    """gist-like rows with column 0 (codes0 values) and column 1 (years 0 .. 34, 10 % unlabelled), the OR mask
    `column 0 in {1, 2} OR (column 1 >= 20 AND column 0 != 0)` built on the device, and its rows"""
    import lab_1806_vec_db_amd as vdb
    from conftest import gist_like

    base = gist_like(n, dim=dim, seed=seed)
    rng = np.random.default_rng(seed)
    c0 = rng.integers(0, codes0, size=n).astype(np.uint32)
    c1 = rng.integers(0, 35, size=n).astype(np.uint32)
    c1[rng.random(n) < 0.1] = NONE
    ix = vdb.GpuIndex(dim, "l2sqr")
    ix.batch_add(base)
    ix.set_labels(0, c0)
    ix.set_labels(1, c1)
    clauses = [[T(0, codes=[1, 2])], [T(1, 20, 0xFFFFFFFF), T(0, 0, 0, neg=True, none=True)]]
    allow = _allowed(n, {0: c0, 1: c1}, clauses)
    assert np.array_equal(allow, np.isin(c0, (1, 2)) | ((c1 != NONE) & (c1 >= 20) & (c0 != 0)))
    return base, ix, ix.make_mask_where_any(clauses), allow


def test_search_under_an_or_mask_direct_path():
    from conftest import gist_like

    base, ix, dm, allow = _search_table(3000, 64, 12, seed=3101)
    try:
        assert 0 < len(dm) == int(allow.sum()) <= 8192
        qs = gist_like(9, dim=64, seed=3102)
        full = _full_order(base, qs)
        hm = ix.make_mask(allow)
        s0 = ix.get_stat("flat_filtered_direct_queries")
        for k in (1, 10, 300):
            got = ix.flat_knn_filtered(qs, k, dm)
            _same_knn(got, _expect_knn(full, allow, k), k)
            _same_knn(got, ix.flat_knn_filtered(qs, k, hm), k)
        assert ix.get_stat("flat_filtered_direct_queries") == s0 + 6 * len(qs)
        r = _expect_knn(full, allow, 40)[1][:, 39].copy()
        got = ix.range_search(qs, r, mask=dm)
        _same_range(got, _expect_range(full, allow, r), "range")
        _same_range(got, ix.range_search(qs, r, mask=hm), "range, host mask")
        hm.close()
        dm.close()
    finally:
        ix.close()


@pytest.mark.parametrize("dim", (64, 128))
def test_search_under_an_or_mask_long_allow_list(dim):
    """20 000 rows, about 12 000 of them allowed: past flat_filtered_direct_max (8192), where the 8-bit tier answers when the dimension
    has one -- 128 has (asserted), 64 has not (one 64-column block): the same mask then goes the way such a table goes"""
    from conftest import gist_like

    base, ix, dm, allow = _search_table(20000, dim, 4, seed=3200 + dim)
    try:
        assert 11000 < len(dm) == int(allow.sum()) < 13000
        qs = gist_like(40, dim=dim, seed=3300 + dim)
        full = _full_order(base, qs)
        hm = ix.make_mask(allow)
        s0 = ix.get_stat("flat_filtered_i8_queries")
        got = ix.flat_knn_filtered(qs, 10, dm)
        took = ix.get_stat("flat_filtered_i8_queries") - s0
        print("dim", dim, "queries through the 8-bit tier:", took)
        assert took == (len(qs) if dim == 128 else 0)
        _same_knn(got, _expect_knn(full, allow, 10), dim)
        _same_knn(got, ix.flat_knn_filtered(qs, 10, hm), dim)
        hm.close()
        dm.close()
    finally:
        ix.close()


def test_range_search_under_an_or_mask_u8_index():
    import lab_1806_vec_db_amd as vdb

    n, dim = 2000, 24
    rng = np.random.default_rng(6)
    rows = rng.integers(0, 256, size=(n, dim), dtype=np.uint8)
    ix = vdb.GpuIndex(dim, "l2sqr", scalar="u8")
    try:
        ix.batch_add_u8(rows)
        lab = rng.integers(0, 100, size=n).astype(np.uint32)
        lab[::9] = NONE
        ix.set_labels(15, lab)
        qs = rng.integers(0, 256, size=(5, dim)).astype(np.float32)
        full = _full_order(rows.astype(np.float32), qs)
        clauses = [[T(15, codes=list(range(0, 100, 7)))], [T(15, 1, 0, none=True)], [T(15, 90, 0xFFFFFFFF)]]
        allow = _allowed(n, {15: lab}, clauses)
        dm, hm = ix.make_mask_where_any(clauses), ix.make_mask(allow)
        r = _expect_knn(full, allow, 30)[1][:, 29].copy()
        got = ix.range_search(qs, r, mask=dm)
        assert int(got[0][-1]) >= 150
        _same_range(got, _expect_range(full, allow, r), "u8")
        _same_range(got, ix.range_search(qs, r, mask=hm), "u8, host mask")
        dm.close()
        hm.close()
    finally:
        ix.close()


def test_two_threads_build_masks_at_once():
    n = 70001
    ix, cols = _labelled(n)
    try:
        rng = np.random.default_rng(41)
        work = [[_random_clauses(rng) for _ in range(40)] for _ in range(2)]
        bools = [[_allowed(n, cols, c) for c in w] for w in work]
        want = [[_pack(b) for b in bs] for bs in bools]
        errors = []
        start = threading.Barrier(2)

        def run(t):
            try:
                start.wait()
                for _ in range(3):
                    many = ix.make_masks_where_any(work[t])
                    both = ix.combine_masks("and", [many[0], many[1]], [False, True])
                    _same(both, _pack(bools[t][0] & ~bools[t][1]), (t, "combine"))
                    for g, mk in enumerate(many):
                        _same(mk, want[t][g], (t, g))
                        mk.close()
                    both.close()
            except BaseException as e:  # noqa: BLE001
                errors.append(e)

        threads = [threading.Thread(target=run, args=(t,)) for t in range(2)]
        for th in threads:
            th.start()
        for th in threads:
            th.join()
        assert not errors, errors
    finally:
        ix.close()
