"""GPU: the five ways to build a row mask on the device from the label columns agree.  One predicate, `column 0 == A and column 1 == B`,
is built through make_mask_where (equality terms), make_mask_where_sets (a range lo == hi, and a one-bit bitmap), make_mask_where_any
(one clause) and as the AND of the two make_masks_partition masks; bit words and ascending allow-list (vdb_mask_rows) are the same in
all five and equal the mask numpy computes from the label arrays.  Every call moves exactly its own counter by the masks it made and,
with profiling on, only its own profile entry has launches.  Also: an OR of two clauses against combine_masks("or"), an equality term
on LABEL_NONE against the TERM_NONE term over the empty range, and one _many call of three masks per form against the singles.

Rows: 63 / 64 / 65 are the tail bits of the last word and one row into a second word, 255 / 256 / 257 the edge of a workgroup's four
words and one row into a second workgroup; 0 is the empty index, which launches nothing."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NONE = 0xFFFFFFFF
A, B = 1, 6
COUNTERS = ("mask_where_masks", "mask_where_set_masks", "mask_where_any_masks", "mask_combine_masks", "mask_partition_masks")
PROFILES = ("mask_where", "mask_where_sets", "mask_where_any", "mask_combine", "mask_partition")


def T(col, lo=None, hi=None, neg=False, none=False, codes=None):
    from lab_1806_vec_db_amd.labels import LabelTerm

    return LabelTerm(col, lo, hi, negate=neg, none=none, codes=codes)


def _labelled(n):
    """an index of n rows with label columns 0 (codes 0 .. 2), 1 (5 .. 6) and 3 (9) written, some rows unlabelled in each, and column 5
    never written; and the numpy twin of the columns"""
    import lab_1806_vec_db_amd as vdb

    rng = np.random.default_rng(1806 + n)
    cols = {0: rng.integers(0, 3, size=n).astype(np.uint32), 1: rng.integers(5, 7, size=n).astype(np.uint32), 3: np.full(n, 9, dtype=np.uint32)}
    for c, share in ((0, 0.2), (1, 0.25), (3, 0.5)):
        cols[c][rng.random(n) < share] = NONE
    ix = vdb.GpuIndex(4, "l2sqr")
    if n:
        ix.batch_add(rng.integers(0, 256, size=(n, 4)).astype(np.float32))
        for c, v in cols.items():
            ix.set_labels(c, v)
    cols[5] = np.full(n, NONE, dtype=np.uint32)
    return ix, cols


def _pack(ok):
    n = len(ok)
    padded = np.zeros((n + 63) // 64 * 64, dtype=np.uint8)
    padded[:n] = ok
    return np.packbits(padded, bitorder="little").view(np.uint64), np.flatnonzero(ok).astype(np.uint32)


def _same(mk, want, what):
    words, ids = mk.rows()
    assert np.array_equal(words, want[0]), what
    assert np.array_equal(ids, want[1]), what
    assert len(mk) == len(want[1]), what


class _Watch:
    """runs one call and checks what it moved: the counters by exactly `made` (a dict, the others by nothing) and, on an index with
    rows, launches under the profile names of `made`'s forms alone"""

    def __init__(self, ix, n):
        self.ix, self.n = ix, n

    def __call__(self, call, **made):
        ix = self.ix
        ix.prof_reset()
        before = {c: ix.get_stat(c) for c in COUNTERS}
        out = call()
        for c, p in zip(COUNTERS, PROFILES):
            assert ix.get_stat(c) - before[c] == made.get(p, 0), (p, made)
            launches = ix.prof_get(p)["launches"]
            assert (launches > 0) == (p in made and self.n > 0), (p, launches, made)
        return out


@pytest.mark.parametrize("n", (0, 1, 63, 64, 65, 255, 256, 257))
def test_the_five_forms_build_the_same_mask(n):
    ix, cols = _labelled(n)
    ix.prof_enable(True)
    watch = _Watch(ix, n)
    want = _pack((cols[0] == A) & (cols[1] == B))

    five = {
        "where": watch(lambda: ix.make_mask_where([(0, A), (1, B)]), mask_where=1),
        "sets, lo == hi": watch(lambda: ix.make_mask_where_sets([T(0, A, A), T(1, B, B)]), mask_where_sets=1),
        "sets, one-bit bitmap": watch(lambda: ix.make_mask_where_sets([T(0, codes=[A]), T(1, codes=[B])]), mask_where_sets=1),
        "any, one clause": watch(lambda: ix.make_mask_where_any([[T(0, A, A), T(1, B, B)]]), mask_where_any=1),
    }
    pa = watch(lambda: ix.make_masks_partition(0, [A]), mask_partition=1)[0]
    pb = watch(lambda: ix.make_masks_partition(1, [B]), mask_partition=1)[0]
    five["and of two partition masks"] = watch(lambda: ix.combine_masks("and", [pa, pb]), mask_combine=1)
    for what, mk in five.items():
        _same(mk, want, (n, what))

    # an OR of two clauses is the OR of the clauses' masks
    want_or = _pack((cols[0] == A) | (cols[1] == B))
    _same(watch(lambda: ix.make_mask_where_any([[T(0, A, A)], [T(1, B, B)]]), mask_where_any=1), want_or, (n, "any, two clauses"))
    ma = watch(lambda: ix.make_mask_where([(0, A)]), mask_where=1)
    mb = watch(lambda: ix.make_mask_where([(1, B)]), mask_where=1)
    _same(watch(lambda: ix.combine_masks("or", [ma, mb]), mask_combine=1), want_or, (n, "or of two masks"))

    # the rows without a value: an equality term on LABEL_NONE, the TERM_NONE term over the empty range; column 5 was never written
    for col in (0, 5):
        want_none = _pack(cols[col] == NONE)
        _same(watch(lambda: ix.make_mask_where([(col, NONE)]), mask_where=1), want_none, (n, "where NONE", col))
        _same(watch(lambda: ix.make_mask_where_sets([T(col, 1, 0, none=True)]), mask_where_sets=1), want_none, (n, "sets NONE", col))
        _same(watch(lambda: ix.make_mask_where_any([[T(col, 1, 0, none=True)]]), mask_where_any=1), want_none, (n, "any NONE", col))

    # one _many call of three masks per form: what the singles make
    wants = [want, _pack(cols[0] == A), _pack(np.ones(n, dtype=np.bool_))]
    many = {
        "where": watch(lambda: ix.make_masks_where([[(0, A), (1, B)], [(0, A)], []]), mask_where=3),
        "sets": watch(lambda: ix.make_masks_where_sets([[T(0, A, A), T(1, codes=[B])], [T(0, codes=[A])], []]), mask_where_sets=3),
        "any": watch(lambda: ix.make_masks_where_any([[[T(0, A, A), T(1, B, B)]], [[T(0, A, A)]], [[]]]), mask_where_any=3),
    }
    for what, mks in many.items():
        assert len(mks) == 3
        for g, mk in enumerate(mks):
            _same(mk, wants[g], (n, "many", what, g))
    codes = [A, NONE, 2]
    parts = watch(lambda: ix.make_masks_partition(0, codes), mask_partition=3)
    assert len(parts) == 3
    for g, mk in enumerate(parts):
        single = watch(lambda: ix.make_mask_where([(0, codes[g])]), mask_where=1)
        _same(mk, _pack(cols[0] == codes[g]), (n, "many", "partition", g))
        _same(mk, single.rows(), (n, "partition against where", g))
