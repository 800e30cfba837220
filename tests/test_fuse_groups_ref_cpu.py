"""CPU: tests/fuse_groups_ref.py, the reference of the document-level fused search, on cases computed by hand, against a brute-force
restatement (dense S x groups matrices) on random lists, against fuse_ref.fuse when every row is its own group, and labels.fuse_groups
(the host fallback of VecDB.search_fused(group_by=)) against the reference -- the GPU tests compare the library against a reference that
is verified here first.  Nothing of the compiled library is used."""
import numpy as np

import fuse_ref
from fuse_groups_ref import LABEL_NONE, MIN, NAN_BITS, RRF, SUM, bits, fuse_groups, label_groups, order_key

F = np.float32
NONE = LABEL_NONE


def _l(ids, dists=None):
    return list(ids), list(dists if dists is not None else [float(i) for i in range(len(ids))])


def _b(sc):
    return [bits(x) for x in sc]


# rows 0 .. 9; labels: rows 0, 1, 2 -> document 0, rows 3, 4 -> document 1, row 5 -> document 5, rows 6, 7 unlabelled, rows 8, 9 -> document 2
LAB = np.array([0, 0, 0, 1, 1, 5, NONE, NONE, 2, 2], dtype=np.uint32)
G = label_groups(LAB)


def test_group_rank_is_not_row_position():
    # one list: rows 0, 1, 2 (document 0) then row 3 (document 1): document 1 sits at ROW position 3 and GROUP rank 1
    ids, sc, ex = fuse_groups([_l([0, 1, 2, 3])], G, 5, RRF, c=0.0)
    assert ids.tolist() == [0, 3] and _b(sc) == [bits(F(1.0)), bits(F(1.0) / F(2.0))] and ex == 1
    assert bits(fuse_ref.fuse([_l([0, 1, 2, 3])], 5, "rrf", c=0.0)[1][3]) == bits(F(1.0) / F(4.0))  # the row-level fusion sees position 3


def test_a_document_covering_two_sub_questions_is_credited_for_both():
    # document 0 answers list 0 with row 0 and list 1 with row 2; document 1 holds rank 0 of list 1 only
    lists = [_l([0, 5], [1.0, 2.0]), _l([3, 2], [0.5, 0.75])]
    ids, sc, _ = fuse_groups(lists, G, 5, RRF, c=60.0)
    s0 = F(F(F(0.0) + F(F(1.0) / F(61.0))) + F(F(1.0) / F(62.0)))
    assert ids.tolist() == [2, 3, 5]  # the representative of document 0 is row 2: its nearest row over the lists (0.75 < 1.0)
    assert _b(sc) == [bits(s0), bits(F(1.0) / F(61.0)), bits(F(1.0) / F(62.0))]
    ids, sc, _ = fuse_groups(lists, G, 5, MIN)
    assert ids.tolist() == [3, 2, 5] and sc.tolist() == [0.5, 0.75, 2.0]


def test_fold_order_and_weights():
    lists = [_l([0]), _l([1]), _l([2])]  # three rows of document 0, rank 0 of every list
    _, a, _ = fuse_groups(lists, G, 1, RRF, weights=[1e8, 3.0, 3.0], c=0.0)
    _, b, _ = fuse_groups(lists, G, 1, RRF, weights=[3.0, 3.0, 1e8], c=0.0)
    assert bits(a[0]) == bits(F(1e8)) and bits(b[0]) == bits(F(1e8) + F(8.0))  # (1e8 + 3) + 3 against (3 + 3) + 1e8


def test_sum_fill_prefix_and_fold_order():
    # document 1 is first seen in the LAST list: it starts from (0 + f_0) + f_1, then adds its own distance
    lists = [_l([0, 5], [1e8, 3.0]), _l([1], [3.0]), _l([3, 0], [1.0, 2.0])]
    ids, sc, ex = fuse_groups(lists, G, 5, SUM)
    d1 = F(F(F(F(0.0) + F(3.0)) + F(3.0)) + F(1.0))        # f_0 = 3, f_1 = 3, then 1
    d0 = F(F(F(F(0.0) + F(1e8)) + F(3.0)) + F(2.0))        # in every list: (1e8 + 3) + 2 = 1e8
    d5 = F(F(F(F(0.0) + F(3.0)) + F(3.0)) + F(2.0))        # list 0, then f_1 = 3, then f_2 = 2
    assert ids.tolist() == [3, 5, 0] and _b(sc) == [bits(d1), bits(d5), bits(d0)] and ex == 1  # (document 0's nearest row: row 0 at 2.0)
    assert bits(d0) == bits(F(1e8))
    # the same terms in another list order give other bits: the fold is ordered
    ids2, sc2, _ = fuse_groups([lists[2], lists[1], lists[0]], G, 5, SUM)
    assert bits(sc2[ids2.tolist().index(0)]) ==bits(F(F(F(2.0) + F(3.0)) + F(1e8))) != bits(d0)


def test_an_empty_list_is_skipped_in_every_fold():
    full = [_l([0, 3], [1.0, 2.0]), _l([3], [0.5])]
    holed = [full[0], _l([]), full[1], _l([])]
    for mode in (RRF, MIN, SUM):
        a, b = fuse_groups(full, G, 5, mode, trunc_len=2), fuse_groups(holed, G, 5, mode, trunc_len=2)
        assert a[0].tolist() == b[0].tolist() and _b(a[1]) == _b(b[1]) and a[2] == b[2] == 0
    ids, sc, ex = fuse_groups([_l([]), _l([])], G, 3, SUM, trunc_len=1)
    assert ids.size == 0 and sc.size == 0 and ex == 1  # no counted entry: nothing is truncated
    # RRF keeps the weight of the list's own number
    _, sc, _ = fuse_groups(holed, G, 5, RRF, weights=[1.0, 7.0, 2.0, 7.0], c=0.0)
    assert bits(sc[0]) == bits(F(F(F(0.0) + F(F(1.0) / F(2.0))) + F(F(2.0) / F(1.0))))


def test_a_nan_fill_and_negative_zero():
    nan = np.array(0xFFC00123, dtype=np.uint32).view(np.float32)[()]
    lists = [_l([0, 3], [1.0, nan]), _l([5], [-0.0])]  # f_0 is a NaN: every group list 0 lacks sums to NaN
    ids, sc, _ = fuse_groups(lists, G, 5, SUM)
    assert ids.tolist() == [0, 3, 5] and _b(sc) == [bits(F(1.0) + F(-0.0)), NAN_BITS, NAN_BITS]  # NaN last, ties by representative
    ids, sc, _ = fuse_groups(lists, G, 5, MIN)
    assert ids.tolist() == [5, 0, 3] and _b(sc) == [0x80000000, bits(F(1.0)), 0xFFC00123]  # MIN keeps the bits it found
    ids, sc, _ = fuse_groups([_l([0], [-0.0]), _l([3], [-0.0])], G, 5, SUM)
    assert _b(sc) == [0, 0]  # (+0 + -0) + -0 = +0 for both
    # -0 == +0 in the order: the representative stays with the first list
    ids, sc, _ = fuse_groups([_l([1], [0.0]), _l([0], [-0.0])], G, 5, MIN)
    assert ids.tolist() == [1] and _b(sc) == [0]


def test_key_spaces_are_distinct():
    # row 6 is unlabelled and 6 is no code here; row 5 carries code 5; unlabelled row 7 ... and a column in which row 5 is unlabelled
    lab = np.array([5, NONE, NONE, NONE, NONE, NONE, 0, 7], dtype=np.uint32)  # row 0 -> code 5; row 5 unlabelled; row 7 -> code 7
    g = label_groups(lab)
    ids, sc, _ = fuse_groups([_l([0, 5, 7, 1])], g, 9, RRF, c=0.0)
    assert ids.tolist() == [0, 5, 7, 1]  # code 5 and unlabelled row 5 are two groups
    ids, sc, _ = fuse_groups([_l([0, 5]), _l([5, 0])], g, 9, RRF, c=0.0)
    assert ids.tolist() == [0, 5] and bits(sc[0]) == bits(sc[1]) == bits(F(1.5))
    # a never-written column: every row its own group
    ids, _, _ = fuse_groups([_l([3, 4, 3])], label_groups(None), 9, MIN)
    assert ids.tolist() == [3, 4]
    assert label_groups(lab, id_offset=100)(105) == ("r", 5) and label_groups(lab, id_offset=100)(100) == ("l", 5)


def test_min_exactness_rule():
    # two lists of trunc_len 2: list 0 is truncated (f_0 = 2.0), list 1 is not
    lists = [_l([0, 3], [1.0, 2.0]), _l([5], [1.5])]
    assert fuse_groups(lists, G, 1, MIN, trunc_len=2)[2] == 1        # k-th score 1.0 < 2.0
    assert fuse_groups(lists, G, 2, MIN, trunc_len=2)[2] == 1        # 1.5 < 2.0
    assert fuse_groups(lists, G, 3, MIN, trunc_len=2)[2] == 0        # the third score IS f_0: a tie at f_s gives 0
    assert fuse_groups(lists, G, 4, MIN, trunc_len=2)[2] == 0        # count < k
    assert fuse_groups(lists, G, 4, MIN, trunc_len=3)[2] == 1        # nothing truncated
    assert fuse_groups(lists, G, 1, RRF, trunc_len=2)[2] == 0 and fuse_groups(lists, G, 1, SUM, trunc_len=2)[2] == 0
    assert fuse_groups(lists, G, 1, RRF, trunc_len=3)[2] == 1 and fuse_groups(lists, G, 1, SUM, trunc_len=None)[2] == 1
    # two truncated lists: the smaller f decides
    two = [_l([0, 3], [1.0, 2.0]), _l([5, 8], [0.5, 1.0])]
    assert fuse_groups(two, G, 1, MIN, trunc_len=2)[2] == 1 and fuse_groups(two, G, 2, MIN, trunc_len=2)[2] == 0  # 1.0 is f_1
    # -0 against +0 is a tie as well
    assert fuse_groups([_l([0, 3], [-0.0, 0.0])], G, 1, MIN, trunc_len=2)[2] == 0
    assert fuse_groups(lists, G, 0, MIN, trunc_len=2)[2] == 0 and fuse_groups(lists, G, 0, RRF, trunc_len=9)[2] == 0  # k == 0: nothing is ranked


def test_representative_and_ties():
    # document 0: 1.0 in list 0 (row 1) and 1.0 in list 1 (row 0): the earlier list keeps the representative
    ids, _, _ = fuse_groups([_l([1], [1.0]), _l([0], [1.0])], G, 5, SUM)
    assert ids.tolist() == [1]
    # equal scores: the lower representative first, in all three modes
    for mode in (RRF, MIN, SUM):
        ids, sc, _ = fuse_groups([_l([8, 3], [1.0, 1.0]), _l([4, 9], [1.0, 1.0])], G, 5, mode, c=0.0)
        # (RRF: document 1 scores 1/2 + 1/1, document 2 1/1 + 1/2; both keep the row of list 0 as representative: the earlier list on a tie)
        assert ids.tolist() == [3, 8] and bits(sc[0]) == bits(sc[1])
    # a repeat of a group inside a list counts once, at its first position, whatever the later distance
    ids, sc, _ = fuse_groups([_l([0, 1, 3, 2], [5.0, 1.0, 6.0, 0.5])], G, 5, MIN)
    assert ids.tolist() == [0, 3] and sc.tolist() == [5.0, 6.0]


def _brute(lists, gid, n_groups, k, mode, weights, c, trunc_len):
    """the rule over dense S x groups matrices of first positions (-1: absent), group ranks by counting"""
    S = len(lists)
    pos = np.full((S, n_groups), -1, dtype=np.int64)
    row = np.zeros((S, n_groups), dtype=np.int64)
    dd = np.zeros((S, n_groups), dtype=np.float32)
    for s, (ids, dists) in enumerate(lists):
        for p in range(len(ids) - 1, -1, -1):  # backwards: the first occurrence is written last
            g = gid[ids[p]]
            pos[s, g], row[s, g], dd[s, g] = p, ids[p], dists[p]
    live = [s for s in range(S) if len(lists[s][0])]
    out = []
    with np.errstate(all="ignore"):
        for g in range(n_groups):
            held = [s for s in live if pos[s, g] >= 0]
            if not held:
                continue
            best = min(held, key=lambda s: (order_key(dd[s, g]), s))
            a = F(0.0)
            for s in live:
                if mode == RRF and pos[s, g] >= 0:
                    rho = int(((pos[s] >= 0) & (pos[s] < pos[s, g])).sum())
                    a = F(a + F(F(weights[s]) / F(F(rho + 1) + F(c))))
                elif mode == SUM:
                    a = F(a + (dd[s, g] if pos[s, g] >= 0 else F(lists[s][1][-1])))
            if mode == MIN:
                a = dd[best, g]
            key = order_key(-a) if mode == RRF else order_key(a)
            out.append((key, int(row[best, g]), NAN_BITS if mode == SUM and np.isnan(a) else bits(a)))
    out.sort(key=lambda t: (t[0], t[1]))
    trunc = [order_key(lists[s][1][-1]) for s in live if len(lists[s][0]) >= trunc_len]
    exact = k > 0 and (not trunc or (mode == MIN and k <= len(out) and all(out[k - 1][0] < t for t in trunc)))
    out = out[:k]
    return [t[1] for t in out], [t[2] for t in out], int(exact)


def _random_case(rng, n):
    lab = rng.integers(0, 12, size=n).astype(np.uint32)
    lab[rng.random(n) < 0.2] = NONE
    gid, names = np.zeros(n, dtype=np.int64), {}
    g = label_groups(lab)
    for r in range(n):
        gid[r] = names.setdefault(g(r), len(names))
    S = int(rng.integers(1, 7))
    lists = []
    for s in range(S):
        m = int(rng.integers(0, 40))
        ids = rng.integers(0, n, size=m).tolist()  # with repeats
        d = rng.choice(np.array([0.0, -0.0, 1.0, 2.5, 7.0, np.inf, np.nan, -1.0], dtype=np.float32), size=m)
        lists.append((ids, d.tolist()))
    return lab, gid, len(names), lists


def test_against_the_dense_restatement_on_random_lists():
    rng = np.random.default_rng(15)
    n = 60
    for trial in range(40):
        lab, gid, ng, lists = _random_case(rng, n)
        S = len(lists)
        w = rng.uniform(1e-3, 1e3, size=S).astype(np.float32).tolist()
        c = float(rng.choice([0.0, 1.0, 60.0]))
        tl = int(rng.integers(1, 40))
        for k in (1, 5, 100):
            for mode in (RRF, MIN, SUM):
                ids, sc, ex = fuse_groups(lists, label_groups(lab), k, mode, weights=w if mode == RRF else None, c=c, trunc_len=tl)
                assert (ids.tolist(), _b(sc), ex) == _brute(lists, gid, ng, k, mode, w, c, tl), (trial, k, mode)


def test_every_row_its_own_group_is_the_row_level_fusion():
    """MIN always; RRF when no id occurs twice in a list (what a search returns): the row-level fusion ranks a row by its POSITION, which
    counts the repeats before it, the group-level one by the distinct groups before it"""
    rng = np.random.default_rng(16)
    for trial in range(20):
        _, _, _, lists = _random_case(rng, 60)
        once = [(list(dict.fromkeys(ids)), d[:len(set(ids))]) for ids, d in lists]
        w = rng.uniform(0.5, 2.0, size=len(lists)).astype(np.float32).tolist()
        for lab in (None, np.full(60, NONE, dtype=np.uint32)):
            for k in (1, 7, 100):
                a = fuse_groups(once, label_groups(lab), k, RRF, weights=w, c=60.0)
                b = fuse_ref.fuse(once, k, "rrf", w, 60.0)
                assert a[0].tolist() == b[0].tolist() and _b(a[1]) == _b(b[1])
                a, b = fuse_groups(lists, label_groups(lab), k, MIN), fuse_ref.fuse(lists, k, "min")
                assert a[0].tolist() == b[0].tolist() and _b(a[1]) == _b(b[1])
    a, b = fuse_groups([_l([3, 3, 6])], label_groups(None), 5, RRF, c=0.0), fuse_ref.fuse([_l([3, 3, 6])], 5, "rrf", c=0.0)
    assert _b(a[1]) == [bits(F(1.0)), bits(F(0.5))] and _b(b[1]) == [bits(F(1.0)), bits(F(1.0) / F(3.0))]  # ... and with a repeat they differ


def test_the_host_fallback_matches_the_reference():
    from lab_1806_vec_db_amd.labels import fuse_groups as host

    rng = np.random.default_rng(17)
    n = 60
    for trial in range(30):
        lab, _, _, lists = _random_case(rng, n)
        values = [None if c == NONE else "doc%d" % c for c in lab.tolist()]
        hl = [(np.asarray(ids, dtype=np.uint64), np.asarray(d, dtype=np.float32), [values[i] for i in ids]) for ids, d in lists]
        w = rng.uniform(0.5, 2.0, size=len(lists)).astype(np.float32)
        tl = int(rng.integers(1, 40))
        for k in (0, 1, 5, 100):
            for mode in (RRF, MIN, SUM):
                ww = w if mode == RRF else None
                a = fuse_groups(lists, label_groups(lab), k, mode, weights=ww, c=60.0, trunc_len=tl)
                b = host(hl, k, mode, ww, 60.0, trunc_len=tl)
                assert a[0].tolist() == b[0].tolist() and _b(a[1]) == _b(b[1]) and a[2] == b[2], (trial, k, mode)
