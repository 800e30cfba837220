"""CPU: tests/fuse_ref.py, the reference of the fused multi-query search, on cases computed by hand, against a brute-force restatement
(a dense S x n rank matrix) on random lists, and the MIN-is-exact property on a small random table -- the GPU tests compare the library
against a reference that is verified here first.  Nothing of the library is used."""
import numpy as np

from fuse_ref import MIN, RRF, bits, fuse, order_key, padded

F = np.float32


def _l(ids, dists=None):
    return list(ids), list(dists if dists is not None else [0.0] * len(ids))


def test_two_lists_sharing_one_row():
    ids, sc = fuse([_l([7, 3]), _l([9, 7])], 10, RRF, c=60.0)
    # 7: 1/61 + 1/62;  3: 1/62;  9: 1/61
    s7 = F(F(0.0) + F(F(1.0) / F(61.0))) + F(F(1.0) / F(62.0))
    assert ids.tolist() == [7, 9, 3]
    assert [bits(x) for x in sc] == [bits(F(s7)), bits(F(1.0) / F(61.0)), bits(F(1.0) / F(62.0))]


def test_fold_order_across_three_lists_with_weights():
    # row 5 sits at rank 0 of every list; the weights make the order of the additions visible: the ulp of f32 at 1e8 is 8
    w = [1e8, 3.0, 3.0]
    ids, sc = fuse([_l([5]), _l([5]), _l([5])], 1, RRF, weights=w, c=0.0)
    assert ids.tolist() == [5] and bits(sc[0]) == bits(F(1e8))  # (1e8 + 3) + 3: each 3 is rounded away
    ids2, sc2 = fuse([_l([5]), _l([5]), _l([5])], 1, RRF, weights=[3.0, 3.0, 1e8], c=0.0)
    assert bits(sc2[0]) == bits(F(1e8) + F(8.0)) != bits(sc[0])  # (3 + 3) + 1e8: the 6 rounds up to one ulp


def test_divide_and_denominator_round_once_each():
    # c = 0.1: den = f32(f32(3) + f32(0.1)), term = f32(2 / den)
    ids, sc = fuse([_l([1, 2, 4])], 3, RRF, weights=[2.0], c=0.1)
    assert ids.tolist() == [1, 2, 4]
    for p, s in enumerate(sc):
        assert bits(s) == bits(F(F(2.0) / F(F(p + 1) + F(0.1))))


def test_a_tie_is_broken_by_row_id():
    ids, sc = fuse([_l([9, 1]), _l([4, 8])], 4, RRF, c=1.0)
    assert ids.tolist() == [4, 9, 1, 8] and bits(sc[0]) == bits(sc[1]) == bits(F(0.5)) and bits(sc[2]) == bits(sc[3])
    ids, sc = fuse([_l([9, 1], [2.0, 2.0]), _l([4, 8], [2.0, 1.0])], 4, MIN)
    assert ids.tolist() == [8, 1, 4, 9]


def test_a_repeat_inside_a_list_counts_once_at_its_first_position():
    ids, sc = fuse([_l([3, 3, 6, 3])], 5, RRF, c=0.0)
    assert ids.tolist() == [3, 6] and bits(sc[0]) == bits(F(1.0)) and bits(sc[1]) == bits(F(1.0) / F(3.0))  # 6 keeps rank 2
    ids, sc = fuse([_l([3, 3, 6], [5.0, 1.0, 2.0])], 5, MIN)
    assert ids.tolist() == [6, 3] and sc.tolist() == [2.0, 5.0]  # the later, smaller distance of the repeat does not count


def test_c_zero():
    ids, sc = fuse([_l([1, 2]), _l([2, 1])], 2, RRF, c=0.0)
    assert ids.tolist() == [1, 2] and bits(sc[0]) == bits(sc[1]) == bits(F(1.5))


def test_min_with_nan_and_signed_zeros_keeps_the_first_lists_bits():
    nan1 = np.array(0x7FC00001, dtype=np.uint32).view(np.float32)
    nan2 = np.array(0xFFC00002, dtype=np.uint32).view(np.float32)
    lists = [
        _l([1, 2, 3, 4, 5], [nan1, -0.0, 0.0, np.inf, nan1]),
        _l([1, 2, 3, 4, 5, 6], [nan2, 0.0, -0.0, -np.inf, 7.0, nan2]),
    ]
    ids, sc = fuse(lists, 10, MIN)
    # -inf < -0 == +0 < 7 < NaN == NaN; ties by id; 2 and 3 keep the bits of list 0 (the first that attains the minimum)
    assert ids.tolist() == [4, 2, 3, 5, 1, 6]
    assert [bits(x) for x in sc] == [bits(F(-np.inf)), 0x80000000, 0x00000000, bits(F(7.0)), 0x7FC00001, 0xFFC00002]
    assert order_key(nan1) == order_key(nan2) > order_key(np.inf) and order_key(-0.0) == order_key(0.0)


def test_k_above_the_union_and_an_empty_list_among_full_ones():
    ids, sc = fuse([_l([4, 2]), _l([]), _l([2])], 7, RRF, c=60.0)
    assert ids.tolist() == [2, 4]
    s2 = F(F(F(0.0) + F(F(1.0) / F(62.0))) + F(F(1.0) / F(61.0)))  # list 0 at rank 1, then list 2 at rank 0 (s stays the list's number)
    assert bits(sc[0]) == bits(s2)
    oi, ob, cnt = padded(ids, sc, 7)
    assert cnt == 2 and oi.tolist() == [2, 4, 0, 0, 0, 0, 0] and ob[2:].tolist() == [0] * 5
    assert fuse([_l([]), _l([])], 3, MIN)[0].size == 0 and fuse([_l([1])], 0, RRF)[0].size == 0


def _brute(lists, n, k, mode, weights, c):
    """the rule over a dense S x n matrix of first positions (-1: absent)"""
    S = len(lists)
    pos = np.full((S, n), -1, dtype=np.int64)
    dd = np.zeros((S, n), dtype=np.float32)
    for s, (ids, dists) in enumerate(lists):
        for p in range(len(ids) - 1, -1, -1):  # backwards: the first occurrence is written last
            pos[s, ids[p]] = p
            dd[s, ids[p]] = dists[p]
    out = []
    for r in range(n):
        if (pos[:, r] < 0).all():
            continue
        if mode == RRF:
            a = F(0.0)
            for s in range(S):
                if pos[s, r] >= 0:
                    a = F(a + F(F(weights[s]) / F(F(pos[s, r] + 1) + F(c))))
            out.append((order_key(-a), r, a))
        else:
            best = None
            for s in range(S):
                if pos[s, r] >= 0 and (best is None or order_key(dd[s, r]) < order_key(best)):
                    best = dd[s, r]
            out.append((order_key(best), r, best))
    out.sort(key=lambda t: (t[0], t[1]))
    out = out[:k]
    return [t[1] for t in out], [bits(t[2]) for t in out]


def test_against_the_dense_restatement_on_random_lists():
    rng = np.random.default_rng(5)
    n = 60
    for trial in range(40):
        S = int(rng.integers(1, 7))
        lists = []
        for s in range(S):
            m = int(rng.integers(0, 50))
            ids = rng.integers(0, n, size=m).tolist()  # with repeats
            d = rng.choice(np.array([0.0, -0.0, 1.0, 2.5, np.inf, np.nan, -1.0], dtype=np.float32), size=m)
            lists.append((ids, d.tolist()))
        w = rng.uniform(1e-3, 1e3, size=S).astype(np.float32).tolist()
        c = float(rng.choice([0.0, 1.0, 60.0]))
        for k in (1, 5, 100):
            ids, sc = fuse(lists, k, RRF, weights=w, c=c)
            assert (ids.tolist(), [bits(x) for x in sc]) == _brute(lists, n, k, RRF, w, c), trial
            ids, sc = fuse(lists, k, MIN)
            assert (ids.tolist(), [bits(x) for x in sc]) == _brute(lists, n, k, MIN, None, 0.0), trial


def test_min_is_the_exact_nearest_to_any_sub_query_with_fetch_k_equal_to_k():
    """fetch_k = k lists, fused, against the full order of min over the sub-queries of the distance -- with ties and duplicates"""
    rng = np.random.default_rng(8)
    n, S = 200, 4
    for trial in range(10):
        D = rng.integers(0, 30, size=(S, n)).astype(np.float32)  # many ties, within and across sub-queries
        allowed = rng.random((S, n)) < 0.6
        for k in (1, 3, 10, 50):
            lists = []
            for s in range(S):
                rows = [r for r in range(n) if allowed[s, r]]
                rows.sort(key=lambda r: (order_key(D[s, r]), r))
                rows = rows[:k]  # fetch_k = k
                lists.append((rows, [D[s, r] for r in rows]))
            ids, sc = fuse(lists, k, MIN)
            full = [(min(order_key(D[s, r]) for s in range(S) if allowed[s, r]), r) for r in range(n) if allowed[:, r].any()]
            full.sort()
            assert ids.tolist() == [r for _, r in full[:k]], (trial, k)
            assert [order_key(x) for x in sc] == [o for o, _ in full[:k]]
