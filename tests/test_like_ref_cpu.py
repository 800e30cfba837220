"""CPU: tests/like_ref.py, the reference of the search by example rows, on cases computed by hand -- the GPU tests compare the library
against a reference that is verified here first.  Nothing of the library is used."""
import numpy as np

from like_ref import drop_listed, like_queries, like_query, same_floats

F = np.float32


def _bits(x):
    return np.asarray(x, dtype=np.float32).view(np.uint32).tolist()


def test_one_positive_is_the_row_with_negative_zero_made_positive():
    rows = np.array([[1.5, -0.0, 0.0, -2.25, 1e-42, 3e38]], dtype=np.float32)
    q = like_query(rows, [0])
    assert _bits(q) == _bits([1.5, 0.0, 0.0, -2.25, 1e-42, 3e38])  # (+0.0) + (-0.0) = +0.0; x / 1 = x
    assert not np.signbit(q[1])


def test_fold_order_is_visible():
    rows = np.array([[1e8], [1.0], [-1e8]], dtype=np.float32)
    # (1e8 + 1) rounds to 1e8 in f32, so the first order loses the 1 and the second keeps it
    assert _bits(like_query(rows, [0, 1, 2])) == _bits([F(0.0) / F(3.0)]) == [0]
    assert _bits(like_query(rows, [0, 2, 1])) == _bits([F(1.0) / F(3.0)])


def test_divide_rounds_at_three():
    rows = np.array([[1.0], [1.0], [2.0], [0.1]], dtype=np.float32)
    q = like_query(rows, [0, 1, 2])
    assert _bits(q) == _bits([F(4.0) / F(3.0)]) == [0x3FAAAAAB]
    q = like_query(rows, [3, 3, 3])  # (0.1f + 0.1f) + 0.1f = 0.3f rounded once per add, then / 3: not 0.1f again in general
    s = F(F(F(0.1) + F(0.1)) + F(0.1))
    assert _bits(q) == _bits([F(s / F(3.0))])


def test_negatives_and_overflow_of_twice_ap():
    rows = np.array([[3e38, 1.0], [3e38, 3.0], [1.0, 10.0]], dtype=np.float32)
    q = like_query(rows, [0, 1], [2])
    # element 0: sp = 3e38 + 3e38 = inf already; element 1: ap = 2, an = 10 -> 4 - 10
    assert np.isposinf(q[0]) and q[1] == F(-6.0)
    rows = np.array([[2e38], [1e38]], dtype=np.float32)
    q = like_query(rows, [0], [1])  # ap = 2e38 is finite, ap + ap overflows to +inf, inf - 1e38 = inf
    assert np.isposinf(q[0])
    q = like_query(rows, [1], [0])  # 2e38 - 2e38 = 0
    assert _bits(q) == [0]


def test_nan_and_inf_rows():
    rows = np.array([[np.nan, np.inf, np.inf, 1.0], [1.0, -np.inf, np.inf, np.inf], [0.0, 0.0, np.inf, np.inf]], dtype=np.float32)
    q = like_query(rows, [0, 1])
    assert np.isnan(q[0]) and np.isnan(q[1]) and np.isposinf(q[2]) and np.isposinf(q[3])
    q = like_query(rows, [0, 1], [2])
    assert np.isnan(q[0]) and np.isnan(q[1]) and np.isnan(q[2]) and np.isnan(q[3])  # inf - inf
    assert same_floats(q, np.full(4, -np.nan, dtype=np.float32)) and not same_floats(q, np.zeros(4, dtype=np.float32))
    assert same_floats(np.array([1.0, -0.0]), np.array([1.0, -0.0])) and not same_floats(np.array([0.0]), np.array([-0.0]))


def test_repeats_weight_a_row():
    rows = np.array([[1.0, 8.0], [4.0, 2.0]], dtype=np.float32)
    assert like_query(rows, [0, 0, 1]).tolist() == [2.0, 6.0]
    assert like_query(rows, [0, 1]).tolist() == [2.5, 5.0]
    assert like_query(rows, [1], [0, 0]).tolist() == [7.0, -4.0]
    qs = like_queries(rows, [[0, 0, 1], [1]], [[], [0, 0]])
    assert qs.tolist() == [[2.0, 6.0], [7.0, -4.0]]


def test_drop_walk_against_set_difference():
    rng = np.random.default_rng(5)
    for _ in range(300):
        n = int(rng.integers(0, 40))
        ids = rng.integers(0, 25, size=n)  # (repeats in the list: every copy of a listed id goes)
        listed = rng.integers(0, 25, size=int(rng.integers(0, 12)))
        k = int(rng.integers(0, 45))
        kept = drop_listed(ids, listed, k)
        brute = [p for p in range(n) if ids[p] not in set(listed.tolist())][:k]
        assert kept == brute
    assert drop_listed([5, 3, 5, 7, 3, 9], [3], 3) == [0, 2, 3]
    assert drop_listed([5, 3, 5], [5, 3], 2) == [] and drop_listed([], [1], 4) == [] and drop_listed([1, 2], [], 0) == []
