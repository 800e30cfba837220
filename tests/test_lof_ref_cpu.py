"""CPU: tests/lof_ref.py on cases worked out by hand, before any GPU test leans on it."""
import numpy as np

import lof_ref as R


def test_four_collinear_points_by_hand():
    """0, 1, 2, 10 on a line, k = 2.  N(0) = {1, 2}, N(1) = {0, 2} (a tie at distance 1: the lower index first), N(2) = {1, 0}, N(10) = {2, 1};
    kdist = 2, 1, 2, 9.  Mean reach: (max(1, 1) + max(2, 2)) / 2, (max(2, 1) + max(2, 1)) / 2, (max(1, 1) + max(2, 2)) / 2, (max(2, 8) + max(1, 9)) / 2."""
    x = np.array([0, 1, 2, 10], dtype=np.float32)
    rows, kdist, lrd, lof = R.of_matrix(np.abs(x[:, None] - x[None, :]), 2)
    assert rows.tolist() == [0, 1, 2, 3] and kdist.tolist() == [2, 1, 2, 9]
    a, b, c, d = 1 / 1.5, 1 / 2.0, 1 / 1.5, 1 / 8.5
    assert np.allclose(lrd, [a, b, c, d], rtol=1e-9, atol=0)
    assert np.allclose(lof, [(b + c) / 2 / a, (a + c) / 2 / b, (b + a) / 2 / c, (c + b) / 2 / d], rtol=1e-9, atol=0)  # 7/8, 4/3, 7/8, 119/24


def test_identical_rows_and_a_single_row():
    _, kdist, lrd, lof = R.of_matrix(np.zeros((7, 7), dtype=np.float32), 3)
    assert (kdist == 0).all() and np.allclose(lrd, 1e10, rtol=1e-12) and (lof == 1.0).all()  # every reach is 0
    _, kdist, lrd, lof = R.of_matrix(np.zeros((1, 1), dtype=np.float32), 3)
    assert np.isnan(kdist).all() and np.isnan(lrd).all() and np.isnan(lof).all()  # kk = 0


def test_planted_far_points_and_a_mask():
    rng = np.random.default_rng(3)
    x = rng.standard_normal((200, 8))
    x[[11, 50, 190]] += 40 * np.eye(8)[[0, 1, 2]]
    D = ((x[:, None, :] - x[None, :, :]) ** 2).sum(axis=2).astype(np.float32)
    rows, _, _, lof = R.of_matrix(D, 10)
    assert sorted(np.argsort(-lof)[:3].tolist()) == [11, 50, 190] and np.sort(lof)[-3] > 2 * np.sort(lof)[-4]
    allowed = np.arange(200) % 2 == 0  # under a mask: the scores of the sub-table, at the rows' positions
    sub = R.of_matrix(D[allowed][:, allowed], 10)
    got = R.of_matrix(D, 10, allowed)
    assert got[0].tolist() == np.flatnonzero(allowed).tolist() and all(np.array_equal(a, b, equal_nan=True) for a, b in zip(got[1:], sub[1:]))
