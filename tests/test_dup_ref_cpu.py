"""CPU: tests/dup_ref.py, the reference the GPU tests of the near-duplicate grouping compare against -- the union-find against the
brute-force restatement by label propagation on hand cases and random graphs, and the planted-copy tables: both margins around the test
radius verified in float64 for the seeds the GPU tests use."""
import numpy as np
import pytest

import dup_ref as R

NONE = R.ROW_NONE


def _both(n, lists, src=None, allowed=None, limit=0, id_offset=0):
    src = list(range(len(lists))) if src is None else src
    lims, ids = R.csr(lists)
    a = R.dup_ref(n, src, lims, ids, allowed, limit, id_offset)
    b = R.dup_brute(n, src, lims, ids, allowed, limit, id_offset)
    assert np.array_equal(a[0], b[0]) and a[1] == b[1], (a, b)
    return a


def test_path_and_reversed_path():
    n = 9
    g, st = _both(n, [[i, i + 1] for i in range(n - 1)] + [[n - 1]])
    assert g.tolist() == [0] * n and st == {"groups": 1, "rows": n, "pairs": n - 1, "truncated": 0}
    g, st = _both(n, [[0]] + [[i, i - 1] for i in range(1, n)])
    assert g.tolist() == [0] * n and st["pairs"] == n - 1
    # given from the far end first: the deep tree of a naive union
    src = list(range(n - 1, 0, -1))
    g, _ = _both(n, [[i - 1] for i in src], src=src)
    assert g.tolist() == [0] * n


def test_star():
    g, st = _both(6, [[0, 1, 2, 3, 4, 5]] + [[i] for i in range(1, 6)])
    assert g.tolist() == [0] * 6 and st == {"groups": 1, "rows": 6, "pairs": 5, "truncated": 0}
    g, _ = _both(6, [[i] for i in range(5)] + [[5, 0, 1, 2, 3, 4]])  # a star on the LAST row: the representative is still row 0
    assert g.tolist() == [0] * 6


def test_two_cliques_and_a_bridge():
    a, b = [1, 2, 3], [5, 6, 7, 8]
    lists = [[] for _ in range(10)]
    for c in (a, b):
        for i in c:
            lists[i] = [i] + [j for j in c if j != i]
    g, st = _both(10, lists)
    assert g.tolist() == [0, 1, 1, 1, 4, 5, 5, 5, 5, 9] and st["groups"] == 2 and st["rows"] == 7
    lists[3] = lists[3] + [5]  # the bridge, listed by one end only
    g, st = _both(10, lists)
    assert g.tolist() == [0, 1, 1, 1, 4, 1, 1, 1, 1, 9] and st["groups"] == 1 and st["rows"] == 7


def test_a_bridge_through_a_disallowed_row_does_not_link():
    # 0 - 1 - 2 with row 1 disallowed: under the mask neither list names it, and it is no query
    allowed = [True, False, True, True]
    g, st = _both(4, [[0], [2, 3], [3, 2]], src=[0, 2, 3], allowed=allowed)
    assert g.tolist() == [0, NONE, 2, 2] and st == {"groups": 1, "rows": 2, "pairs": 2, "truncated": 0}


def test_a_duplicated_edge_counts_twice_and_links_once():
    g, st = _both(3, [[0, 1, 1], [1, 0], [2]])
    assert g.tolist() == [0, 0, 2] and st == {"groups": 1, "rows": 2, "pairs": 3, "truncated": 0}


def test_a_cut_list():
    # row 0 lists itself and 1, 2, 3 in that order; limit 2 keeps [0, 1]: rows 2 and 3 stay out unless they list somebody themselves
    lists = [[0, 1, 2, 3], [1, 0], [2], [3, 2, 0]]
    g, st = _both(4, lists, limit=2)
    assert g.tolist() == [0, 0, 2, 2] and st == {"groups": 2, "rows": 4, "pairs": 3, "truncated": 3}
    full, _ = _both(4, lists)
    assert full.tolist() == [0, 0, 0, 0]
    for i in range(4):  # a cut group is a subset of a true one
        assert set(np.flatnonzero(g == g[i])) <= set(np.flatnonzero(full == full[i]))
    g, st = _both(4, lists, id_offset=100)
    assert g.tolist() == [100] * 4


@pytest.mark.parametrize("seed", range(12))
def test_random_graphs(seed):
    rng = np.random.default_rng(seed)
    n = int(rng.integers(1, 60))
    allowed = rng.random(n) < 0.8 if seed % 3 == 0 else None
    rows = np.flatnonzero(allowed) if allowed is not None else np.arange(n)
    lists = []
    for i in rows.tolist():
        deg = int(rng.integers(0, 4)) if rng.random() < 0.6 else 0
        lists.append([i] * int(rng.integers(0, 2)) + rng.choice(rows, size=deg).tolist())
    limit = int(rng.integers(0, 4)) if seed % 2 else 0
    g, st = _both(n, lists, src=rows.tolist(), allowed=allowed, limit=limit, id_offset=7 * (seed % 2))
    assert g.shape == (n,) and st["rows"] >= 2 * st["groups"]


@pytest.mark.parametrize("kind", ("f32", "u8"))
def test_planted_table_margins_in_float64(kind):
    n, dim = 20000, 128
    x, radius, truth, pairs, chains = R.planted_table(n, dim, kind, R.PLANTED_SEEDS[kind])
    assert x.dtype == (np.uint8 if kind == "u8" else np.float32) and x.shape == (n, dim)
    x64 = x.astype(np.float64)
    # every planted pair inside the radius by a factor of 2
    d = ((x64[pairs[:, 0]] - x64[pairs[:, 1]]) ** 2).sum(axis=1)
    assert d.max() * 2 <= radius and d.min() > 0
    # every other pair outside it by a factor of 2: candidates from the Gram form, decided by the direct sum
    planted = set(map(tuple, np.sort(pairs, axis=1).tolist()))
    sq = (x64 ** 2).sum(axis=1)
    near = 0
    for a in range(0, n, 2000):
        g = sq[a:a + 2000, None] + sq[None, :] - 2.0 * (x64[a:a + 2000] @ x64.T)
        ii, jj = np.nonzero(g < 2 * radius * (1 + 1e-6) + 1e-9)
        for i, j in zip((ii + a).tolist(), jj.tolist()):
            if i < j and (i, j) not in planted:
                near += 1
                assert ((x64[i] - x64[j]) ** 2).sum() >= 2 * radius, (i, j)
    assert near >= sum(max(len(c) - 2, 0) for c in chains)  # (the chains' rows two apart sit exactly at twice the radius)
    # the truth: 200 groups, their sizes 2 .. 6, chains among them with ends farther apart than the radius
    reps, counts = np.unique(truth, return_counts=True)
    assert (counts >= 2).sum() == 200 and counts.max() <= 6 and len(chains) >= 50
    assert any(len(c) >= 3 and ((x64[c[0]] - x64[c[-1]]) ** 2).sum() > radius for c in chains)
    assert all(truth[i] == min(c) for c in chains for i in c)
