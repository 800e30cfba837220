"""The reference of the density clustering, plain Python / numpy over CSR neighbour lists with distances or a distance matrix: kinds from
list lengths, a union-find over core-core pairs named by the lowest core row, border rows by the minimum (np.float32 distance, row)."""
import numpy as np

import dup_ref

ROW_NONE, ROW_NOISE = 2 ** 64 - 1, 2 ** 64 - 2
STATS = ("clusters", "core", "border", "noise", "pairs")
COUNTERS = ("flat_dbscan_calls", "flat_dbscan_chunks", "flat_dbscan_pairs")


def csr(lists):
    """(lims uint64 [nq + 1], ids uint64, dists float32) of a list of lists of (id, distance)"""
    return dup_ref.csr([[j for j, _ in x] for x in lists]) + (np.array([d for x in lists for _, d in x], dtype=np.float32),)


def lists_of_edges(n, edges):
    """(src, lists): both ends of every edge (i, j, d) list the other, every row lists itself at 0, lists ascending by (distance, row)"""
    D = np.where(np.eye(n, dtype=bool), np.float32(0), np.float32(np.nan))
    for i, j, d in edges:
        D[i, j] = D[j, i] = d
    return lists_of_matrix(D, np.inf)


def lists_of_matrix(D, eps, allowed=None):
    """(src, lists) from a float32 distance matrix: per allowed row its allowed rows with D <= eps (never a NaN), by (distance, row)"""
    ok, lists = np.ones(len(D), dtype=bool) if allowed is None else np.asarray(allowed, dtype=bool), []
    for i in np.flatnonzero(ok).tolist():
        with np.errstate(invalid="ignore"):
            js = np.flatnonzero((D[i] <= np.float32(eps)) & ok)
        lists.append([(int(j), D[i][j]) for j in js[np.lexsort((js, D[i][js]))]])
    return np.flatnonzero(ok).tolist(), lists


_PATH = [(0, 1, 1), (1, 2, 1), (2, 3, 1), (3, 4, 1)]
_TWO = [(0, 1, 1), (0, 5, 1), (3, 4, 1), (3, 6, 1), (3, 2, 1)]  # cores 0 and 3 (4 entries each with the edge to row 2), row 2 between them
HAND_CASES = [  # answers written down by hand: (name, rows, min_samples, edges, label, kind); every row also lists itself
    ("a path: the inner rows are core, the ends border", 5, 3, _PATH, [1] * 5, [2, 3, 3, 3, 2]),
    ("a star: the hub is core, the leaves border", 5, 5, [(0, k, 1) for k in range(1, 5)], [0] * 5, [3, 2, 2, 2, 2]),
    ("the nearer core wins though it is the higher row", 7, 4, _TWO + [(0, 2, 2)], [0, 0, 3, 3, 3, 0, 3], [3, 2, 2, 3, 2, 2, 2]),
    ("equal distances go to the lower row", 7, 4, _TWO + [(0, 2, 1)], [0, 0, 0, 3, 3, 0, 3], [3, 2, 2, 3, 2, 2, 2]),
    ("min_samples above every degree: all noise", 5, 4, _PATH, [ROW_NOISE] * 5, [1] * 5),
]


def dbscan_ref(n, src, lims, ids, dists, min_samples, allowed=None, id_offset=0):
    """(label uint64 [n], kind uint8 [n], stats dict): src / ids hold LOCAL rows"""
    ok = np.ones(n, dtype=bool) if allowed is None else np.asarray(allowed, dtype=bool)
    lists = {int(s): [(np.float32(dists[p]), int(ids[p])) for p in range(int(lims[q]), int(lims[q + 1]))] for q, s in enumerate(src)}
    bits = {(i, j): d.tobytes() for i, lst in lists.items() for d, j in lst}  # (asserted on every input: the lists are symmetric)
    assert all(bits.get((j, i)) == b for (i, j), b in bits.items()), "the lists are not symmetric"
    kind, parent, label = ok.astype(np.uint8), list(range(n)), np.full(n, ROW_NONE, dtype=np.uint64)
    kind[[i for i, lst in lists.items() if len(lst) >= min_samples]] = 3

    def find(x):
        while parent[x] != x:
            parent[x] = x = parent[parent[x]]
        return x

    for i, j in bits:
        if kind[i] == 3 and kind[j] == 3 and find(i) != find(j):
            parent[max(find(i), find(j))] = min(find(i), find(j))
    for i in np.flatnonzero(ok).tolist():
        cores = [(d, j) for d, j in lists.get(i, []) if kind[j] == 3 and j != i]
        kind[i] = 3 if kind[i] == 3 else 2 if cores else 1
        label[i] = find(i) + id_offset if kind[i] == 3 else find(min(cores)[1]) + id_offset if cores else ROW_NOISE
    counts = [len({find(i) for i in np.flatnonzero(kind == 3).tolist()})] + [int((kind == k).sum()) for k in (3, 2, 1)]
    return label, kind, dict(zip(STATS, counts + [sum(1 for i, j in bits if i != j)]))


def of_matrix(D, eps, min_samples, allowed=None, id_offset=0):
    src, lists = lists_of_matrix(D, eps, allowed)
    return dbscan_ref(len(D), src, *csr(lists), min_samples, allowed, id_offset)


def same(got, want):
    assert got[2] == want[2] and got[0].dtype == np.uint64 and got[1].dtype == np.uint8, (got[2], want[2])
    assert np.array_equal(got[1], want[1]) and np.array_equal(got[0], want[0]), np.flatnonzero(got[0] != want[0])[:8]
