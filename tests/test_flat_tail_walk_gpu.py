"""GPU parity: the two walks of the 8-bit pass's exact stage (k_flat_tail_lb, parameter "flat_tail_lb_walk").

Walk 1 selects the 64 smallest open keys anew in every round and fetches every row of a round.  Walk 0 (the default) serves four rounds
from one selection of 256 keys and, in rounds after the first, does not fetch rows that the k-th exact distance so far already excludes.
The rounds, the candidates that matter and every certification are the same, so everything a caller can observe must be the same bits:
indices, distances, counts, what is handed on (flat_i8_redo, flat_i8_second_queries) and, with flat_i8_stats, the histogram of rounds
walked and the hit counts.  Walk 0 is also held to the oracle.  (flat_i8_rows_walked is not maintained by the library: not compared.)
"""
import numpy as np
import pytest

from conftest import gist_like

pytestmark = pytest.mark.gpu

NWS = (40, 41, 8, 4, 2, 1)


@pytest.fixture(scope="module")
def mods():
    import lab_1806_vec_db_amd as vdb
    from oracle import oracle as O
    return vdb, O


def _check_all(idx, d, cnt, oi, od, oc, nan_ok=False):
    assert cnt.tolist() == oc.tolist()
    for q in range(idx.shape[0]):
        assert idx[q].tolist() == oi[q].tolist(), (q, idx[q], oi[q])
        assert np.array_equal(d[q], od[q], equal_nan=nan_ok), (q, d[q], od[q])


def _observed(ix, search, walk):
    """one search under `walk`: (its arrays, everything else the walk can change)"""
    ix.set_param("flat_tail_lb_walk", walk)
    ix.set_param("flat_i8_stats", 1)  # (resets the histogram and the hit counters)
    names = ("flat_i8_queries", "flat_i8_redo", "flat_i8_second_queries", "flat_i8_second_redo")
    s0 = {s: ix.get_stat(s) for s in names}
    out = search()
    seen = {s: ix.get_stat(s) - s0[s] for s in names}
    seen.update({f"rounds_{r}": ix.get_stat(f"flat_i8_rounds_{r}") for r in range(9)})
    seen["hits_sum"] = ix.get_stat("flat_i8_hits_sum")
    seen["hits_max"] = ix.get_stat("flat_i8_hits_max")
    return out, seen


def _both_walks(ix, search, what):
    """walk 1, then walk 0: equal array for array and counter for counter; returns walk 0's arrays and counters"""
    try:
        out1, seen1 = _observed(ix, search, 1)
        out0, seen0 = _observed(ix, search, 0)
    finally:
        ix.set_param("flat_tail_lb_walk", 0)  # (process-wide)
        ix.set_param("flat_i8_stats", 0)
    assert seen0 == seen1, (what, seen0, seen1)
    for a0, a1 in zip(out0, out1):
        assert a0.dtype == a1.dtype and a0.shape == a1.shape, what
        assert np.array_equal(a0.view(np.uint32) if a0.dtype == np.float32 else a0, a1.view(np.uint32) if a1.dtype == np.float32 else a1), what
    return out0, seen0


@pytest.fixture(scope="module")
def separable(mods):
    _, O = mods
    base, qs = gist_like(30000, seed=3101), gist_like(130, seed=3102)
    ref = {(kind, k): O.flat_knn_batch(base, qs, k, kind, nthreads=8) for kind in (O.L2SQR, O.COSINE) for k in (1, 10, 64)}
    return base, qs, ref


@pytest.mark.parametrize("dist", ["l2sqr", "cosine"])
def test_separable_rows_every_form(mods, separable, dist):
    """30 000 gist-like rows x 130 queries at dim 960, every form of the kernel, k = 1, 10, 64"""
    vdb, O = mods
    base, qs, ref = separable
    kind = O.L2SQR if dist == "l2sqr" else O.COSINE
    ix = vdb.GpuIndex(960, dist)
    ix.batch_add(base)
    ix.set_flat_mode(2)
    try:
        for nw in NWS:
            ix.set_param("flat_tail_lb_nw", nw)
            for k in (1, 10, 64):
                (idx, d, cnt), seen = _both_walks(ix, lambda: ix.flat_knn(qs, k), (dist, nw, k))
                assert seen["flat_i8_queries"] == len(qs)
                _check_all(idx, d, cnt, *ref[(kind, k)])
    finally:
        ix.set_param("flat_tail_lb_nw", 0)
        ix.close()


@pytest.fixture(scope="module")
def clusters(mods):
    """the near-duplicate clusters of test_i8_pass_redo_tiers (tests/test_flat_i8_gpu.py)"""
    _, O = mods
    rng = np.random.default_rng(77)
    dim, n, nq = 192, 30000, 140
    centers = rng.standard_normal((30, dim)).astype(np.float32)
    base = (centers[rng.integers(30, size=n)] + 1e-4 * rng.standard_normal((n, dim))).astype(np.float32)
    base[100:140] = base[99]  # 41 identical rows
    qs = (centers[rng.integers(30, size=nq)] + 1e-4 * rng.standard_normal((nq, dim))).astype(np.float32)
    qs[0] = base[99]
    return base, qs, O.flat_knn_batch(base, qs, 10, 0, nthreads=8)


@pytest.mark.parametrize("second", [0, 1])
def test_walks_cross_window_edges(mods, clusters, second):
    """clusters of ~1000 members the walk cannot close: it runs for as many rounds as flat_i8_rows allows -- 1, 3, 4 (exactly one window), 5
    (one round into the next window), 8 and 32 (many windows) -- and with the second attempt on (flat_i8_second 0) walks up to 128 rounds
    over an 8192-slot list"""
    vdb, _ = mods
    base, qs, (oi, od, oc) = clusters
    ix = vdb.GpuIndex(192, "l2sqr")
    ix.batch_add(base)
    ix.set_flat_mode(2)
    ix.set_param("flat_i8", 2)
    ix.set_param("flat_i8_refine", 1)
    ix.set_param("flat_i8_second", second)
    try:
        for rows in (64, 192, 256, 320, 512, 2048):
            ix.set_param("flat_i8_rows", rows)
            (idx, d, cnt), seen = _both_walks(ix, lambda: ix.flat_knn(qs, 10), (second, rows))
            print(f"second {second} rows {rows}: {seen}")
            assert seen["flat_i8_queries"] == len(qs)
            if second == 1:
                assert seen["flat_i8_second_queries"] == 0
            _check_all(idx, d, cnt, oi, od, oc)
    finally:
        ix.close()


@pytest.mark.parametrize("n", [66, 131, 301])
def test_short_lists(mods, n):
    """The smallest tables the 8-bit pass takes (more than 64 rows; flat_small 1 keeps calls of these sizes off the one-launch kernel): hit
    lists shorter than one round, shorter than a window, or ending inside a window.  With flat_i8_rows 64 as with the default 256."""
    vdb, O = mods
    dim, nq = 128, 40
    rng = np.random.default_rng(n)
    base = rng.standard_normal((n, dim)).astype(np.float32)
    qs = rng.standard_normal((nq, dim)).astype(np.float32)
    ix = vdb.GpuIndex(dim, "l2sqr")
    ix.batch_add(base)
    ix.set_flat_mode(2)
    ix.set_param("flat_small", 1)
    ix.set_param("flat_i8", 2)
    try:
        for rows in (64, 256):
            ix.set_param("flat_i8_rows", rows)
            for k in (1, 10):
                (idx, d, cnt), seen = _both_walks(ix, lambda: ix.flat_knn(qs, k), (n, rows, k))
                print(f"n {n} rows {rows} k {k}: {seen}")
                assert seen["flat_i8_queries"] == nq  # the pass took the table
                _check_all(idx, d, cnt, *O.flat_knn_batch(base, qs, k, 0, nthreads=8))
    finally:
        ix.close()


@pytest.mark.parametrize("dist", ["l2sqr", "cosine"])
def test_equal_keys_and_equal_distances(mods, dist):
    """70 copies of one row and 300 of another, queries equal to those rows (and near them): equal keys at the skip boundary and equal
    distances at D_k must come out in the reference's order (ascending row index)"""
    vdb, O = mods
    dim, n = 128, 20000
    rng = np.random.default_rng(31)
    base = rng.standard_normal((n, dim)).astype(np.float32)
    base[rng.choice(np.arange(1000, 9000), 69, replace=False)] = base[500]   # 70 rows equal to row 500, scattered
    base[rng.choice(np.arange(9000, n), 299, replace=False)] = base[600]     # 300 rows equal to row 600
    qs = rng.standard_normal((40, dim)).astype(np.float32)
    qs[0], qs[1] = base[500], base[600]
    qs[2] = base[500] + np.float32(1e-3) * rng.standard_normal(dim).astype(np.float32)
    qs[3] = base[600] + np.float32(1e-3) * rng.standard_normal(dim).astype(np.float32)
    kind = O.L2SQR if dist == "l2sqr" else O.COSINE
    ix = vdb.GpuIndex(dim, dist)
    ix.batch_add(base)
    ix.set_flat_mode(2)
    ix.set_param("flat_i8", 2)
    try:
        for rows in (256, 1024):
            ix.set_param("flat_i8_rows", rows)
            for k in (10, 64):
                (idx, d, cnt), seen = _both_walks(ix, lambda: ix.flat_knn(qs, k), (dist, rows, k))
                print(f"{dist} rows {rows} k {k}: {seen}")
                _check_all(idx, d, cnt, *O.flat_knn_batch(base, qs, k, kind, nthreads=8))
    finally:
        ix.close()


def test_nothing_to_skip_by_construction(mods):
    """a Cosine table with an all-zero row (the bound's `plain` is false for the whole index: nothing certifies, nothing is skipped) and
    queries with a NaN coordinate (L2Sqr and Cosine): the same answers as walk 1, and the oracle's"""
    vdb, O = mods
    dim, n = 128, 20000
    rng = np.random.default_rng(32)
    base = rng.standard_normal((n, dim)).astype(np.float32)
    qs = rng.standard_normal((40, dim)).astype(np.float32)
    qs[1, 3] = np.nan
    for dist, kind, zero_row in (("cosine", O.COSINE, True), ("cosine", O.COSINE, False), ("l2sqr", O.L2SQR, False)):
        b = base.copy()
        if zero_row:
            b[7] = 0
        ix = vdb.GpuIndex(dim, dist)
        ix.batch_add(b)
        ix.set_flat_mode(2)
        ix.set_param("flat_i8", 2)
        try:
            (idx, d, cnt), seen = _both_walks(ix, lambda: ix.flat_knn(qs, 10), (dist, zero_row))
            print(f"{dist} zero row {zero_row}: {seen}")
            _check_all(idx, d, cnt, *O.flat_knn_batch(b, qs, 10, kind, nthreads=8), nan_ok=True)
        finally:
            ix.close()


def test_masked_search(mods):
    """flat_knn_filtered under an allow-list of half the rows, on the smallest table tests/test_flat_filtered_gpu.py runs the 8-bit tier on
    (17 000 x 128, flat_filtered_direct_max 0): walk 0 = walk 1 = the oracle's order restricted to the allowed rows"""
    vdb, O = mods
    n, dim, nq, k = 17000, 128, 130, 10
    base, qs = gist_like(n, dim=dim, seed=3401), gist_like(nq, dim=dim, seed=3402)
    allow = np.random.default_rng(33).random(n) < 0.5
    oi, od, oc = O.flat_knn_batch(base, qs, n, 0, nthreads=16)
    ix = vdb.GpuIndex(dim, "l2sqr")
    ix.batch_add(base)
    ix.set_flat_mode(2)
    ix.set_param("flat_filtered_direct_max", 0)
    mk = ix.make_mask(allow)
    try:
        f0 = ix.get_stat("flat_filtered_i8_queries")
        (idx, d, cnt), seen = _both_walks(ix, lambda: ix.flat_knn_filtered(qs, k, mk), "masked")
        assert ix.get_stat("flat_filtered_i8_queries") - f0 == 2 * nq
        for q in range(nq):
            keep = allow[oi[q].astype(np.int64)]
            assert cnt[q] == k and idx[q].tolist() == oi[q][keep][:k].tolist() and np.array_equal(d[q], od[q][keep][:k]), q
    finally:
        mk.close()
        ix.close()
