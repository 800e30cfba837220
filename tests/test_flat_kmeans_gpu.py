"""GPU: k-means end to end (GpuIndex.kmeans; vdb_flat_kmeans) on planted blobs, 2000 x 64 in 8 blobs, against a float64 restatement of
the rule.  The restatement checks at every step that each row's two nearest centroids are apart by a margin no f32 evaluation can close,
so every Lloyd step is unambiguous and partition and iteration count must match exactly."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NONE = 0xFFFFFFFF
STATS = ("kmeans_calls", "kmeans_iterations", "kmeans_rows_assigned", "kmeans_unsure_rows", "fetch_calls")


def _blobs():
    rng = np.random.default_rng(21)
    centers = rng.uniform(-4, 4, (8, 64))
    owner = rng.integers(0, 8, 2000)
    return (centers[owner] + rng.standard_normal((2000, 64)) * 0.2).astype(np.float32), owner


def _lloyd64(x, cent, max_iter, tol):
    """(centroids, assign, iters) by the rule of include/vdbhip.h in float64, L2Sqr"""
    x, cent = x.astype(np.float64), cent.astype(np.float64).copy()
    prev, before, t = None, None, 0
    while True:
        d = ((x[:, None, :] - cent[None]) ** 2).sum(-1)
        ds = np.sort(d, axis=1)
        assert ((ds[:, 1] - ds[:, 0]) > 1e-3 * ds[:, 1]).all()  # unambiguous in f32: the fold's error is below 1e-5 of the distance
        assign = d.argmin(axis=1)
        now = ds[:, 0].sum()
        if t == max_iter or (t > 0 and ((assign == prev).all() or abs(now - before) <= tol * before)):
            return cent, assign, t
        for j in range(len(cent)):
            if (assign == j).any():
                cent[j] = x[assign == j].mean(axis=0).astype(np.float32)
        prev, before, t = assign, now, t + 1


def _same_partition(a, b):
    return len(set(zip(a.tolist(), b.tolist()))) == len(set(a.tolist())) == len(set(b.tolist()))


def test_planted_blobs_from_given_and_seeded_centroids():
    import lab_1806_vec_db_amd as vdb

    x, owner = _blobs()
    init = x[[int(np.flatnonzero(owner == j)[0]) for j in range(8)]]  # one start in every blob
    ix = vdb.GpuIndex(64, "l2sqr", device=0)
    ix.batch_add(x)
    want_c, want_a, want_t = _lloyd64(x, init, 20, 1e-4)
    cent, assign, sizes, iters, inertia = ix.kmeans(8, init=init)
    assert want_t >= 1 and iters == want_t and np.array_equal(assign, want_a.astype(np.uint32))
    assert np.array_equal(sizes, np.bincount(want_a, minlength=8).astype(np.uint64)) and np.allclose(cent, want_c, rtol=0, atol=1e-5)
    assert np.isclose(inertia, ((x.astype(np.float64) - want_c[want_a]) ** 2).sum(), rtol=1e-4)
    again = ix.kmeans(8, init=init)
    assert all(np.array_equal(np.asarray(a), np.asarray(b)) for a, b in zip((cent, assign, sizes, iters, inertia), again))
    # max_iter = 0: the assignment to the initial centroids, no update
    c0, a0, _, t0, _ = ix.kmeans(8, max_iter=0, init=init)
    assert t0 == 0 and np.array_equal(c0.view(np.uint32), init.view(np.uint32)) and np.array_equal(a0, _lloyd64(x, init, 0, 1e-4)[1].astype(np.uint32))
    # seeded: the same twice, another seed is accepted, and the planted partition once every blob holds a start (k-means++ on blobs
    # this far apart puts one start into each: asserted through the result, not assumed)
    s1, s2 = ix.kmeans(8, seed=3), ix.kmeans(8, seed=3)
    assert all(np.array_equal(np.asarray(a), np.asarray(b)) for a, b in zip(s1, s2))
    assert _same_partition(s1[1], owner) and s1[2].sum() == 2000
    # under a mask: the rows outside keep LABEL_NONE, the rows inside fall into their blobs
    allow = np.arange(2000) % 4 != 0
    mk = ix.make_mask(allow)
    mc, ma, ms, _, _ = ix.kmeans(8, seed=3, mask=mk)
    assert (ma[~allow] == NONE).all() and _same_partition(ma[allow], owner[allow]) and ms.sum() == allow.sum()
    mk.close()
    ix.close()


def test_refusals_leave_outputs_and_counters_untouched():
    import lab_1806_vec_db_amd as vdb

    x, _ = _blobs()
    ix, other = vdb.GpuIndex(64, "l2sqr", device=0), vdb.GpuIndex(64, "l2sqr", device=0)
    ix.batch_add(x[:100])
    other.batch_add(x[:100])
    foreign, stale = other.make_mask(np.ones(100, bool)), ix.make_mask(np.ones(100, bool))
    few = ix.make_mask(np.arange(100) < 3)
    ix.batch_add(x[100:110])
    few2 = ix.make_mask(np.arange(110) < 3)
    u8 = vdb.GpuIndex(64, "l2sqr", device=0, scalar="u8")
    u8.batch_add_u8(np.zeros((10, 64), np.uint8))
    before = [ix.get_stat(s) for s in STATS]
    for call in (lambda: ix.kmeans(0), lambda: ix.kmeans(111), lambda: ix.kmeans(65536), lambda: ix.kmeans(4, mask=few2),
                 lambda: ix.kmeans(2, mask=stale), lambda: ix.kmeans(2, mask=foreign), lambda: ix.kmeans(2, init=np.zeros((2, 63), np.float32)),
                 lambda: ix.kmeans_assign(np.zeros((2, 63), np.float32)), lambda: u8.kmeans(2)):
        with pytest.raises(vdb.VdbError):
            call()
    assert [ix.get_stat(s) for s in STATS] == before
    for m in (foreign, stale, few, few2):
        m.close()
    for i in (ix, other, u8):
        i.close()
