"""GPU: the k-means centroid update (one iteration from given centroids, GpuIndex.kmeans(max_iter=1)) against numpy: member counts equal,
centroids within one f32 ulp of f32(float64 mean) -- the kernel sums in f64 over 16 segments, numpy pairwise, so the two f64 sums may
round to neighbouring f32 values and equality is not asserted.  "six": clusters of 0 (keeps its centroid bit for bit), 1, 63, 64, 65 and
5000 members (every segment of the update holds several rows).  "three_hundred": 300 clusters of 0 .. 31 members, so the member sort runs
both of its 8-bit digit passes and ids above 255 must land in order.  dim 70 crosses the 64-column slab of an update workgroup."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

LAYOUTS = {"six": (0, 1, 63, 64, 65, 5000), "three_hundred": tuple((7 * j) % 32 for j in range(300))}


@pytest.mark.parametrize("dist", ("l2sqr", "cosine"))
@pytest.mark.parametrize("layout", sorted(LAYOUTS))
def test_one_update_against_numpy(dist, layout):
    import lab_1806_vec_db_amd as vdb

    sizes_want = LAYOUTS[layout]
    dim, c = 70, len(sizes_want)
    rng = np.random.default_rng(5)
    cent = (rng.standard_normal((c, dim)) * 10).astype(np.float32)  # pairwise far apart in distance and in angle; no row is near an empty one
    owner = rng.permutation(np.repeat(np.arange(c), sizes_want))
    rows = (cent[owner] + rng.uniform(-0.5, 0.5, (len(owner), dim))).astype(np.float32)
    ix = vdb.GpuIndex(dim, dist, device=0)
    ix.batch_add(rows)
    runs = [ix.kmeans(c, max_iter=1, init=cent) for _ in range(2)]
    got, assign, sizes, iters, _ = runs[0]
    assert iters == 1 and sizes.tolist() == list(sizes_want) and np.array_equal(assign, owner.astype(np.uint32))
    for j in range(c):
        if sizes_want[j] == 0:
            assert np.array_equal(got[j].view(np.uint32), cent[j].view(np.uint32)), j
            continue
        want = rows[owner == j].astype(np.float64).mean(axis=0).astype(np.float32)
        assert (np.abs(got[j].astype(np.float64) - want.astype(np.float64)) <= np.spacing(np.abs(want))).all(), j
    for a, b in zip(runs[0][:3], runs[1][:3]):
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8))
    assert ix.get_stat("kmeans_calls") == 2 and ix.get_stat("kmeans_iterations") == 2
    ix.close()
