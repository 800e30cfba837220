"""GPU: the k-means assignment step (GpuIndex.kmeans_assign; vdb_kmeans_assign / _device) against the argmin over the oracle's pair
distances under (distance, centroid id): assignments equal, best distances bit-equal.

Every table carries the inputs a wrong fused argmin gets wrong: a duplicated centroid (first and last id: the tie goes to the lowest), a
row equal to it, a row at the exact midpoint of centroids 1 and 2 (their distances are the same f32 bits), near-twin centroids in one MFMA
block (4, 5) and in two centroid tiles (3, 64), rows next to them, a zero row and a NaN row.  Sizes: dims below, off and on the MFMA
k-block of 32; centroid counts around the tile of 64; row counts around the tile of 128."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

DIMS = (4, 20, 100, 960)
CS = (1, 2, 63, 64, 65, 300)
MS = (1, 127, 128, 129, 1000)
NONE = 0xFFFFFFFF


def _case(dim, c, m, seed):
    rng = np.random.default_rng(seed)
    cent = rng.random((c, dim), dtype=np.float32)
    rows = cent[rng.integers(0, c, m)] + rng.standard_normal((m, dim)).astype(np.float32) * np.float32(0.05)
    if c > 2:
        cent[2] = cent[1]
        cent[1, 0], cent[2, 0] = 0.25, 0.75
    if c > 5:
        cent[5] = cent[4] + np.float32(1e-4)
    if c > 64:
        cent[64] = cent[3] + np.float32(1e-4)
    if c > 1:
        cent[c - 1] = cent[0]
    special = [cent[0], cent[min(1, c - 1)].copy(), cent[min(3, c - 1)] + np.float32(5e-5), cent[min(4, c - 1)] + np.float32(5e-5), np.zeros(dim), np.full(dim, np.nan)]
    special[1][0] = 0.5
    for i, v in enumerate(special[:m]):
        rows[i] = v
    return cent, rows.astype(np.float32)


def _oracle(cent, rows, kind):
    from oracle import oracle as O

    oi, od, _ = O.flat_knn_batch(cent, rows, 1, kind, nthreads=16)
    return oi[:, 0].astype(np.uint32), od[:, 0]


def _same_bits(got, want):
    both_nan = np.isnan(got) & np.isnan(want)
    return np.array_equal(got.view(np.uint32)[~both_nan], want.view(np.uint32)[~both_nan])


@pytest.mark.parametrize("dist,kind", (("l2sqr", 0), ("cosine", 1)))
@pytest.mark.parametrize("dim", DIMS)
@pytest.mark.parametrize("m", MS)
@pytest.mark.parametrize("c", CS)
def test_assignment_is_the_oracles_argmin(dist, kind, dim, m, c):
    import lab_1806_vec_db_amd as vdb

    cent, rows = _case(dim, c, m, 1000 * dim + m)
    ix = vdb.GpuIndex(dim, dist, device=0)
    ix.batch_add(rows)
    assign, best, unsure = ix.kmeans_assign(cent)
    want_a, want_d = _oracle(cent, rows, kind)
    assert np.array_equal(assign, want_a), np.flatnonzero(assign != want_a)[:8]
    assert _same_bits(best, want_d)
    if c > 1:
        assert unsure > 0  # row 0 equals two centroids (and row 1 is a midpoint): ties the matrix pass must not settle
    if m > 5:
        assert np.isnan(best[5])
    assert ix.get_stat("kmeans_rows_assigned") == m and ix.get_stat("kmeans_unsure_rows") == unsure
    ix.close()


@pytest.mark.parametrize("dist,kind", (("l2sqr", 0), ("cosine", 1)))
def test_device_forms_match_the_host_forms(dist, kind):
    """vdb_kmeans_assign_device (with and without the best distances) and vdb_flat_kmeans_device over torch tensors: the host forms' bits"""
    import torch

    import lab_1806_vec_db_amd as vdb

    cent, rows = _case(20, 65, 300, 9)
    ix = vdb.GpuIndex(20, dist, device=0)
    ix.batch_add(rows)
    want_a, want_d, _ = ix.kmeans_assign(cent)
    d_cent = torch.from_numpy(cent).cuda()
    d_assign = torch.zeros(300, dtype=torch.int32, device="cuda")
    d_best = torch.full((300,), 7.0, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    ix.kmeans_assign_device(d_cent.data_ptr(), 65, d_assign.data_ptr())
    assert np.array_equal(d_assign.cpu().numpy().view(np.uint32), want_a) and (d_best == 7.0).all()
    d_assign.zero_()
    torch.cuda.synchronize()
    ix.kmeans_assign_device(d_cent.data_ptr(), 65, d_assign.data_ptr(), d_best.data_ptr())
    assert np.array_equal(d_assign.cpu().numpy().view(np.uint32), want_a) and _same_bits(d_best.cpu().numpy(), want_d)
    with pytest.raises(vdb.VdbError):
        ix.kmeans_assign_device(d_cent.data_ptr() + 2, 65, d_assign.data_ptr())
    good = rows[6:300:50]  # finite rows as starts
    h = ix.kmeans(len(good), max_iter=3, init=good)
    o_cent = torch.zeros(len(good), 20, dtype=torch.float32, device="cuda")
    o_sizes = torch.zeros(len(good), dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    it, inertia = ix.kmeans_device(len(good), o_cent.data_ptr(), d_assign.data_ptr(), o_sizes.data_ptr(), max_iter=3, init=good)
    got = (o_cent.cpu().numpy(), d_assign.cpu().numpy().view(np.uint32), o_sizes.cpu().numpy().view(np.uint64))
    assert all(a.tobytes() == b.tobytes() for a, b in zip(got, h[:3])) and it == h[3]  # (the NaN row makes a centroid NaN: bytes, not ==)
    assert inertia == h[4] or (np.isnan(inertia) and np.isnan(h[4]))
    with pytest.raises(vdb.VdbError):
        ix.kmeans_device(len(good), o_cent.data_ptr() + 4, d_assign.data_ptr(), o_sizes.data_ptr(), init=good)
    ix.close()


@pytest.mark.parametrize("dist,kind", (("l2sqr", 0), ("cosine", 1)))
def test_mask_with_id_offset(dist, kind):
    import lab_1806_vec_db_amd as vdb

    cent, rows = _case(20, 65, 300, 7)
    ix = vdb.GpuIndex(20, dist, device=0)
    ix.batch_add(rows)
    ix.set_id_offset(1000)
    allow = np.arange(300) % 3 != 1
    mk = ix.make_mask(allow)
    assign, best, _ = ix.kmeans_assign(cent, mk)
    want_a, want_d = _oracle(cent, rows, kind)
    assert np.array_equal(assign[allow], want_a[allow]) and _same_bits(best[allow], want_d[allow])
    assert (assign[~allow] == NONE).all() and np.isnan(best[~allow]).all()
    assert ix.get_stat("kmeans_rows_assigned") == allow.sum()
    mk.close()
    ix.close()


@pytest.mark.parametrize("dist,kind", (("l2sqr", 0), ("cosine", 1)))
def test_well_separated_rows_never_take_the_exact_fold(dist, kind):
    """centroids 3 e_j, rows within 0.01 of theirs: the float64 margin between best and second-best distance is verified to exceed four
    times the E the plan reports for these norms (the matrix pass sees the margin through scores that are each off by less than E / 2)"""
    import lab_1806_vec_db_amd as vdb

    dim, c, m = 100, 8, 1000
    rng = np.random.default_rng(11)
    cent = np.zeros((c, dim), dtype=np.float32)
    cent[np.arange(c), np.arange(c)] = 3.0
    owner = rng.integers(0, c, m)
    rows = (cent[owner] + rng.uniform(-0.01, 0.01, (m, dim))).astype(np.float32)
    x, y = rows.astype(np.float64), cent.astype(np.float64)
    if kind == 0:
        d = ((x[:, None, :] - y[None]) ** 2).sum(-1)
    else:
        d = 1.0 - x @ y.T / (np.linalg.norm(x, axis=1)[:, None] * np.linalg.norm(y, axis=1)[None])
    ds = np.sort(d, axis=1)
    err = vdb.GpuIndex.kmeans_plan(m, dim, c, lloyd=False, cosine=bool(kind), xn=float(np.linalg.norm(x, axis=1).max()), cn=3.0,
                                   d_best=float(ds[:, 0].max()))[5]
    assert err > 0 and (ds[:, 1] - ds[:, 0]).min() > 4 * err
    ix = vdb.GpuIndex(dim, dist, device=0)
    ix.batch_add(rows)
    assign, _, unsure = ix.kmeans_assign(cent)
    assert np.array_equal(assign, owner.astype(np.uint32)) and unsure == 0 and ix.get_stat("kmeans_unsure_rows") == 0
    ix.close()
