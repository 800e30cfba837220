"""GPU: GpuIndex.covariance (k_pca_colsum / k_pca_syrk / k_pca_cov_reduce: f64 sums on the matrix pipe) against numpy float64.

The bounds are the standard ones for a sum of m terms, u = 2^-53: either side may lose up to about m u of the sum of the absolute terms,
so |mean - mu| <= 2 (m + 8) u mean(|X|) and |cov - want| <= 2 (m + 8) u A with A the covariance of the absolute centred values.  They are
derived, not tuned.  dim 1 / 15 / 16 / 17 / 70 / 130: inside an MFMA tile, at and across its edge, across the 64-column block (one
off-diagonal block), three block columns (a block pair that is not adjacent).  m 2 .. 5: around the 4-row instruction step; 65: past the
16-row slice; 1000: 16 row segments of 64 rows, the last ragged.  The rows have a non-zero column mean, so a missing centring shows."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
STATS = ("pca_cov_calls", "pca_cov_rows", "pca_project_calls", "pca_project_rows")


def _rows(m, dim, seed=0):
    return (np.random.default_rng(seed).standard_normal((m, dim)) * 3 + 5).astype(np.float32)


def _check(got, x, center):
    mean, cov, m = got
    X = x.astype(np.float64)
    assert m == len(X) and mean.dtype == cov.dtype == np.float64 and cov.shape == (X.shape[1],) * 2
    mu = X.mean(0) if center else np.zeros(X.shape[1])
    D = X - mu
    want, A = D.T @ D / (m - center), np.abs(D).T @ np.abs(D) / (m - center)
    err_mean, err_cov = np.abs(mean - mu), np.abs(cov - want)
    print("mean err / bound", (err_mean / (2 * (m + 8) * U * np.abs(X).mean(0))).max(), "cov err / bound", (err_cov / (2 * (m + 8) * U * A)).max())
    assert (err_mean <= 2 * (m + 8) * U * np.abs(X).mean(0)).all() if center else not mean.any()
    assert (err_cov <= 2 * (m + 8) * U * A).all()


@pytest.mark.parametrize("m", (2, 3, 4, 5, 65, 1000))
@pytest.mark.parametrize("dim", (1, 15, 16, 17, 70, 130))
def test_covariance_against_numpy(dim, m):
    import lab_1806_vec_db_amd as vdb

    if m == 1000:
        assert vdb.GpuIndex.pca_plan(m, dim)[2] > 1  # more than one row segment
    x = _rows(m, dim)
    ix = vdb.GpuIndex(dim, "l2sqr", device=0)
    ix.batch_add(x)
    _check(ix.covariance(), x, 1)
    _check(ix.covariance(center=False), x, 0)
    assert [ix.get_stat(s) for s in STATS] == [2, 2 * m, 0, 0]
    ix.close()


def test_symmetry_repeat_mask_and_device_form():
    import torch

    import lab_1806_vec_db_amd as vdb

    x = _rows(1000, 130, seed=1)
    ix = vdb.GpuIndex(130, "cosine", device=0)
    ix.batch_add(x)
    a, b = ix.covariance(), ix.covariance()
    assert np.array_equal(a[1].view(np.uint64), a[1].T.view(np.uint64))  # symmetric bit for bit
    assert all(np.array_equal(p.view(np.uint64), q.view(np.uint64)) for p, q in zip(a[:2], b[:2]))  # the same bits from two calls
    allowed = np.arange(1000) % 3 == 0
    mask = ix.make_mask(allowed)
    got = ix.covariance(mask=mask)
    _check(got, x[allowed], 1)
    t_mean, t_cov = torch.full((131,), -7.0, dtype=torch.float64, device="cuda"), torch.full((130 * 130 + 1,), -7.0, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    assert ix.covariance_device(t_mean.data_ptr(), t_cov.data_ptr(), mask=mask) == 334
    assert np.array_equal(t_mean.cpu().numpy()[:130], got[0]) and np.array_equal(t_cov.cpu().numpy()[:-1].reshape(130, 130), got[1])
    assert t_mean[130].item() == -7.0 and t_cov[-1].item() == -7.0
    for h in (mask, ix):
        h.close()


def test_refusals_leave_outputs_and_counters_alone():
    import torch

    import lab_1806_vec_db_amd as vdb

    x = _rows(20, 8)
    ix, other, u8 = vdb.GpuIndex(8, "l2sqr", device=0), vdb.GpuIndex(8, "l2sqr", device=0), vdb.GpuIndex(64, "l2sqr", device=0, scalar="u8")
    ix.batch_add(x), other.batch_add(x), u8.batch_add_u8(np.ones((9, 64), dtype=np.uint8))
    wide = vdb.GpuIndex(2049, "l2sqr", device=0)
    wide.batch_add(np.ones((2, 2049), dtype=np.float32))
    one, none, foreign, stale = ix.make_mask(np.arange(20) == 3), ix.make_mask(np.zeros(20, dtype=bool)), other.make_mask(np.ones(20, dtype=bool)), other.make_mask(np.ones(20, dtype=bool))
    t_mean, t_cov, t_out = (torch.full((n,), -7.0, dtype=d, device="cuda") for n, d in ((2049, torch.float64), (2049 * 2049, torch.float64), (64, torch.float32)))
    t_w = torch.ones((9, 9), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    before = [[h.get_stat(s) for s in STATS] for h in (ix, other, u8, wide)]
    cov = lambda h, **kw: h.covariance_device(t_mean.data_ptr(), t_cov.data_ptr(), **kw)
    proj = lambda h, n_comp, **kw: h.project_device(t_w.data_ptr(), n_comp, t_out.data_ptr(), **kw)
    for call, word in ((lambda: cov(u8), "f32 rows"), (lambda: cov(ix, mask=one), "at least 2 rows"), (lambda: cov(ix, center=False, mask=none), "at least 1 rows"),
                       (lambda: cov(wide), "1 .. 2048"), (lambda: cov(ix, mask=foreign), "another index"), (lambda: proj(u8, 2), "f32 rows"),
                       (lambda: proj(ix, 0), "n_comp = 0"), (lambda: proj(ix, 9), "9 components of 8"), (lambda: proj(ix, 2, mask=foreign), "another index"),
                       (lambda: ix.project(np.ones((2, 9), dtype=np.float32)), "dimension mismatch"),
                       (lambda: ix.project_vectors(x, np.ones((1025, 8), dtype=np.float32)), "more than 1024")):
        with pytest.raises(vdb.VdbError, match=word):
            call()
    other.batch_add(x[:1])
    for call in (lambda: cov(other, mask=stale), lambda: proj(other, 2, mask=stale)):
        with pytest.raises(vdb.VdbError, match="stale"):
            call()
    assert all((t == -7.0).all().item() for t in (t_mean, t_cov, t_out))
    assert [[h.get_stat(s) for s in STATS] for h in (ix, other, u8, wide)] == before
    for h in (one, none, foreign, stale, ix, other, u8, wide):
        h.close()
