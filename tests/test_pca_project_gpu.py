"""GPU: GpuIndex.project / project_vectors (k_pca_project: f64 MFMA accumulation over the dimension, one rounding to f32) against numpy
float64.  |got - want64| <= spacing(f32(|want64|)) + 2 (dim + 8) u B, u = 2^-53, B = |X - mean| |W|^T: one f32 rounding plus the f64
summation bound that can move a value across a rounding boundary.  dim 1 / 17 / 70 / 130: below one k-step of 4, a ragged 16-dimension
slice, several slices; n_comp 1 / 16 / 17 / 65: inside, at and across a 16-component tile, a second component block; rows 1 / 63 / 64 / 65 /
200: around the 64-row workgroup, several of them."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

U = 2.0 ** -53


def _data(rows, dim, n_comp, seed=0):
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((rows, dim)) * 3 + 5).astype(np.float32)
    return x, rng.standard_normal((n_comp, dim)).astype(np.float32), rng.standard_normal(dim) + 5


def _check(got, x, W, mean):
    D = x.astype(np.float64) - (0 if mean is None else mean)
    want, B = D @ W.astype(np.float64).T, np.abs(D) @ np.abs(W).astype(np.float64).T
    assert got.dtype == np.float32 and got.shape == want.shape
    bound = np.spacing(np.abs(want).astype(np.float32)).astype(np.float64) + 2 * (x.shape[1] + 8) * U * B
    print("err / bound", (np.abs(got - want) / bound).max())
    assert (np.abs(got - want) <= bound).all()


@pytest.mark.parametrize("dim,n_comp,rows", [(d, c, r) for d in (1, 17, 70, 130) for c in (1, 16, 17, 65) if c <= d for r in (1, 63, 64, 65, 200)])
def test_project_against_numpy(dim, n_comp, rows):
    import lab_1806_vec_db_amd as vdb

    x, W, mean = _data(rows, dim, n_comp)
    ix = vdb.GpuIndex(dim, "l2sqr", device=0)
    ix.batch_add(x)
    got = ix.project(W, mean)
    _check(got, x, W, mean)
    assert np.array_equal(ix.project_vectors(x, W, mean).view(np.uint32), got.view(np.uint32))  # the same kernel, the same bits
    assert [ix.get_stat(s) for s in ("pca_project_calls", "pca_project_rows", "pca_cov_calls")] == [1, rows, 0]
    ix.close()


def test_no_mean_mask_and_device_output():
    import torch

    import lab_1806_vec_db_amd as vdb

    x, W, mean = _data(200, 70, 17, seed=1)
    ix = vdb.GpuIndex(70, "cosine", device=0)
    ix.batch_add(x)
    _check(ix.project(W), x, W, None)
    allowed = np.arange(200) % 3 == 1
    mask = ix.make_mask(allowed)
    got = ix.project(W, mean, mask)  # compact, in ascending allowed-row order
    _check(got, x[allowed], W, mean)
    assert np.array_equal(got, ix.project(W, mean)[allowed])
    m = int(allowed.sum())
    t_w, t_mean = torch.from_numpy(W).cuda(), torch.from_numpy(mean).cuda()
    t_out = torch.full((1 + m * 17 + 1,), -7.0, dtype=torch.float32, device="cuda")  # the output starts 4 bytes into the allocation
    torch.cuda.synchronize()
    ix.project_device(t_w.data_ptr(), 17, t_out.data_ptr() + 4, t_mean.data_ptr(), mask)
    out = t_out.cpu().numpy()
    assert out[0] == -7.0 and out[-1] == -7.0 and np.array_equal(out[1:-1].reshape(m, 17), got)
    none = ix.make_mask(np.zeros(200, dtype=bool))
    assert ix.project(W, mean, none).shape == (0, 17)
    for h in (mask, none, ix):
        h.close()
