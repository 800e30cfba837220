"""GPU: GpuIndex.silhouette (k_sil_prepare / k_sil_pairs / k_sil_finish: every pair distance in f64 on the matrix pipe) against a plain
float64 numpy reference: the full distance matrix and the cluster sums.

The bound is derived in docs/DESIGN_flat.md 4.1aj, u = 2^-53, n = dim: a pair's D is off by at most E_ij = (n + 4) u (|x_i| + |x_j|)^2
(over |x_i||x_j| for Cosine, its root with the Euclidean flag); a and b inherit the largest e_i of their row plus a relative (m + 2) u
for their sums; then |s^ - s| <= 4 (e_i + (m + 2) u max(a, b)) / max(a, b) + 2^-23.  It needs max(a, b) >= 1000 e_i, a condition on the
INPUTS that every test asserts of the reference first.

Shapes (dim, scored rows, clusters): dim 1 / 4 / 5 inside an MFMA k-step and across it, 64 / 65 / 130 at and across the 16-dimension slice;
3 rows in one tile; 63 / 64 / 65 / 128 / 130 rows at and across the 64-row tile (two clusters of exactly 64: both end on a tile edge);
300 rows in 3 clusters of 100: a cluster spans two tiles, several row blocks; 70 clusters: more tiles than one walk step, singletons."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
NONE = 0xFFFFFFFF
STATS = ("silhouette_calls", "silhouette_rows")
SHAPES = ((1, 3, 2), (4, 63, 3), (5, 64, 2), (64, 128, 2), (64, 65, 3), (65, 130, 70), (130, 300, 3))
MODES = (("l2sqr", False), ("l2sqr", True), ("cosine", False))
# (every cosine distance in one dimension is 0 or 2: a = b = 0 on whole clusters, nothing for the bound to hold on)
CASES = [s + md for s in SHAPES for md in MODES if not (s[0] == 1 and md[0] == "cosine")]


def _blobs(dim, m, c, seed=0):
    """(rows, cluster of each row): Gaussian blobs about separated centres, the clusters dealt out in shuffled order, so that the
    (code, row) order is not the row order"""
    rng = np.random.default_rng(seed)
    cl = rng.permutation(np.arange(m) % c)
    x = (rng.standard_normal((c, dim)) * 4 + 1)[cl] + rng.standard_normal((m, dim)) * 0.25
    return x.astype(np.float32), cl


def _codes(cl, c):
    """sparse, large codes whose order is not the cluster order, the largest code there is among them"""
    table = (np.arange(c, dtype=np.uint64) * 61000007 + 5) % 0xFFFFFFF0
    table[c // 2] = 0xFFFFFFFE
    return table[cl].astype(np.uint32)


def _reference(x, codes, metric, euclid):
    """(s, tol, the size of each row's cluster) of the rows of x, all scored, in float64; asserts the condition on the inputs"""
    X, m, n = x.astype(np.float64), len(x), x.shape[1]
    nr, G = np.sqrt((X * X).sum(1)), X @ X.T
    E = (n + 4) * U * (nr[:, None] + nr[None, :]) ** 2
    if metric == "cosine":
        D, E = np.maximum(1 - G / np.outer(nr, nr), 0), E / np.outer(nr, nr)
    else:
        D = np.maximum(nr[:, None] ** 2 + nr[None, :] ** 2 - 2 * G, 0)
        D, E = (np.sqrt(D), np.sqrt(E)) if euclid else (D, E)
    np.fill_diagonal(D, 0)  # the pair (i, i) is left out by position
    values, own, size = np.unique(codes, return_inverse=True, return_counts=True)
    sums = np.stack([D[:, own == c].sum(1) for c in range(len(values))], 1)
    rows = np.arange(m)
    a = sums[rows, own] / np.maximum(size[own] - 1, 1)
    means = sums / size
    means[rows, own] = np.inf
    b = means.min(1)
    mx, e = np.maximum(a, b), E.max(1)
    live = (size[own] > 1) & (mx > 0)
    assert (mx[size[own] > 1] >= 1000 * e[size[own] > 1]).all(), "the inputs are too ill-conditioned for the bound"
    s = np.where(live, (b - a) / np.where(live, mx, 1), 0.0)
    return s, np.where(live, 4 * (e + (m + 2) * U * mx) / np.where(live, mx, 1) + 2.0 ** -23, 0.0), size[own]


def _check(got, x, codes, scored, metric, euclid):
    s, mean, m, clusters = got
    want, tol, size = _reference(x[scored], codes[scored], metric, euclid)
    assert m == scored.sum() and clusters == len(np.unique(codes[scored])) and s.dtype == np.float32 and len(s) == len(x)
    assert np.isnan(s[~scored]).all()
    err = np.abs(s[scored].astype(np.float64) - want)
    print("largest error / bound", (err[tol > 0] / tol[tol > 0]).max() if (tol > 0).any() else 0.0)
    assert (err <= tol).all() and (s[scored][size == 1] == 0).all()
    assert abs(mean - want.mean()) <= tol.mean()


@pytest.mark.parametrize("dim, m, c, metric, euclid", CASES)
def test_against_numpy(dim, m, c, metric, euclid):
    import lab_1806_vec_db_amd as vdb

    x, cl = _blobs(dim, m, c, seed=dim + m)
    codes = _codes(cl, c)
    ix = vdb.GpuIndex(dim, metric, device=0)
    ix.batch_add(x)
    ix.set_labels(2, codes)
    got = ix.silhouette(2, euclidean=euclid)
    _check(got, x, codes, np.ones(m, dtype=bool), metric, euclid)
    again = ix.silhouette(2, euclidean=euclid)
    assert np.array_equal(got[0].view(np.uint32), again[0].view(np.uint32)) and np.float64(got[1]).view(np.uint64) == np.float64(again[1]).view(np.uint64)
    assert [ix.get_stat(s) for s in STATS] == [2, 2 * m]
    ix.close()


@pytest.mark.parametrize("metric, euclid", MODES)
def test_unscored_rows_mask_identical_rows_and_device_form(metric, euclid):
    import torch

    import lab_1806_vec_db_amd as vdb

    x, cl = _blobs(65, 200, 4, seed=3)
    codes = _codes(cl, 4)
    a, b = np.flatnonzero(cl == 1)[-3:-1]
    x[b] = x[a]  # two identical rows inside a larger cluster
    codes[np.flatnonzero(cl == 3)[1:]] = NONE  # cluster 3 keeps one labelled row: a singleton
    codes[[5, 17, 150]] = NONE
    x[9, 40], x[30, 0], x[77] = np.nan, np.inf, 0.0
    allowed = np.arange(200) % 7 != 4
    scored = allowed & (codes != NONE) & np.isfinite(x).all(1) & ((metric != "cosine") | (x != 0).any(1))
    ix, only = vdb.GpuIndex(65, metric, device=0), vdb.GpuIndex(65, metric, device=0)
    ix.batch_add(x), only.batch_add(x[scored])
    ix.set_labels(0, codes), only.set_labels(0, codes[scored])
    mask = ix.make_mask(allowed)
    got = ix.silhouette(0, mask, euclid)
    _check(got, x, codes, scored, metric, euclid)
    assert scored[a] and scored[b]
    alone = only.silhouette(0, euclidean=euclid)  # the rows that are not scored change no bit of the others
    assert np.array_equal(got[0][scored].view(np.uint32), alone[0].view(np.uint32)) and got[1:] == alone[1:]
    t_s, t_mean = torch.full((201,), -7.0, dtype=torch.float32, device="cuda"), torch.full((2,), -7.0, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    assert ix.silhouette_device(0, t_s.data_ptr(), t_mean.data_ptr(), mask, euclid) == got[2:]
    assert np.array_equal(t_s.cpu().numpy()[:200].view(np.uint32), got[0].view(np.uint32)) and t_mean[0].item() == got[1]
    assert t_s[200].item() == -7.0 and t_mean[1].item() == -7.0
    for h in (mask, ix, only):
        h.close()


def test_refusals_leave_outputs_and_counters_alone():
    import torch

    import lab_1806_vec_db_amd as vdb

    x, cl = _blobs(8, 20, 3)
    ix, other, cos = vdb.GpuIndex(8, "l2sqr", device=0), vdb.GpuIndex(8, "l2sqr", device=0), vdb.GpuIndex(8, "cosine", device=0)
    u8, wide = vdb.GpuIndex(64, "l2sqr", device=0, scalar="u8"), vdb.GpuIndex(2049, "l2sqr", device=0)
    ix.batch_add(x), other.batch_add(x), cos.batch_add(x), u8.batch_add_u8(np.ones((9, 64), dtype=np.uint8)), wide.batch_add(np.ones((4, 2049), dtype=np.float32))
    for h in (ix, other, cos):
        h.set_labels(0, cl.astype(np.uint32))
    u8.set_labels(0, np.arange(9) % 2), wide.set_labels(0, np.arange(4) % 2)
    ix.set_labels(1, np.full(20, 7)), ix.set_labels(2, np.arange(20))
    ix.set_labels(3, np.where(np.arange(20) < 2, 1, NONE))  # two scored rows in one cluster
    foreign, stale = other.make_mask(np.ones(20, dtype=bool)), other.make_mask(np.ones(20, dtype=bool))
    t_s, t_mean = torch.full((20,), -7.0, dtype=torch.float32, device="cuda"), torch.full((1,), -7.0, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    handles = (ix, other, cos, u8, wide)
    before = [[h.get_stat(s) for s in STATS] for h in handles]
    sil = lambda h, col, **kw: h.silhouette_device(col, t_s.data_ptr(), t_mean.data_ptr(), **kw)
    for call, word in ((lambda: sil(u8, 0), "f32 rows"), (lambda: sil(wide, 0), "1 .. 2048"), (lambda: sil(ix, 5), "column 5 was never written"),
                       (lambda: sil(ix, 16), "columns are 0 .. 15"), (lambda: sil(ix, 0, mask=foreign), "another index"),
                       (lambda: sil(cos, 0, euclidean=True), "on a Cosine table"), (lambda: sil(ix, 1), "1 clusters among 20 scored rows"),
                       (lambda: sil(ix, 2), "20 clusters among 20 scored rows"), (lambda: sil(ix, 3), "1 clusters among 2 scored rows")):
        with pytest.raises(vdb.VdbError, match=word):
            call()
    other.batch_add(x[:1])
    with pytest.raises(vdb.VdbError, match="stale"):
        sil(other, 0, mask=stale)
    assert (t_s == -7.0).all().item() and t_mean[0].item() == -7.0
    assert [[h.get_stat(s) for s in STATS] for h in handles] == before
    for h in (foreign, stale) + handles:
        h.close()
