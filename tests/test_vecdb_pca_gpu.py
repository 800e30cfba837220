"""GPU: VecDB.fit_pca / transform / reduce on a table of exactly rank 3: 600 rows x 40 dims, Z B + offset with B three orthonormal rows of
+-1/4 scaled 10, 5, 2, Z in multiples of 1/64 and an integer offset, so every element is exact in f32 and dimensions 4 .. 40 of the
covariance carry rounding only."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

U = 2.0 ** -53


@pytest.fixture(scope="module")
def table():
    import lab_1806_vec_db_amd as vdb

    rng = np.random.default_rng(0)
    s = np.arange(16)
    B = np.zeros((3, 40))
    B[0, :16], B[1, :16], B[2, :16] = 0.25, np.where(s & 1, -0.25, 0.25), np.where(s & 2, -0.25, 0.25)
    x64 = (np.round(rng.standard_normal((600, 3)) * 64) / 64) @ (B * np.array([[10.0], [5.0], [2.0]])) + (np.arange(40) % 7 - 3)
    x = x64.astype(np.float32)
    assert np.array_equal(x.astype(np.float64), x64)
    db = vdb.VecDB()
    db.create_table_if_not_exists("t", 40, "l2sqr")
    db.batch_add("t", x, [{"id": str(r), "tenant": "a" if r % 5 < 2 else "b"} for r in range(600)])
    return db, x64


def _sign_fixed_eigh(cov, n):
    w, v = np.linalg.eigh(cov)
    comp = v[:, ::-1].T[:n].copy()
    for c in comp:
        if c[np.argmax(np.abs(c))] < 0:
            c *= -1.0
    return w[::-1][:n], comp.astype(np.float32)


def test_fit_pca(table):
    db, x = table
    model = db.fit_pca("t", 3)
    mean, cov, m = db._t("t").index.covariance()
    w, comp = _sign_fixed_eigh(cov, 3)
    assert model.n_rows == m == 600 and model.center and (np.diff(model.explained_variance) < 0).all()
    assert np.array_equal(model.components.view(np.uint32), comp.view(np.uint32)) and np.array_equal(model.explained_variance, w)
    assert np.array_equal(model.mean, mean) and model.components.dtype == np.float32
    D = x - x.mean(0)
    bound = 40 * 2 * (m + 8) * U * np.trace(np.abs(D).T @ np.abs(D)) / np.trace(D.T @ D)
    print("ratio sum - 1", model.explained_variance_ratio.sum() - 1, "bound", bound)
    assert abs(model.explained_variance_ratio.sum() - 1) <= bound
    with pytest.raises(ValueError, match="n_components"):
        db.fit_pca("t", 41)


def test_fit_pca_under_a_filter(table):
    db, x = table
    rows = np.array([r % 5 < 2 for r in range(600)])
    model = db.fit_pca("t", 2, filter={"tenant": "a"})
    assert model.n_rows == rows.sum() == 240 and model.components.shape == (2, 40)
    assert (np.abs(model.mean - x[rows].mean(0)) <= 2 * (240 + 8) * U * np.abs(x[rows]).mean(0)).all()


def test_reduce_keeps_the_neighbours(table):
    db, x = table
    model = db.reduce("t", "t3", 3)
    assert db.get_len("t3") == 600 and db.get_dim("t3") == 3 and db.get_dist("t3") == "l2sqr"
    assert db._t("t3").metadata == db._t("t").metadata and db._t("t3").metadata[7] is not db._t("t").metadata[7]
    for q in range(0, 600, 30):
        d = np.sort(((x - x[q]) ** 2).sum(1))
        assert d[5] - d[4] > 1e-3 * d[4]  # the data alone keeps the 5th and 6th neighbour apart
        want = {h[0]["id"] for h in db.search("t", x[q], 5)}
        assert {h[0]["id"] for h in db.search("t3", db.transform(model, x[q])[0], 5)} == want and len(want) == 5
    with pytest.raises(RuntimeError, match="already exists"):
        db.reduce("t", "t3", model)
    half = db.reduce("t", "t2", model, filter={"tenant": "b"})  # a given model, the filter's rows only, compact
    assert half is model and db.get_len("t2") == 360 and all(md["tenant"] == "b" for md in db._t("t2").metadata)
