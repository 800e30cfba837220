"""GPU: VecDB.silhouette / silhouette_samples on three separated Gaussian blobs of 50 rows x 24 dims, against the float64 reference and
bound of test_flat_silhouette_gpu."""
import numpy as np
import pytest
from test_flat_silhouette_gpu import _reference

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", params=("l2sqr", "cosine"))
def table(request):
    import lab_1806_vec_db_amd as vdb

    rng = np.random.default_rng(1)
    blob = rng.permutation(np.arange(150) % 3)
    x = (np.eye(3, 24) * 9 + 1)[blob] + rng.standard_normal((150, 24)) * 0.2
    x = x.astype(np.float32)
    mixed = rng.permutation(blob)
    db = vdb.VecDB()
    db.create_table_if_not_exists("t", 24, request.param)
    db.batch_add("t", x, [{"id": str(r), "half": "lo" if r < 90 else "hi", "mixed": str(m)} for r, m in enumerate(mixed.tolist())])
    db.cluster("t", 3, "found", seed=2)
    return db, x, blob, mixed, request.param


def _codes(values):
    return np.unique(np.asarray(values), return_inverse=True)[1].astype(np.uint32)


def _agrees(db, x, field, metric, **kw):
    """silhouette and silhouette_samples against the reference over the rows they report; returns the answer"""
    out = db.silhouette("t", field, **kw)
    rows, s = db.silhouette_samples("t", field, **kw)
    meta = db.get("t")[1]
    values = [meta[r][field] for r in rows.tolist()]
    want, tol, _ = _reference(x[rows], _codes(values), metric, metric == "l2sqr")
    assert out["rows"] == len(rows) and (np.abs(s - want) <= tol).all() and abs(out["mean"] - want.mean()) <= tol.mean()
    for v, (mean, size) in out["by_value"].items():
        pick = np.array(values) == v
        assert size == pick.sum() and abs(mean - want[pick].mean()) <= tol[pick].mean()
    assert sum(size for _, size in out["by_value"].values()) == len(rows)
    return out, rows


def test_found_clusters_score_near_one_and_shuffled_labels_near_zero(table):
    db, x, blob, mixed, metric = table
    out, _ = _agrees(db, x, "found", metric)  # euclidean=None: the root on l2sqr, the table's distance on cosine
    assert len(out["by_value"]) == 3 and out["mean"] > 0.8
    out, _ = _agrees(db, x, "mixed", metric)
    assert abs(out["mean"]) < 0.2


def test_filter_and_sample(table):
    db, x, blob, mixed, metric = table
    _, rows = _agrees(db, x, "found", metric, filter={"half": "lo"})
    assert rows.tolist() == list(range(90))
    _, rows = _agrees(db, x, "found", metric, sample=40, seed=5)
    assert rows.tolist() == sorted(np.random.default_rng(5).choice(np.arange(150), 40, replace=False).tolist())
    _, rows = _agrees(db, x, "found", metric, filter={"half": "hi"}, sample=25, seed=6)
    assert rows.tolist() == sorted(np.random.default_rng(6).choice(np.arange(90, 150), 25, replace=False).tolist())
    assert _agrees(db, x, "found", metric, sample=1000)[1].size == 150


def test_a_field_without_a_label_column_raises(table):
    import lab_1806_vec_db_amd as vdb

    db, x, blob, mixed, metric = table
    with pytest.raises(vdb.VdbError, match="Cosine table" if metric == "cosine" else "clusters among"):
        db.silhouette("t", "found" if metric == "cosine" else "id", euclidean=True)  # the flag on cosine; one value per row on l2sqr
    for i in range(16):
        db.count_by("t", f"extra{i}")  # the columns run out
    with pytest.raises(ValueError, match="no label column"):
        db.silhouette("t", "one_more")
