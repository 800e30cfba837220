"""GPU: VecDB.outlier_scores / find_outliers / knn_graph against a model of the table: tests/lof_ref.py over the rows' integer positions on a
line (exact squared distances), re-read from the table after every edit."""
import math

import numpy as np
import pytest

import lab_1806_vec_db_amd as vdb
import lof_ref as R

pytestmark = pytest.mark.gpu
DIM, K = 16, 3


def _check(db, filt):
    data = db.extract_data("t")  # the model: positions and metadata as the table holds them now
    pos, meta = np.array([v[3] for v, _ in data], dtype=np.float64), [m for _, m in data]
    with np.errstate(invalid="ignore"):
        D = ((pos[:, None] - pos[None, :]) ** 2).astype(np.float32)
    inside = None if filt is None else np.array([m["lang"] == filt["lang"] for m in meta])
    rows, nbr, nd, cnt = R.graph_of_order(*R.order_of_matrix(D), K, inside)
    kdist, _, lof = R.of_lists(nbr, nd, cnt)
    g = db.knn_graph("t", K, filter=filt)
    used = np.arange(K)[None, :] < cnt[:, None]
    assert np.array_equal(g[0], rows) and np.array_equal(g[1], np.where(used, rows[nbr], 0)) and np.array_equal(g[2], np.where(used, nd, 0), equal_nan=True) and np.array_equal(g[3], cnt)
    got = db.outlier_scores("t", K, filter=filt)
    assert np.array_equal(got[0], rows)
    R.close(got[1], lof)
    got = db.outlier_scores("t", K, method="kdist", filter=filt)
    assert np.array_equal(got[0], rows) and np.array_equal(got[1], kdist, equal_nan=True)
    # the ordering rule on the exact scores: score descending, row ascending, NaN last
    order = sorted(range(len(rows)), key=lambda p: (math.isnan(kdist[p]), 0.0 if math.isnan(kdist[p]) else -float(kdist[p]), int(rows[p])))
    for top in (4, len(rows) + 3):
        hits = db.find_outliers("t", K, top=top, method="kdist", filter=filt, with_vectors=True)
        assert [(m, s) for m, s, _ in hits if not math.isnan(s)] == [(meta[rows[p]], float(kdist[p])) for p in order[:top] if not math.isnan(kdist[p])]
        assert [m for m, _, _ in hits] == [meta[rows[p]] for p in order[:top]] and all(np.array_equal(v, data[rows[p]][0], equal_nan=True) for (_, _, v), p in zip(hits, order))
    best = db.find_outliers("t", K, top=1, filter=filt)  # method "lof": the far row stands out (asserted on the model first)
    assert int(np.nanargmax(lof)) == int(np.flatnonzero(pos[rows] == 5000)[0]) and best[0][0] == meta[rows[int(np.nanargmax(lof))]] and len(best[0]) == 2
    return len(rows)


def test_outliers_follow_the_table_through_edits():
    """two chains of ten rows at unit steps, two rows far away and a NaN row, shuffled; added in two batches, then some rows deleted"""
    pos = np.concatenate([[5000], np.random.default_rng(8).permutation(np.concatenate([np.arange(10), 100 + np.arange(10), [1000, np.nan]]))])
    x = np.pad(pos[:, None].astype(np.float32), ((0, 0), (3, DIM - 4)))
    meta = [{"id": str(i), "lang": "de" if p % 100 in (4, 5) else "en"} for i, p in enumerate(pos)]  # (the NaN row and the far rows: "en")
    db = vdb.VecDB()
    db.create_table_if_not_exists("t", DIM, "l2sqr")
    db.batch_add("t", x[:15], [dict(m) for m in meta[:15]])
    sizes = [_check(db, f) for f in (None, {"lang": "en"})]
    db.batch_add("t", x[15:], [dict(m) for m in meta[15:]])
    sizes += [_check(db, f) for f in (None, {"lang": "en"})]
    assert db.delete("t", {"lang": "de"}) == 4
    sizes += [_check(db, f) for f in (None, {"lang": "en"})]
    assert sizes[2:] == [23, 19, 19, 19] and sizes[0] == 15
    with pytest.raises(ValueError):
        db.outlier_scores("t", K, method="zscore")
    assert db.find_outliers("t", K, top=0) == [] and math.isnan(db.outlier_scores("t", K, filter={"id": "0"})[1][0])  # a single matching row
