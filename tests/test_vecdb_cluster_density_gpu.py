"""GPU: VecDB.cluster_density against a model of the table: tests/dbscan_ref.py over the rows' integer positions on a line (exact distances)."""
import collections

import numpy as np
import pytest

import dbscan_ref as R
import lab_1806_vec_db_amd as vdb

pytestmark = pytest.mark.gpu
DIM, N = 16, 30


@pytest.mark.parametrize("filt", (None, {"lang": "en"}))
def test_cluster_density_against_the_model(filt):
    """two chains of ten rows at unit steps and ten rows far away, shuffled: inner rows core, chain ends border, the rest noise"""
    pos = np.random.default_rng(6).permutation(np.concatenate([np.arange(10), 100 + np.arange(10), 1000 * np.arange(1, 11)]))
    x = np.pad(pos[:, None].astype(np.float32), ((0, 0), (3, DIM - 4)))
    model = [{"id": str(i), "lang": "en" if pos[i] % 100 < 7 else "de", "topic": "old"} for i in range(N)]
    db = vdb.VecDB()
    db.create_table_if_not_exists("t", DIM, "l2sqr")
    db.batch_add("t", x, [dict(m) for m in model])
    inside = np.array([filt is None or m["lang"] == "en" for m in model])
    label, kind, stats = R.of_matrix(((pos[:, None] - pos[None, :]) ** 2).astype(np.float32), 1.0, 3, inside)
    assert stats["clusters"] == 2 and min(stats[k] for k in ("core", "border", "noise")) >= 1  # a condition on the input
    names = sorted(set(label[kind >= 2].tolist()))  # the clusters ordered by lowest core row
    for r in np.flatnonzero(inside).tolist():
        model[r].pop("topic")
        if kind[r] >= 2:
            model[r]["topic"] = str(names.index(int(label[r])))
    for f in ({"topic": "old"}, {"topic": "0"}, {"lang": "de"}):  # cached masks: two that name the field, one that does not
        db.search("t", x[0], 3, filter=f)
    cached = set(db._t("t").masks)
    got = db.cluster_density("t", 1.0, 3, "topic", filter=filt)
    assert {k: got[k] for k in R.STATS[:4]} == {k: stats[k] for k in R.STATS[:4]} and got["sizes"].tolist() == [int((label[kind >= 2] == v).sum()) for v in names]
    assert [m for _, m in db.extract_data("t")] == model  # written for clustered rows, removed from noise rows, kept outside the filter
    naming = {k for k in cached if "topic" in {f for f, _ in k}}
    assert len(naming) == 2 and not naming & set(db._t("t").masks) and cached - naming <= set(db._t("t").masks)  # only those are dropped
    assert db.count_by("t", "topic") == dict(collections.Counter(m.get("topic") for m in model))
    hits = db.search("t", x[0], N, filter={"topic": "1"})
    assert sorted(m["id"] for m, _ in hits) == sorted(m["id"] for m in model if m.get("topic") == "1") and len(hits) == got["sizes"][1]
