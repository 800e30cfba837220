"""GPU: VecDB.cluster -- k-means under a filter, the cluster ids written as decimal strings into a metadata key -- through the calls the ids
are for: count_by equals the sizes, filter={field: v} returns only rows of cluster v, group_by=field caps the hits per cluster, rows outside
the filter keep their value, a second call overwrites.  The table is four blobs far apart, so the clusters are the blobs."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

DIM, N = 16, 400


def _table(vdb):
    rng = np.random.default_rng(41)
    blob = np.arange(N) % 4
    x = (np.eye(4, DIM)[blob] * 8 + rng.standard_normal((N, DIM)) * 0.1).astype(np.float32)
    db = vdb.VecDB()
    db.create_table_if_not_exists("t", DIM, "l2sqr")
    db.batch_add("t", x, [{"id": str(i), "lang": ("en", "de")[i % 8 < 4], "topic": "old"} for i in range(N)])
    return db, x, blob


@pytest.mark.parametrize("filt", (None, {"lang": "en"}))
def test_cluster_ids_work_with_filter_group_by_and_count_by(filt):
    import lab_1806_vec_db_amd as vdb

    db, x, blob = _table(vdb)
    inside = np.array([filt is None or i % 8 >= 4 for i in range(N)])
    db.search("t", x[0], 3, filter={"topic": "old"})  # a cached mask that names the field, and one that does not
    db.search("t", x[0], 3, filter={"lang": "de"})
    cent, sizes = db.cluster("t", 4, "topic", filter=filt, seed=1)
    meta = [m for _, m in db.extract_data("t")]
    topic = np.array([m["topic"] for m in meta])
    assert cent.shape == (4, DIM) and sizes.sum() == inside.sum() and (topic[~inside] == "old").all()
    # the clusters are the blobs: one id per blob among the clustered rows
    ids = {b: set(topic[inside & (blob == b)].tolist()) for b in range(4)}
    assert all(len(v) == 1 for v in ids.values()) and set().union(*ids.values()) == {"0", "1", "2", "3"}
    cb = db.count_by("t", "topic")
    assert {k: v for k, v in cb.items() if k != "old"} == {str(j): int(sizes[j]) for j in range(4)} and cb.get("old", 0) == (~inside).sum()
    for v in ("0", "3"):
        hits = db.search("t", x[1], N, filter={"topic": v})
        assert len(hits) == int(sizes[int(v)]) and all(m["topic"] == v for m, _ in hits)
    hits = db.search("t", x[1], 8, group_by="topic", group_size=2, filter=filt)
    assert len(hits) == 8 and all([m["topic"] for m, _ in hits].count(str(j)) == 2 for j in range(4))
    assert db.search("t", x[0], 3, filter={"lang": "de"})[0][0]["lang"] == "de"
    # a second call on the same field overwrites: two clusters, every row
    _, sizes2 = db.cluster("t", 2, "topic")
    topic2 = [m["topic"] for _, m in db.extract_data("t")]
    assert set(topic2) == {"0", "1"} and db.count_by("t", "topic") == {"0": int(sizes2[0]), "1": int(sizes2[1])}
