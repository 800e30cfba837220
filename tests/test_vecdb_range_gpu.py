"""GPU: VecDB.search_within returns the complete set inside the bound -- what search(k = len, upper_bound = r) returns -- on the
scenarios of test_vecdb_gpu.py, with an HNSW index and a PQ table present and after delete."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def test_pyo3_scenario_with_hnsw_and_pq():
    from lab_1806_vec_db_amd.vecdb import VecDB

    db = VecDB()
    db.create_table_if_not_exists("table_1", 4)
    db.add("table_1", [1.0, 0.0, 0.0, 0.0], {"content": "a"})
    db.add("table_1", [0.0, 1.0, 0.0, 0.0], {"content": "b"})
    db.build_hnsw_index("table_1")
    db.add("table_1", [0.0, 0.0, 1.0, 0.0], {"content": "c"})
    db.add("table_1", [0.0, 0.0, 1.0, 1.0], {"content": "d", "type": "oops"})
    q = [1.0, 0.0, 0.0, 0.0]
    n = db.get_len("table_1")
    assert db.search_within("table_1", q, 0.5) == db.search("table_1", q, n, None, 0.5)  # HNSW present
    assert [m["content"] for m, _ in db.search_within("table_1", [0.0, 0.0, 1.0, 0.0], 0.5)] == ["c", "d"]
    db.delete("table_1", {"type": "oops"})
    db.build_hnsw_index("table_1")
    db.build_pq_table("table_1")
    assert db.has_hnsw_index("table_1") and db.has_pq_table("table_1")
    n = db.get_len("table_1")
    res = db.search_within("table_1", q, 0.5)
    assert len(res) == 1 and res[0][0]["content"] == "a"
    assert res == db.search("table_1", q, n, None, 0.5)
    res = db.search_within("table_1", q, 1.0)  # boundary inclusive: the orthogonal rows at distance exactly 1, ties by row
    assert [(m["content"], d) for m, d in res] == [("a", 0.0), ("b", 1.0), ("c", 1.0)]
    assert sorted(m["content"] for m, _ in db.search("table_1", q, n, None, 1.0)) == ["a", "b", "c"]
    assert db.search_within("table_1", q, 1.0, limit=2) == res[:2]
    assert db.search_within("table_1", q, float("nan")) == [] and db.search_within("table_1", q, -1.0) == []
    with pytest.raises(RuntimeError):
        db.search_within("nope", q, 1.0)


def test_l2_table_after_delete_equals_search():
    from lab_1806_vec_db_amd.vecdb import VecDB

    db = VecDB()
    db.create_table_if_not_exists("t", 8, "l2sqr")
    rng = np.random.default_rng(0)
    rows = rng.standard_normal((50, 8)).astype(np.float32)
    db.batch_add("t", rows, [{"i": str(i), "par": str(i % 2)} for i in range(50)])
    db.add("t", rows[0], {"i": "50", "par": "0"})
    db.build_hnsw_index("t", 50)
    db.build_pq_table("t", 0.5, None, 4)
    assert db.delete("t", {"par": "1"}) == 25  # clears HNSW and PQ: search is FlatIndex::knn again
    n = db.get_len("t")
    for qi in (2, 0, 10):
        everything = db.search("t", rows[qi], n)
        assert len(everything) == n
        for ub in (everything[0][1], everything[4][1], everything[n // 2][1], np.nextafter(np.float32(everything[4][1]), np.float32(0)),
                   float("inf")):
            want = db.search("t", rows[qi], n, upper_bound=ub)
            assert db.search_within("t", rows[qi], ub) == want
            assert db.search_within("t", rows[qi], ub, limit=3) == db.search("t", rows[qi], 3, upper_bound=ub)
    # rows[0] is in the table twice ("0" and "50"): both at distance 0
    assert sorted(m["i"] for m, d in db.search_within("t", rows[0], 0.0)) == ["0", "50"]
    # with the indexes back the answer is still the exact one
    db.build_hnsw_index("t", 50)
    db.build_pq_table("t", 0.5, None, 4)
    db.clear_hnsw_index("t")
    flat = db.search("t", rows[2], n, upper_bound=5.0)
    db.build_hnsw_index("t", 50)
    assert db.search_within("t", rows[2], 5.0) == flat
