"""GPU: VecDB.update / batch_update -- new vectors for the rows a metadata pattern matches, in place.

After every call extract_data must equal a test-local list, and search, batch_search(filters=[...]), search_within and group_by must
return exactly what a FRESH VecDB filled with the updated data returns.  Also: the matches per pattern, last pattern wins, the HNSW
index and the PQ table cleared by a match and left alone without one, the table's mask cache left alone (a repeated multi-tenant
batch_search builds no mask after a batch_update, and does after a delete), a 17th key's host-loop pattern, the errors."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

MASK_STATS = ("mask_where_masks", "mask_where_set_masks", "mask_where_any_masks", "mask_combine_masks", "mask_partition_masks")


@pytest.fixture(scope="module")
def vdb():
    import lab_1806_vec_db_amd as v
    return v


def _fill(vdb, vecs, meta):
    db = vdb.VecDB()
    db.create_table_if_not_exists("t", vecs.shape[1], "l2sqr")
    db.batch_add("t", vecs, meta)
    return db


def _mask_stats(db):
    ix = db._t("t").index
    return {s: ix.get_stat(s) for s in MASK_STATS}


def _same_answers(vdb, db, vecs, meta, qs, filters):
    """every kind of search on `db` against a fresh VecDB filled with (vecs, meta)"""
    fresh = _fill(vdb, vecs, meta)
    for q in qs[:3]:
        assert db.search("t", q, 5) == fresh.search("t", q, 5)
        assert db.search("t", q, 5, filter=filters[0]) == fresh.search("t", q, 5, filter=filters[0])
    assert db.batch_search("t", qs, 5) == fresh.batch_search("t", qs, 5)
    got = db.batch_search("t", qs, 5, filters=filters)
    assert got == fresh.batch_search("t", qs, 5, filters=filters)
    ub = got[0][2][1]  # the third distance of the first query under its filter
    assert db.search_within("t", qs[0], ub) == fresh.search_within("t", qs[0], ub)
    assert db.search_within("t", qs[0], ub, filter=filters[0]) == fresh.search_within("t", qs[0], ub, filter=filters[0])
    assert db.batch_search("t", qs, 4, group_by="tenant", group_size=1) == fresh.batch_search("t", qs, 4, group_by="tenant", group_size=1)
    assert db.search("t", qs[1], 4, filter=filters[1], group_by="id") == fresh.search("t", qs[1], 4, filter=filters[1], group_by="id")
    fresh.delete_table("t")
    return got


def test_update_small_table(vdb):
    rng = np.random.default_rng(51)
    n, dim = 300, 32
    vecs = rng.standard_normal((n, dim)).astype(np.float32)
    meta = [{"id": str(i), "tenant": f"t{i % 8}"} for i in range(n)]
    db = _fill(vdb, vecs, meta)
    ix = db._t("t").index
    qs = rng.standard_normal((12, dim)).astype(np.float32)
    filters = [{"tenant": f"t{q % 8}"} for q in range(12)]

    def check():
        data = db.extract_data("t")
        assert [m for _, m in data] == meta and np.array_equal(np.array([v for v, _ in data], dtype=np.float32), vecs)
        assert db.get_len("t") == n
        return _same_answers(vdb, db, vecs, meta, qs, filters)

    def new():
        return rng.standard_normal(dim).astype(np.float32)

    # by id, before any key has a label column: the host loop
    v = new()
    assert ix.get_stat("label_columns") == 0
    assert db.update("t", {"id": "17"}, v) == 1
    assert ix.get_stat("label_columns") == 0  # an update gives no key a column
    vecs[17] = v
    qs[0] = v + np.float32(1e-3)
    filters[0] = {"tenant": "t1"}  # (17 % 8)
    got = check()
    assert got[0][0][0] == meta[17]
    assert ix.get_stat("update_calls") == 1 and ix.get_stat("update_rows") == 1
    # by tenant: the cached mask of the searches above
    s0 = _mask_stats(db)
    v = new()
    assert db.update("t", {"tenant": "t3"}, v) == len(range(3, n, 8))
    assert _mask_stats(db) == s0  # the matches came from the cache
    vecs[3::8] = v
    check()
    # nothing matches: 0, no library call, a built HNSW index and PQ table stay
    db.build_hnsw_index("t", ef_construction=40)
    db.build_pq_table("t", m=8)
    calls = ix.get_stat("update_calls")
    assert db.update("t", {"id": "no such id"}, new()) == 0
    assert db.batch_update("t", [{"tenant": "nobody"}, {"id": "5", "tenant": "t6"}], [new(), new()]) == [0, 0]
    assert db.has_hnsw_index("t") and db.has_pq_table("t") and ix.get_stat("update_calls") == calls
    # a match clears both, as delete does
    v = new()
    assert db.update("t", {"id": "5", "tenant": "t5"}, v) == 1
    vecs[5] = v
    assert not db.has_hnsw_index("t") and not db.has_pq_table("t")
    check()
    # two patterns hit one row: the LAST one's vector
    va, vb, vc = new(), new(), new()
    assert db.batch_update("t", [{"tenant": "t2"}, {"id": "10"}, {"id": "18"}, {"tenant": "t2"}, {"id": "7"}], [va, vb, vc, vb, vc]) == \
        [len(range(2, n, 8)), 1, 1, len(range(2, n, 8)), 1]
    vecs[2::8] = vb  # the second tenant pattern overrides the first one and both id patterns (10 and 18 are tenant t2's)
    vecs[7] = vc
    calls += 2
    assert ix.get_stat("update_calls") == calls  # ONE library call for the batch
    check()
    assert db.batch_update("t", [{"tenant": "t2"}, {"id": "10"}], [va, vc]) == [len(range(2, n, 8)), 1]
    vecs[2::8] = va
    vecs[10] = vc
    check()
    assert db.batch_update("t", [], []) == []
    # errors
    for bad in ("id", None, vdb.AnyOf({"id": "1"}, {"id": "2"}), [("id", "1")]):
        with pytest.raises(TypeError):
            db.update("t", bad, new())
    with pytest.raises(TypeError):
        db.batch_update("t", [{"id": "1"}, vdb.Not({"id": "2"})], [new(), new()])
    with pytest.raises(RuntimeError, match="Dimension mismatch: table dim 32"):
        db.update("t", {"id": "1"}, np.zeros(31, dtype=np.float32))
    with pytest.raises(RuntimeError, match="Dimension mismatch: table dim 32"):
        db.batch_update("t", [{"id": "1"}, {"id": "2"}], np.zeros((2, 33), dtype=np.float32))
    with pytest.raises(RuntimeError, match="differ in length"):
        db.batch_update("t", [{"id": "1"}], np.zeros((2, 32), dtype=np.float32))
    with pytest.raises(RuntimeError, match="not found"):
        db.update("nope", {"id": "1"}, new())
    check()  # and none of them changed anything
    db.delete_table("t")


def test_update_by_a_17th_key(vdb):
    """sixteen keys hold the index's label columns; a pattern on a 17th one is matched by the host loop"""
    rng = np.random.default_rng(52)
    n, dim = 200, 32
    vecs = rng.standard_normal((n, dim)).astype(np.float32)
    meta = [{"id": str(i), "tenant": f"t{i % 8}", **{f"k{j}": str(i % (j + 2)) for j in range(16)}} for i in range(n)]
    db = _fill(vdb, vecs, meta)
    ix = db._t("t").index
    for j in range(15):
        db.search("t", vecs[0], 2, filter={f"k{j}": "0"})
    db.search("t", vecs[0], 2, filter={"tenant": "t0"})
    assert ix.get_stat("label_columns") == 16
    s0 = _mask_stats(db)
    v = rng.standard_normal(dim).astype(np.float32)
    assert db.update("t", {"k15": "3", "tenant": "t1"}, v) == sum(1 for i in range(n) if i % 17 == 3 and i % 8 == 1)
    assert _mask_stats(db) == s0 and ix.get_stat("label_columns") == 16
    for i in range(n):
        if i % 17 == 3 and i % 8 == 1:
            vecs[i] = v
    data = db.extract_data("t")
    assert [m for _, m in data] == meta and np.array_equal(np.array([x for x, _ in data], dtype=np.float32), vecs)
    qs = np.stack([v + np.float32(1e-3), vecs[9]])
    _same_answers(vdb, db, vecs, meta, qs, [{"tenant": "t1"}, {"k15": "3"}])
    db.delete_table("t")


def test_update_big_table_keeps_the_mask_cache(vdb):
    """20 000 x 128: the unfiltered batch and the large tenant's filter run the 8-bit tier; the cached masks survive a batch_update"""
    rng = np.random.default_rng(53)
    n, dim = 20000, 128
    off = rng.standard_normal(dim) * 0.5
    vecs = (rng.standard_normal((n, dim)) + off).astype(np.float32)
    tenant = ["big" if i % 5 < 3 else f"t{i % 5}" for i in range(n)]  # 12 000 rows / 4000 / 4000
    gid = np.arange(n) % 199  # (199 and 5 are coprime: every group has rows of every tenant)
    meta = [{"id": str(i), "tenant": tenant[i], "group": f"g{gid[i]}"} for i in range(n)]
    db = _fill(vdb, vecs, meta)
    ix = db._t("t").index
    nq = 64
    qs = (rng.standard_normal((nq, dim)) + off).astype(np.float32)
    filters = [{"tenant": ("big", "t3", "t4", "big")[q % 4]} for q in range(nq)]
    db.batch_search("t", qs, 5, filters=filters)  # the tenants' masks are cached
    db.search("t", qs[0], 3, filter={"group": "g0"})  # "group" has a column
    gsel = list(range(0, 199, 10))  # 20 groups of 100 or 101 rows
    groups = [f"g{g}" for g in gsel]
    sizes = [int((gid == g).sum()) for g in gsel]
    new = (rng.standard_normal((len(groups), dim)) + off).astype(np.float32)
    f0 = ix.get_stat("flat_filtered_i8_queries")
    assert db.batch_update("t", [{"group": g} for g in groups], new) == sizes
    assert ix.get_stat("update_calls") == 1 and ix.get_stat("update_rows") == sum(sizes)
    for j, g in enumerate(gsel):
        vecs[gid == g] = new[j]
    qs[:20] = new + np.float32(1e-3)
    s1 = _mask_stats(db)
    got = db.batch_search("t", qs, 5, filters=filters)
    assert _mask_stats(db) == s1  # no mask was rebuilt ...
    assert ix.get_stat("flat_filtered_i8_queries") > f0  # ... and the large tenant's went through the 8-bit tier, on rebuilt constants
    for j in range(20):  # the 100 rows that now hold new[j]: the query's tenant's among them come first, at the same distance
        assert got[j][0][0]["group"] == groups[j] and got[j][0][0]["tenant"] == filters[j]["tenant"]
    for i in (0, 10, 190, 199, 19900, n - 1):
        assert np.array_equal(ix[i], vecs[i])
    fresh = _fill(vdb, vecs, meta)
    assert got == fresh.batch_search("t", qs, 5, filters=filters)
    assert db.batch_search("t", qs, 5) == fresh.batch_search("t", qs, 5)
    assert db.batch_search("t", qs[:8], 4, filters=filters[:8], group_by="group") == fresh.batch_search("t", qs[:8], 4, filters=filters[:8], group_by="group")
    ub = got[0][4][1]
    assert db.search_within("t", qs[0], ub, filter=filters[0]) == fresh.search_within("t", qs[0], ub, filter=filters[0])
    fresh.delete_table("t")
    # a delete DOES drop the cache: the same search builds masks again
    assert db.delete("t", {"id": "1"}) == 1
    s2 = _mask_stats(db)
    db.batch_search("t", qs, 5, filters=filters)
    assert _mask_stats(db) != s2
    db.delete_table("t")
