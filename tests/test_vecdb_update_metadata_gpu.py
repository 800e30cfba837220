"""GPU: VecDB.update_metadata / batch_update_metadata -- the metadata of the rows a pattern matches changed in place.

The model is a list of dicts that the test updates with a test-local function.  After each write count, count_by, get and
search(filter=...) on the table must equal the model's answers (the search against a float64 brute force over the matching rows), and the
live label columns, decoded through the table's dictionary, must equal the model's values.  Also: exactly the cached masks that name a
changed key are dropped; the HNSW graph and the PQ table stay and answer as before; the batch form matches before the call, lets the
last pattern win per key, and makes one library call; refusals; a failed library call changes nothing; later batch_add / delete keep
the columns in step."""
import collections

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N, DIM = 3000, 16
NONE = 0xFFFFFFFF
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


def _table(n=N, seed=61):
    rng = np.random.default_rng(seed)
    vecs = rng.standard_normal((n, DIM)).astype(np.float32)
    meta = [{"id": str(i), "tenant": f"t{i % 7}", "year": str(2020 + i % 4)} for i in range(n)]
    for i in range(0, n, 5):
        meta[i]["lang"] = "en" if i % 2 else "de"
    return rng, vecs, meta


def _match(m, pattern):
    return all(m.get(k) == v for k, v in pattern.items())


def _apply(model, pattern, changes):
    """the test's own statement of update_metadata; returns the number of rows matched"""
    hit = [m for m in model if _match(m, pattern)]
    for m in hit:
        for k, v in changes.items():
            if v is None:
                m.pop(k, None)
            else:
                m[k] = v
    return len(hit)


def _masks_built(db):
    ix = db._t("t").index
    return sum(ix.get_stat(s) for s in MASK_STATS)


def _columns_equal_model(db, model):
    """every live column, decoded through the table's dictionary, holds the model's value of its key for every row"""
    t = db._t("t")
    for key in t.codec.keys():
        col = t.codec.column_of(key)
        inv = {c: v for v, c in t.codec.codes[col].items()}
        got = [None if c == NONE else inv[c] for c in t.index.get_labels(col).tolist()]
        assert got == [m.get(key) for m in model], key


def _check(db, model, vecs, q, filters, fields=("tenant", "year")):
    assert db.get_len("t") == len(model)
    for f in filters:
        rows = [i for i, m in enumerate(model) if _match(m, f)]
        assert db.count("t", f) == len(rows), f
        for field in fields:
            assert db.count_by("t", field, f) == dict(collections.Counter(model[i].get(field) for i in rows)), (f, field)
        got_vecs, got_meta = db.get("t", f)
        assert got_meta == [model[i] for i in rows] and np.array_equal(got_vecs, vecs[rows]), f
        hits = db.search("t", q, 5, filter=f)
        d = ((vecs[rows].astype(np.float64) - q.astype(np.float64)) ** 2).sum(axis=1)
        order = np.argsort(d, kind="stable")[:5]
        assert [m for m, _ in hits] == [model[rows[j]] for j in order], f
        # (f32 folds of DIM squares against float64: relative error of a few DIM * 2^-24)
        assert np.allclose([x for _, x in hits], d[order], rtol=1e-5, atol=1e-6), f
    _columns_equal_model(db, model)


def test_write_shapes(vdb):
    rng, vecs, model = _table()
    db = _fill(vdb, vecs, model)  # (batch_add copies the dicts: the model stays the test's)
    ix = db._t("t").index
    q = rng.standard_normal(DIM).astype(np.float32)
    filters = [{"tenant": "t3"}, {"year": "2021"}, {"tenant": "t1", "year": "2022"}, {}, {"tenant": "nobody"}]
    _check(db, model, vecs, q, filters)  # tenant and year have columns from here on
    assert ix.get_stat("label_columns") == 2
    calls = ix.get_stat("labels_scatter_calls")
    # a value never seen
    assert db.update_metadata("t", {"tenant": "t3"}, {"year": "1999"}) == _apply(model, {"tenant": "t3"}, {"year": "1999"}) == len(range(3, N, 7))
    assert ix.get_stat("labels_scatter_calls") == calls + 1 and ix.get_stat("labels_scatter_rows") == len(range(3, N, 7))
    _check(db, model, vecs, q, filters + [{"year": "1999"}])
    # None removes the key
    assert db.update_metadata("t", {"year": "2021"}, {"tenant": None}) == _apply(model, {"year": "2021"}, {"tenant": None}) > 0
    assert all("tenant" not in m for m in model if m["year"] == "2021")
    _check(db, model, vecs, q, filters + [{"tenant": None}, {"tenant": None, "year": "2021"}])
    # the pattern names the key it changes; two keys at once
    assert db.update_metadata("t", {"tenant": "t1", "year": "2022"}, {"tenant": "t9", "year": "2022b"}) == \
        _apply(model, {"tenant": "t1", "year": "2022"}, {"tenant": "t9", "year": "2022b"}) > 0
    _check(db, model, vecs, q, filters + [{"tenant": "t9"}, {"year": "2022b"}])
    # a changed key without a column: host only, no column made; the column it gets later is encoded from the updated metadata
    calls = ix.get_stat("labels_scatter_calls")
    assert db.update_metadata("t", {"tenant": "t5"}, {"lang": "fr", "note": "moved"}) == _apply(model, {"tenant": "t5"}, {"lang": "fr", "note": "moved"}) > 0
    assert ix.get_stat("label_columns") == 2 and ix.get_stat("labels_scatter_calls") == calls  # nothing to write on the device
    assert db.update_metadata("t", {"lang": "de"}, {"lang": None}) == _apply(model, {"lang": "de"}, {"lang": None}) > 0  # (host loop: no column yet)
    assert ix.get_stat("label_columns") == 2
    _check(db, model, vecs, q, filters + [{"lang": "fr"}, {"lang": "de"}, {"lang": None, "tenant": "t2"}], fields=("tenant", "lang"))
    assert ix.get_stat("label_columns") == 3
    # nothing matched; empty changes: nothing changes, no call, no mask dropped
    cached = set(db._t("t").masks)
    calls = ix.get_stat("labels_scatter_calls")
    assert db.update_metadata("t", {"tenant": "nobody"}, {"year": "3000"}) == 0
    assert db.update_metadata("t", {"tenant": "t2"}, {}) == sum(1 for m in model if m.get("tenant") == "t2") > 0
    assert set(db._t("t").masks) == cached and ix.get_stat("labels_scatter_calls") == calls
    _check(db, model, vecs, q, filters)
    # later writes keep the columns in step: batch_add of rows with old and new values, delete by a changed key
    more = rng.standard_normal((40, DIM)).astype(np.float32)
    more_meta = [{"id": f"n{i}", "tenant": "t9" if i % 2 else "t40", "year": "1999", "lang": "fr"} for i in range(40)]
    db.batch_add("t", more, more_meta)
    vecs = np.concatenate([vecs, more])
    model += [dict(m) for m in more_meta]
    _check(db, model, vecs, q, filters + [{"tenant": "t9"}, {"tenant": "t40", "lang": "fr"}], fields=("tenant", "lang"))
    assert db.update_metadata("t", {"tenant": "t40"}, {"year": "2041"}) == _apply(model, {"tenant": "t40"}, {"year": "2041"}) == 20
    gone = [i for i, m in enumerate(model) if m.get("year") == "1999"]
    assert db.delete("t", {"year": "1999"}) == len(gone) > 0
    got = db.extract_data("t")  # (delete moves rows: the model follows the table's order by id)
    by_id = {m["id"]: (m, vecs[i]) for i, m in enumerate(model) if m.get("year") != "1999"}
    model = [by_id[m["id"]][0] for _, m in got]
    vecs = np.array([by_id[m["id"]][1] for _, m in got], dtype=np.float32)
    assert [m for _, m in got] == model
    _check(db, model, vecs, q, filters + [{"year": "2041"}, {"year": "1999"}], fields=("tenant", "lang"))
    db.delete_table("t")


def test_seventeenth_key_on_the_host_path(vdb):
    rng = np.random.default_rng(62)
    n = 400
    vecs = rng.standard_normal((n, DIM)).astype(np.float32)
    model = [{"id": str(i), **{f"k{j}": str((i + j) % 3) for j in range(17)}} for i in range(n)]
    db = _fill(vdb, vecs, model)
    ix = db._t("t").index
    for j in range(16):
        assert db.count("t", {f"k{j}": "1"}) == sum(1 for m in model if m[f"k{j}"] == "1")
    assert ix.get_stat("label_columns") == 16
    calls = ix.get_stat("labels_scatter_calls")
    # pattern and change on the key that cannot have a column: host loop, host write
    assert db.update_metadata("t", {"k16": "2"}, {"k16": "two"}) == _apply(model, {"k16": "2"}, {"k16": "two"}) > 0
    assert ix.get_stat("labels_scatter_calls") == calls
    # a host-matched pattern that changes a live column and the 17th key together
    assert db.update_metadata("t", {"k16": "two", "k0": "1"}, {"k3": "x", "k16": None}) == _apply(model, {"k16": "two", "k0": "1"}, {"k3": "x", "k16": None}) > 0
    assert ix.get_stat("labels_scatter_calls") == calls + 1
    q = rng.standard_normal(DIM).astype(np.float32)
    _check(db, model, vecs, q, [{"k16": "two"}, {"k16": None}, {"k3": "x"}, {"k3": "x", "k16": "0"}, {"k16": "2"}], fields=("k3", "k16"))
    db.delete_table("t")


def test_mask_cache_drops_exactly_the_filters_that_name_a_changed_key(vdb):
    from lab_1806_vec_db_amd.labels import filter_key

    rng, vecs, model = _table()
    db = _fill(vdb, vecs, model)
    t = db._t("t")
    q = rng.standard_normal(DIM).astype(np.float32)
    tenant_f = [{"tenant": f"t{j}"} for j in range(7)]
    year_f = [{"year": str(2020 + j)} for j in range(4)]
    both = vdb.AnyOf({"tenant": "t1"}, {"year": "2020"})
    for f in tenant_f + year_f + [both, {}, {"tenant": "t2", "year": "2021"}]:
        db.search("t", q, 3, filter=f)
    cached = set(t.masks)
    assert cached == {filter_key(f) for f in tenant_f + year_f + [both, {}, {"tenant": "t2", "year": "2021"}]}
    built = _masks_built(db)
    assert db.update_metadata("t", {"tenant": "t1"}, {"year": "2030"}) == _apply(model, {"tenant": "t1"}, {"year": "2030"})
    assert _masks_built(db) == built  # the pattern's mask came from the cache
    assert set(t.masks) == {filter_key(f) for f in tenant_f + [{}]}  # the year masks, the two-key pattern and the AnyOf over both are gone
    for f in tenant_f:
        db.search("t", q, 3, filter=f)
    db.search("t", q, 3, filter={})
    assert _masks_built(db) == built  # still cached
    hits = db.search("t", q, 3, filter={"year": "2030"})
    assert _masks_built(db) == built + 1  # rebuilt from the updated column
    assert [m["tenant"] for m, _ in hits] == ["t1"] * 3
    db.search("t", q, 3, filter=both)
    assert _masks_built(db) == built + 2
    assert db.count("t", both) == sum(1 for m in model if m.get("tenant") == "t1" or m.get("year") == "2020")
    db.delete_table("t")


def test_hnsw_and_pq_stay_and_answer_as_before(vdb):
    rng, vecs, model = _table(n=1200, seed=63)
    db = _fill(vdb, vecs, model)
    db.count("t", {"tenant": "t0"})  # tenant has a column
    db.build_pq_table("t", m=8)
    db.build_hnsw_index("t", ef_construction=40)
    assert db.has_hnsw_index("t") and db.has_pq_table("t")
    qs = rng.standard_normal((4, DIM)).astype(np.float32)
    before = [db.search("t", q, 5, ef=32) for q in qs]
    assert db.update_metadata("t", {"tenant": "t4"}, {"tenant": "t4b", "seen": "yes"}) == _apply(model, {"tenant": "t4"}, {"tenant": "t4b", "seen": "yes"}) > 0
    assert db.batch_update_metadata("t", [{"tenant": "t2"}], [{"tenant": "t2b"}]) == [_apply(model, {"tenant": "t2"}, {"tenant": "t2b"})]
    assert db.has_hnsw_index("t") and db.has_pq_table("t")
    after = [db.search("t", q, 5, ef=32) for q in qs]
    for b, a in zip(before, after):
        assert [(m["id"], d) for m, d in b] == [(m["id"], d) for m, d in a]  # the same rows at the same distances ...
        assert [m for m, _ in a] == [model[int(m["id"])] for m, _ in a]     # ... with the new metadata
    assert db.count("t", {"tenant": "t4b"}) == len(range(4, 1200, 7)) and db.count("t", {"tenant": "t4"}) == 0
    db.delete_table("t")


def test_batch_form(vdb):
    rng, vecs, model = _table()
    db = _fill(vdb, vecs, model)
    ix = db._t("t").index
    q = rng.standard_normal(DIM).astype(np.float32)
    filters = [{"tenant": "t2"}, {"year": "2021"}, {"lang": "en"}, {}]
    _check(db, model, vecs, q, filters, fields=("tenant", "year", "lang"))  # tenant, year and lang have columns
    patterns = [{"tenant": "t2"}, {"year": "2021"}, {"tenant": "t2"}, {"tenant": "nobody"}, {"id": "7"}, {"lang": "en", "year": "2023"}]
    changes = [{"year": "A", "lang": "x"}, {"year": "B", "tenant": "t2"}, {"year": "C"}, {"year": "never"}, {"note": "seven", "lang": None}, {}]
    # every pattern is matched against the table as it stands BEFORE the call: pattern 2 is also matched by the rows pattern 1 turns
    # into tenant t2, and they do not receive its change; per key the last matching pattern wins
    matched = [[m for m in model if _match(m, p)] for p in patterns]
    want = [len(h) for h in matched]
    assert want[0] > 0 and want[1] > 0 and want[3] == 0 and want[4] == 1 and want[5] > 0
    for hit, ch in zip(matched, changes):
        for m in hit:
            for k, v in ch.items():
                if v is None:
                    m.pop(k, None)
                else:
                    m[k] = v
    calls, rows = ix.get_stat("labels_scatter_calls"), ix.get_stat("labels_scatter_rows")
    built = set(db._t("t").masks)
    assert db.batch_update_metadata("t", patterns, changes) == want
    assert ix.get_stat("labels_scatter_calls") == calls + 1  # ONE library call for the batch
    touched = {id(m) for hit, ch in zip(matched, changes) if ch for m in hit}
    assert ix.get_stat("labels_scatter_rows") == rows + len(touched)  # the union of the matched rows, each once
    assert model[7].get("note") == "seven" and "lang" not in model[7]
    both = [m for m in model if m["id"] in {x["id"] for x in matched[0]} & {x["id"] for x in matched[1]}]
    assert both and all(m["year"] == "C" and m["lang"] == "x" and m["tenant"] == "t2" for m in both)
    assert set(db._t("t").masks) == {k for k in built if k == frozenset()}  # every cached filter named tenant, year or lang; {} stays
    _check(db, model, vecs, q, filters + [{"year": "A"}, {"year": "B"}, {"year": "C"}, {"lang": "x"}, {"year": "never"}], fields=("tenant", "year", "lang"))
    assert db.batch_update_metadata("t", [], []) == []
    # refusals
    for bad in ("id", None, vdb.AnyOf({"id": "1"}, {"id": "2"}), [("id", "1")]):
        with pytest.raises(TypeError):
            db.update_metadata("t", bad, {"year": "x"})
    with pytest.raises(TypeError):
        db.batch_update_metadata("t", [{"id": "1"}, vdb.Not({"id": "2"})], [{"a": "b"}, {"a": "b"}])
    with pytest.raises(RuntimeError, match="differ in length"):
        db.batch_update_metadata("t", [{"id": "1"}, {"id": "2"}], [{"a": "b"}])
    with pytest.raises(RuntimeError, match="differ in length"):
        db.batch_update_metadata("t", [{"id": "1"}], [{"a": "b"}, {"a": "c"}])
    with pytest.raises(RuntimeError, match="not found"):
        db.update_metadata("no such table", {}, {"a": "b"})
    _check(db, model, vecs, q, filters, fields=("tenant", "year", "lang"))
    db.delete_table("t")


def test_a_failed_library_call_leaves_the_table_as_it_was(vdb, monkeypatch):
    rng, vecs, model = _table(n=1000, seed=64)
    db = _fill(vdb, vecs, model)
    ix = db._t("t").index
    q = rng.standard_normal(DIM).astype(np.float32)
    filters = [{"tenant": "t3"}, {"year": "2021"}, {}]
    _check(db, model, vecs, q, filters)
    cached = set(db._t("t").masks)

    def boom(*a, **k):
        raise vdb.VdbError("forced failure")

    monkeypatch.setattr(ix, "set_labels_mask", boom)
    monkeypatch.setattr(ix, "set_labels_rows", boom)
    with pytest.raises(vdb.VdbError, match="forced"):
        db.update_metadata("t", {"tenant": "t3"}, {"year": "2077", "note": "x"})
    with pytest.raises(vdb.VdbError, match="forced"):
        db.batch_update_metadata("t", [{"tenant": "t3"}, {"year": "2021"}], [{"year": "2077"}, {"tenant": "t8"}])
    monkeypatch.undo()
    assert [m for _, m in db.extract_data("t")] == model and set(db._t("t").masks) == cached
    _check(db, model, vecs, q, filters + [{"year": "2077"}, {"tenant": "t8"}])
    assert db.update_metadata("t", {"tenant": "t3"}, {"year": "2077"}) == _apply(model, {"tenant": "t3"}, {"year": "2077"})  # the table still takes writes
    _check(db, model, vecs, q, filters + [{"year": "2077"}])
    db.delete_table("t")
