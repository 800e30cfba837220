"""GPU: VecDB.upsert / batch_upsert / get_by -- the write and the fetch by a key field -- and the label_lookup routing of
_Table.match_rows behind batch_update.

The model is a list of [vector, dict] that the test upserts into with a plain Python loop.  After each write extract_data, get_by
(present, absent and never-seen values, with and without vectors), count_by and a filtered search on another key must equal the
model's answers (the search against a float64 brute force over the matching rows); updated rows keep their row ids (the model's
positions); the mask cache keeps exactly what the rule says; one batch is one label_lookup call.  Also: a key that is not unique and a
dict without the key raise with nothing changed; a 17th key and a column with an unhashable value take the host route with the same
answers; batch_update finds the same rows with the lookup routing on and off; the HNSW graph and the PQ table are cleared or kept."""
import collections

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N, DIM = 300, 8
NONE = 0xFFFFFFFF
MASK_STATS = ("mask_where_masks", "mask_where_set_masks", "mask_where_any_masks", "mask_combine_masks", "mask_partition_masks")


@pytest.fixture(scope="module")
def vdb():
    import lab_1806_vec_db_amd as v
    return v


def _meta(i, prefix=""):
    return {"id": f"{prefix}{i}", "tenant": f"t{i % 7}", "year": str(2020 + i % 4)}


def _table(vdb, n=N, seed=71, meta=None):
    rng = np.random.default_rng(seed)
    vecs = rng.standard_normal((n, DIM)).astype(np.float32)
    meta = [_meta(i) for i in range(n)] if meta is None else meta
    db = vdb.VecDB()
    db.create_table_if_not_exists("t", DIM, "l2sqr")
    db.batch_add("t", vecs, meta)
    return rng, db, [[vecs[i], dict(meta[i])] for i in range(n)]


def _upsert(model, id_field, vecs, metas):
    """the test's own statement of batch_upsert; returns (updated, added)"""
    last = {m[id_field]: i for i, m in enumerate(metas)}
    upd = add = 0
    for i, m in enumerate(metas):
        if last[m[id_field]] != i:
            continue  # a later entry names the same value: that one wins
        rows = [r for r, (_, d) in enumerate(model) if d.get(id_field) == m[id_field]]
        assert len(rows) <= 1
        if rows:
            model[rows[0]] = [np.asarray(vecs[i], dtype=np.float32), dict(m)]
            upd += 1
        else:
            model.append([np.asarray(vecs[i], dtype=np.float32), dict(m)])
            add += 1
    return upd, add


def _masks_built(db):
    ix = db._t("t").index
    return sum(ix.get_stat(s) for s in MASK_STATS)


def _columns_equal_model(db, model):
    t = db._t("t")
    for key in t.codec.keys():
        col = t.codec.column_of(key)
        inv = {c: v for v, c in t.codec.codes[col].items()}
        got = [None if c == NONE else inv.get(c, "?") for c in t.index.get_labels(col).tolist()]
        want = [d.get(key) for _, d in model]
        assert [g for g, w in zip(got, want) if isinstance(w, (str, type(None)))] == [w for w in want if isinstance(w, (str, type(None)))], key


def _check(db, model, q, id_field="id", asked=(), filters=({"tenant": "t3"}, {"year": "2021"})):
    assert db.get_len("t") == len(model)
    data = db.extract_data("t")
    assert [d for _, d in data] == [d for _, d in model]
    assert np.array_equal(np.array([v for v, _ in data], dtype=np.float32).reshape(len(model), DIM), np.array([v for v, _ in model]).reshape(len(model), DIM))
    # get_by: present values (one repeated), an absent one the dictionary may know, a never-seen one
    values = [d[id_field] for _, d in model[:: max(len(model) // 9, 1)] if isinstance(d.get(id_field), str)] + list(asked) + ["never-seen-value"]
    values = values + values[:1]
    want = [[r for r, (_, d) in enumerate(model) if d.get(id_field) == v] for v in values]
    got = db.get_by("t", id_field, values)
    assert got == [[(model[r][1],) for r in rows] for rows in want]
    got = db.get_by("t", id_field, values, with_vectors=True)
    assert [[m for m, _ in e] for e in got] == [[model[r][1] for r in rows] for rows in want]
    assert all(np.array_equal(v, model[r][0]) for e, rows in zip(got, want) for (_, v), r in zip(e, rows))
    by_tenant = db.get_by("t", "tenant", ["t2", "nobody"])
    assert by_tenant == [[(d,) for _, d in model if d.get("tenant") == "t2"], []]
    assert db.count_by("t", "tenant") == dict(collections.Counter(d.get("tenant") for _, d in model))
    for f in filters:
        rows = [i for i, (_, d) in enumerate(model) if all(d.get(k) == v for k, v in f.items())]
        hits = db.search("t", q, 5, filter=f)
        x = np.array([model[i][0] for i in rows], dtype=np.float64).reshape(len(rows), DIM)
        dd = ((x - q.astype(np.float64)) ** 2).sum(axis=1)
        order = np.argsort(dd, kind="stable")[:5]
        assert [m for m, _ in hits] == [model[rows[j]][1] for j in order], f
        # (f32 folds of DIM squares against float64: relative error of a few DIM * 2^-24)
        assert np.allclose([d for _, d in hits], dd[order], rtol=1e-5, atol=1e-6), f
    _columns_equal_model(db, model)


def test_write_shapes(vdb):
    rng, db, model = _table(vdb)
    ix = db._t("t").index
    q = rng.standard_normal(DIM).astype(np.float32)
    assert db.count("t", {"tenant": "t3"}) > 0 and db.count("t", {"year": "2021"}) > 0  # tenant and year have columns; id has none
    assert ix.get_stat("label_columns") == 2 and ix.get_stat("label_lookup_calls") == 0

    def write(vecs, metas):
        calls, before = ix.get_stat("label_lookup_calls"), len(model)
        kept = [(r, model[r][1]["id"]) for r in range(before)]
        known = any(m["id"] in {i for _, i in kept} for m in metas)  # (no row ever left: the dictionary holds the table's ids)
        got = db.batch_upsert("t", "id", vecs, metas)
        assert got == _upsert(model, "id", vecs, metas)
        assert ix.get_stat("label_lookup_calls") == calls + known  # ONE lookup whatever the batch holds; none when every value is unseen
        assert all(model[r][1]["id"] == i for r, i in kept)   # updated rows keep their row ids; new rows come behind, in batch order
        return got

    # all new -- and the first use of the key: `id` gets its column
    vecs = rng.standard_normal((40, DIM)).astype(np.float32)
    assert write(vecs, [dict(_meta(i, "n"), note="fresh") for i in range(40)]) == (0, 40)
    assert ix.get_stat("label_columns") == 3 and db._t("t").codec.column_of("id") is not None
    _check(db, model, q, asked=["n0", "n39"])
    # all present: new vectors, the metadata dict REPLACED (note goes, tenant moves, a new key comes)
    vecs = rng.standard_normal((30, DIM)).astype(np.float32)
    assert write(vecs, [{"id": f"n{i}", "tenant": "t3", "lang": "en"} for i in range(30)]) == (30, 0)
    assert all("note" not in d and "year" not in d for _, d in model[N:N + 30]) and all(d["note"] == "fresh" for _, d in model[N + 30:])
    _check(db, model, q, asked=["n5"])
    # mixed, 200 ids in one batch, shuffled: half present, half new
    ids = [str(i) for i in range(0, 200, 2)] + [f"m{i}" for i in range(100)]
    order = rng.permutation(200)
    vecs = rng.standard_normal((200, DIM)).astype(np.float32)
    assert write(vecs, [{"id": ids[j], "tenant": f"t{j % 5}", "year": "2021"} for j in order]) == (100, 100)
    _check(db, model, q, asked=["m7", "8"])
    # an id named twice, once among the present and once among the new: the LAST entry wins, the earlier ones are dropped
    vecs = rng.standard_normal((6, DIM)).astype(np.float32)
    metas = [{"id": "3", "v": "a"}, {"id": "z1", "v": "b"}, {"id": "3", "v": "c"}, {"id": "z2", "v": "d"}, {"id": "z1", "v": "e"}, {"id": "3", "v": "f"}]
    assert write(vecs, metas) == (1, 2)
    assert model[3][1] == {"id": "3", "v": "f"} and np.array_equal(model[3][0], vecs[5])
    assert [d for _, d in model[-2:]] == [{"id": "z2", "v": "d"}, {"id": "z1", "v": "e"}]
    _check(db, model, q, asked=["3", "z1", "z2"])
    # one entry; an empty batch changes nothing and looks nothing up
    assert db.upsert("t", "id", vecs[0], {"id": "solo", "tenant": "t3"}) == (0, 1) == _upsert(model, "id", vecs[:1], [{"id": "solo", "tenant": "t3"}])
    assert db.count("t", {"tenant": "t3"}) > 0
    calls, cached = ix.get_stat("label_lookup_calls"), set(db._t("t").masks)
    assert db.batch_upsert("t", "id", [], []) == (0, 0)
    assert ix.get_stat("label_lookup_calls") == calls and set(db._t("t").masks) == cached and cached
    _check(db, model, q, asked=["solo"])
    # the length and dimension checks are batch_add's
    with pytest.raises(RuntimeError, match="Dimension mismatch"):
        db.batch_upsert("t", "id", np.zeros((2, DIM + 1), np.float32), [{"id": "a"}, {"id": "b"}])
    with pytest.raises(RuntimeError, match="differ in length"):
        db.batch_upsert("t", "id", np.zeros((2, DIM), np.float32), [{"id": "a"}])
    _check(db, model, q)


def test_mask_cache_rule(vdb):
    rng, db, model = _table(vdb)
    ix = db._t("t").index
    t = db._t("t")
    q = rng.standard_normal(DIM).astype(np.float32)
    db.upsert("t", "id", model[0][0], dict(model[0][1]))  # (the id column; nothing differs, so nothing is dropped below)
    key = lambda f: frozenset(f.items())  # noqa: E731
    filters = [{"tenant": "t3"}, {"year": "2021"}, {}, {"tenant": "t1", "year": "2022"}]
    for f in filters:
        db.count("t", f)
    assert set(t.masks) == {key(f) for f in filters}
    # updates that change only `year`: the masks that name year go, the others stay -- and are used without being rebuilt
    vecs = rng.standard_normal((20, DIM)).astype(np.float32)
    metas = [dict(model[i][1], year="1999") for i in range(20)]
    assert db.batch_upsert("t", "id", vecs, metas) == _upsert(model, "id", vecs, metas) == (20, 0)
    assert set(t.masks) == {key({"tenant": "t3"}), key({})}
    built = _masks_built(db)
    assert db.count("t", {"tenant": "t3"}) == sum(1 for _, d in model if d["tenant"] == "t3") and _masks_built(db) == built
    assert db.count("t", {"year": "2021"}) == sum(1 for _, d in model if d["year"] == "2021") and _masks_built(db) == built + 1
    # an update that changes no value: every mask stays; a key that goes away counts as changed
    cached = set(t.masks)
    assert db.batch_upsert("t", "id", vecs[:3], [dict(model[i][1]) for i in range(3)]) == (3, 0)
    _upsert(model, "id", vecs[:3], [dict(model[i][1]) for i in range(3)])
    assert set(t.masks) == cached
    gone = {k: v for k, v in model[5][1].items() if k != "tenant"}
    assert db.upsert("t", "id", vecs[5], gone) == _upsert(model, "id", vecs[5:6], [gone]) == (1, 0)
    assert set(t.masks) == {key({}), key({"year": "2021"})}
    # a row added: every mask goes (they are sized for the old table)
    assert db.upsert("t", "id", vecs[6], {"id": "new", "tenant": "t3"}) == _upsert(model, "id", vecs[6:7], [{"id": "new", "tenant": "t3"}]) == (0, 1)
    assert set(t.masks) == set()
    _check(db, model, q, asked=["new"], filters=({"tenant": "t3"}, {"year": "1999"}))
    assert ix.get_stat("label_columns") == 3


def test_refusals_change_nothing(vdb):
    meta = [_meta(i) for i in range(N)]
    meta[77]["id"] = "5"  # two rows carry id 5
    rng, db, model = _table(vdb, meta=meta)
    t = db._t("t")
    ix = t.index
    q = rng.standard_normal(DIM).astype(np.float32)
    db.count("t", {"id": "0"})  # (the id column: a refused upsert below makes none)
    db.count("t", {"tenant": "t3"})
    stats = ("update_calls", "update_rows", "labels_scatter_calls", "labels_scatter_rows", "label_columns") + MASK_STATS
    before, cached = [ix.get_stat(s) for s in stats], set(t.masks)
    vecs = rng.standard_normal((4, DIM)).astype(np.float32)
    with pytest.raises(ValueError, match="'5'.*not unique"):
        db.batch_upsert("t", "id", vecs, [{"id": "1", "tenant": "x"}, {"id": "brand-new"}, {"id": "5"}, {"id": "2"}])
    with pytest.raises(ValueError, match="entry 1"):
        db.batch_upsert("t", "id", vecs[:2], [{"id": "1"}, {"tenant": "t1"}])  # a dict without the key
    with pytest.raises(ValueError, match="entry 0"):
        db.batch_upsert("t", "id", vecs[:1], [{"id": 17}])  # a value that is no str
    assert [ix.get_stat(s) for s in stats] == before and set(t.masks) == cached
    assert "brand-new" not in t.codec.codes[t.codec.column_of("id")]  # a lookup does not grow the dictionary
    _check(db, model, q, filters=({"tenant": "t3"},))
    assert db.get_by("t", "id", ["5", "6"]) == [[(model[5][1],), (model[77][1],)], [(model[6][1],)]]  # (several rows: through the masks)


def test_host_routes(vdb):
    # a 17th key: sixteen keys take the sixteen columns first
    meta = [dict(_meta(i), **{f"k{j}": str(i % (j + 2)) for j in range(14)}) for i in range(N)]
    rng, db, model = _table(vdb, meta=meta)
    ix = db._t("t").index
    q = rng.standard_normal(DIM).astype(np.float32)
    for f in ["tenant", "year"] + [f"k{j}" for j in range(14)]:
        db.count_by("t", f)
    assert ix.get_stat("label_columns") == 16
    vecs = rng.standard_normal((60, DIM)).astype(np.float32)
    metas = [dict(_meta(i), k0="0") for i in range(0, 60, 2)] + [dict(_meta(i, "h"), k3="1") for i in range(30)]
    assert db.batch_upsert("t", "id", vecs, metas) == _upsert(model, "id", vecs, metas) == (30, 30)
    assert db._t("t").codec.column_of("id") is None and ix.get_stat("label_columns") == 16 and ix.get_stat("label_lookup_calls") == 0
    _check(db, model, q, asked=["h3", "4"])
    # a column whose dictionary holds the stand-in for unhashable values
    meta = [_meta(i) for i in range(N)]
    meta[10]["id"] = ["a", "list"]
    meta[11]["id"] = ["another"]
    rng, db, model = _table(vdb, meta=meta)
    ix = db._t("t").index
    db.count("t", {"id": "0"})
    assert db._t("t").codec.column_of("id") is not None and db._t("t").codec.value_codes("id") is None
    vecs = rng.standard_normal((50, DIM)).astype(np.float32)
    metas = [dict(_meta(i), year="1999") for i in range(5, 30)] + [_meta(i, "u") for i in range(25)]
    assert db.batch_upsert("t", "id", vecs, metas) == _upsert(model, "id", vecs, metas) == (23, 27)  # (rows 10 and 11 carry no str: "10", "11" are new)
    assert ix.get_stat("label_lookup_calls") == 0
    _check(db, model, q, asked=["u3", "10", "12"])
    with pytest.raises(ValueError, match="not unique"):
        db.batch_upsert("t", "tenant", vecs[:1], [{"tenant": "t1"}])  # (a column without the stand-in: the device route refuses alike)


def test_batch_update_finds_the_same_rows_either_way(vdb, monkeypatch):
    import lab_1806_vec_db_amd.vecdb as V

    assert V.LOOKUP_MIN is None or V.LOOKUP_MIN >= 64
    meta = [_meta(i) for i in range(N)]
    for i in (201, 202, 203):
        meta[i]["id"] = str(i - 200)  # ids 1, 2, 3 are carried by two rows each
    pats = [{"id": str(i)} for i in range(95)] + [{"id": "nobody"}, {"id": "no one"}] + [{"id": str(i)} for i in (250, 251, 252)]
    answers = []
    for lookup_min in (1, None):
        monkeypatch.setattr(V, "LOOKUP_MIN", lookup_min)
        rng, db, model = _table(vdb, meta=meta)
        ix = db._t("t").index
        db.count("t", {"id": "299"})  # (batch_update gives no key a column; this pattern is none of the batch's, whose masks are all uncached)
        vecs = rng.standard_normal((100, DIM)).astype(np.float32)
        calls, built = ix.get_stat("label_lookup_calls"), _masks_built(db)
        got = db.batch_update("t", pats, vecs)
        if lookup_min is None:
            assert ix.get_stat("label_lookup_calls") == calls and _masks_built(db) == built + 100
        else:  # ONE lookup; the masks of the three ids with two rows, and of the two values the dictionary has never seen
            assert ix.get_stat("label_lookup_calls") == calls + 1 and ix.get_stat("label_lookup_codes") == 98
            assert ix.get_stat("mask_where_masks") == built + 5 == _masks_built(db)
        want = [sum(1 for m in meta if m["id"] == p["id"]) for p in pats]
        assert got == want and got[0] == 1 and got[1] == 2 and got[95] == 0
        answers.append((got, db.extract_data("t")))
        for i, p in enumerate(pats):
            for r, m in enumerate(meta):
                if m["id"] == p["id"]:
                    assert np.array_equal(np.array(answers[-1][1][r][0], dtype=np.float32), vecs[i]), (lookup_min, i, r)
    assert answers[0] == answers[1]


def test_hnsw_and_pq(vdb):
    rng, db, model = _table(vdb)
    vecs = rng.standard_normal((10, DIM)).astype(np.float32)
    db.build_hnsw_index("t")
    db.build_pq_table("t", m=4)
    assert db.has_hnsw_index("t") and db.has_pq_table("t")
    metas = [_meta(i, "p") for i in range(10)]
    assert db.batch_upsert("t", "id", vecs, metas) == _upsert(model, "id", vecs, metas) == (0, 10)  # only added: as batch_add
    assert db.has_hnsw_index("t") and not db.has_pq_table("t")
    db.build_pq_table("t", m=4)
    metas = [dict(_meta(i), year="1999") for i in range(3)] + [_meta(0, "q")]
    assert db.batch_upsert("t", "id", vecs[:4], metas) == _upsert(model, "id", vecs[:4], metas) == (3, 1)  # a row updated: as batch_update
    assert not db.has_hnsw_index("t") and not db.has_pq_table("t")
    _check(db, model, rng.standard_normal(DIM).astype(np.float32), asked=["p3", "q0"])
