"""GPU: VecDB.find_duplicates / mark_duplicates / delete_duplicates against a test-local model of the table.

The model is a list of [vector, dict].  Its grouping is computed in float64 over the rows a test-local lambda selects: every row's
neighbours within the radius in (distance, row) order, cut at the limit, joined by tests/dup_ref.py's union-find.  The table is built so
that no pair of rows lies between 0.75 and 1.5 times the radius (asserted), so float64 and the library's f32 agree on every pair; a
chain's rows two apart sit at exactly twice the radius."""
import numpy as np
import pytest

import dup_ref as R

pytestmark = pytest.mark.gpu

DIM = 16
STEP = 1.0 / 16
RADIUS = 2 * STEP * STEP


@pytest.fixture(scope="module")
def vdb():
    import lab_1806_vec_db_amd as v
    return v


def _meta(i):
    return {"id": str(i), "lang": ("en", "de", "fr")[i % 3], "year": str(2000 + i % 20)}


def _vectors(n, seed):
    """n rows: random rows far apart, and planted among them stars (copies within 0.4 STEP of a seed) and chains (steps of STEP on axis 0)"""
    rng = np.random.default_rng(seed)
    x = (rng.random((n, DIM)) * 4).astype(np.float32)
    place = rng.permutation(n).tolist()
    for c in range(n // 12):
        s = place.pop()
        copies = [place.pop() for _ in range(int(rng.integers(1, 4)))]
        if c % 2:
            x[s, 0] = 0.25
            for k, r in enumerate(copies, start=1):
                x[r] = x[s]
                x[r, 0] = np.float32(0.25 + STEP * k)
        else:
            for r in copies:
                v = rng.standard_normal(DIM)
                x[r] = (x[s].astype(np.float64) + v * (0.4 * STEP / np.linalg.norm(v))).astype(np.float32)
    return rng, x


def _table(vdb, n=360, seed=31):
    rng, x = _vectors(n, seed)
    meta = [_meta(i) for i in range(n)]
    db = vdb.VecDB()
    db.create_table_if_not_exists("t", DIM, "l2sqr")
    db.batch_add("t", x, meta)
    return rng, db, [[x[i], dict(meta[i])] for i in range(n)]


def _model_groups(model, pred=None, radius=RADIUS, limit=None):
    """(groups as lists of ascending rows, ordered by representative; truncated)"""
    n = len(model)
    ok = np.array([pred is None or bool(pred(d)) for _, d in model], dtype=bool)
    x = np.array([v for v, _ in model], dtype=np.float64).reshape(n, DIM)
    d = ((x[:, None, :] - x[None, :, :]) ** 2).sum(axis=2)
    off = d[~np.eye(n, dtype=bool)]
    assert not ((off > 0.75 * radius) & (off < 1.5 * radius)).any()  # no pair near the radius: f32 and float64 agree
    src, lists = [], []
    for i in np.flatnonzero(ok).tolist():
        near = [j for j in np.lexsort((np.arange(n), d[i])).tolist() if ok[j] and d[i, j] <= radius]
        src.append(i)
        lists.append(near)
    lims, ids = R.csr(lists)
    group, stats = R.dup_ref(n, src, lims, ids, ok, limit or 0)
    groups = {}
    for i in np.flatnonzero(ok).tolist():
        groups.setdefault(int(group[i]), []).append(i)
    return [g for _, g in sorted(groups.items()) if len(g) >= 2], stats["truncated"]


def _filters(vdb):
    from lab_1806_vec_db_amd.labels import Ge, In

    return [
        (None, None),
        ({"lang": "en"}, lambda d: d.get("lang") == "en"),
        ({"year": Ge("2010")}, lambda d: d.get("year") is not None and d["year"] >= "2010"),
        ({"lang": In(["en", "fr"]), "year": "2003"}, lambda d: d.get("lang") in ("en", "fr") and d.get("year") == "2003"),
        (vdb.AnyOf({"lang": "de"}, vdb.Not({"year": "2001"})), lambda d: d.get("lang") == "de" or d.get("year") != "2001"),
        ({"lang": "nobody"}, lambda d: False),
    ]


def _check_find(vdb, db, model, limits=(None,)):
    for filt, pred in _filters(vdb):
        for limit in limits:
            want, trunc = _model_groups(model, pred, limit=limit)
            got, got_trunc = db.find_duplicates("t", RADIUS, filter=filt, limit=limit)
            assert got == [[model[r][1] for r in g] for g in want], (filt, limit)
            assert got_trunc == trunc, (filt, limit)


def test_find_duplicates_with_filters_of_each_kind_and_after_writes(vdb):
    rng, db, model = _table(vdb)
    want, _ = _model_groups(model)
    assert len(want) == 30 and any(len(g) >= 3 for g in want)
    _check_find(vdb, db, model, limits=(None, 1, 2, 3))
    # batch_add: copies of existing rows, and of each other
    new = np.array([model[7][0], model[7][0], model[200][0] + np.float32(0.004)], dtype=np.float32)
    metas = [{"id": "a", "lang": "en", "year": "2010"}, {"id": "b", "lang": "de", "year": "2011"}, {"id": "c", "lang": "en", "year": "2012"}]
    db.batch_add("t", new, metas)
    model.extend([new[i], dict(metas[i])] for i in range(3))
    _check_find(vdb, db, model)
    # delete: the rows of one language go, the last rows move into their places
    db.delete("t", {"lang": "fr"})
    keep = [e for e in model if e[1]["lang"] != "fr"]
    # (delete's net effect on the order is swap_remove in descending order: replay it)
    for r in sorted((i for i, e in enumerate(model) if e[1]["lang"] == "fr"), reverse=True):
        model[r] = model[-1]
        model.pop()
    assert sorted(e[1]["id"] for e in model) == sorted(e[1]["id"] for e in keep)
    assert [d for _, d in db.extract_data("t")] == [d for _, d in model]
    _check_find(vdb, db, model)
    # update: one row moves onto another; update_metadata: rows change sides of a filter
    db.update("t", {"id": "10"}, model[11][0])
    at = [i for i, e in enumerate(model) if e[1]["id"] == "10"][0]
    model[at][0] = model[11][0]
    db.update_metadata("t", {"year": "2004"}, {"lang": "en"})
    for e in model:
        if e[1]["year"] == "2004":
            e[1]["lang"] = "en"
    _check_find(vdb, db, model, limits=(None, 2))


def test_mark_duplicates_and_group_by(vdb):
    rng, db, model = _table(vdb, seed=32)
    ix = db._t("t").index
    field = "dup"
    # masks of filters that name the field and of others, cached before the mark
    q = (rng.random(DIM) * 4).astype(np.float32)
    db.search("t", q, 5, filter={"lang": "en"})
    db.search("t", q, 5, filter={field: "0"})
    db.search("t", q, 5, filter=vdb.AnyOf({field: "1"}, {"lang": "de"}))
    for filt, pred in _filters(vdb)[:5]:
        want, _ = _model_groups(model, pred)
        wrote = bool(want) or any(field in d for _, d in model if pred is None or pred(d))
        for _, d in model:
            if pred is None or pred(d):
                d.pop(field, None)
        for g, rows in enumerate(want):
            for r in rows:
                model[r][1][field] = str(g)
        t = db._t("t")
        db.search("t", q, 5, filter={"lang": "en"})
        db.search("t", q, 5, filter={field: "0"})
        cached = set(t.masks)
        got = db.mark_duplicates("t", RADIUS, field, filter=filt)
        assert got == (len(want), sum(len(g) for g in want)), filt
        assert [d for _, d in db.extract_data("t")] == [d for _, d in model], filt
        # the mask cache dropped exactly the filters that name the field -- when a row was written; else nothing
        from lab_1806_vec_db_amd.labels import filter_keys

        names = lambda k: field in filter_keys_of(k, filter_keys)  # noqa: E731
        assert {k for k in cached if not names(k)} <= set(t.masks), filt
        assert any(names(k) for k in cached if k in t.masks) == (not wrote), filt
        # search(group_by=field, group_size=1): one hit per duplicate group, every unique row
        dist = ((np.array([v for v, _ in model], dtype=np.float64) - q.astype(np.float64)) ** 2).sum(axis=1)
        seen, expect = set(), []
        for r in np.lexsort((np.arange(len(model)), dist)).tolist():
            v = model[r][1].get(field)
            if v is None or v not in seen:
                expect.append(r)
                if v is not None:
                    seen.add(v)
            if len(expect) == 40:
                break
        hits = db.search("t", q, 40, group_by=field, group_size=1)
        assert [m for m, _ in hits] == [model[r][1] for r in expect], filt
        # count_by over the field: the device column follows the write
        cb = db.count_by("t", field)
        have = [d[field] for _, d in model if field in d]  # (rows outside the filter keep the marks of earlier rounds)
        assert {k: v for k, v in cb.items() if k is not None} == {v: have.count(v) for v in set(have)}, filt
    assert ix.get_stat("flat_dup_calls") == 5


def filter_keys_of(cache_key, filter_keys):
    """the metadata keys a mask-cache key names: a frozenset of (key, value) items for a pattern, the expression itself otherwise"""
    return {k for k, _ in cache_key} if isinstance(cache_key, frozenset) else set(filter_keys(cache_key))


def test_delete_duplicates(vdb):
    rng, db, model = _table(vdb, seed=33)
    db.build_hnsw_index("t")
    assert db.has_hnsw_index("t")

    def replay(filt_pred, limit=None):
        want, _ = _model_groups(model, filt_pred, limit=limit)
        gone = sorted((r for g in want for r in g[1:]), reverse=True)
        for r in gone:
            model[r] = model[-1]
            model.pop()
        return len(gone)

    # under a filter first: only its groups shrink
    filt, pred = _filters(vdb)[1]
    n_gone = replay(pred)
    assert n_gone > 0
    assert db.delete_duplicates("t", RADIUS, filter=filt) == n_gone
    assert not db.has_hnsw_index("t")
    assert [d for _, d in db.extract_data("t")] == [d for _, d in model]
    got = np.array([v for v, _ in db.extract_data("t")], dtype=np.float32)
    assert np.array_equal(got, np.array([v for v, _ in model], dtype=np.float32))
    # then the whole table, and a second call at the same radius: what the model says -- not necessarily 0, because a chain's
    # representative and the rows beyond its removed middle may now be apart, or again within reach
    first = replay(None)
    assert db.delete_duplicates("t", RADIUS) == first and first > 0
    assert [d for _, d in db.extract_data("t")] == [d for _, d in model]
    second = replay(None)
    assert db.delete_duplicates("t", RADIUS) == second
    assert [d for _, d in db.extract_data("t")] == [d for _, d in model]
    _check_find(vdb, db, model)
    # nothing to remove: nothing moves
    third = replay(None)
    assert third == 0 and db.delete_duplicates("t", RADIUS) == 0 and db.get_len("t") == len(model)
