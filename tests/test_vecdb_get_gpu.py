"""GPU: VecDB.get, extract_data over one bulk fetch, and `with_vectors` on search / batch_search / search_within / batch_search_within.

300 rows x dim 8 with `tenant` and `year` metadata.  get(filter) against the rows a test-local lambda selects -- a pattern, In / Ge
predicates, an AnyOf expression, no filter; again after delete, batch_update and batch_add; `limit`; an empty match.  extract_data
against the per-row loop it replaces.  with_vectors: metadata and distances identical to the call without it, every vector the row's
vector bit for bit, exactly one fetch call per search call and none for a batch without hits."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N, DIM = 300, 8


@pytest.fixture(scope="module")
def vdb():
    import lab_1806_vec_db_amd as v
    return v


def _meta(i):
    return {"id": str(i), "tenant": f"t{i % 7}", "year": str(1995 + (i * 11) % 30)}


def _fill(vdb, vecs, meta):
    db = vdb.VecDB()
    db.create_table_if_not_exists("t", vecs.shape[1], "l2sqr")
    db.batch_add("t", vecs, meta)
    return db


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _filters():
    from lab_1806_vec_db_amd.labels import AnyOf, Ge, In

    return (
        ({"tenant": "t3"}, lambda m: m["tenant"] == "t3"),
        ({"tenant": In(["t1", "t5"]), "year": Ge(2010)}, lambda m: m["tenant"] in ("t1", "t5") and float(m["year"]) >= 2010),
        (AnyOf({"tenant": "t0", "year": Ge(2020)}, {"year": "1995"}), lambda m: (m["tenant"] == "t0" and float(m["year"]) >= 2020) or m["year"] == "1995"),
        (None, lambda m: True),
        ({"tenant": "nobody"}, lambda m: False),
    )


def _check_get(db, vecs, meta):
    ix = db._t("t").index
    for f, fn in _filters():
        rows = [i for i, m in enumerate(meta) if fn(m)]
        before = ix.get_stat("fetch_calls")
        v, md = db.get("t", f)
        assert v.dtype == np.float32 and v.shape == (len(rows), DIM), f
        assert np.array_equal(_bits(v), _bits(vecs[rows])) and md == [meta[i] for i in rows], f
        assert ix.get_stat("fetch_calls") - before == (1 if rows else 0), f  # ONE library call
        assert db.count("t", f) == len(rows)
        for limit in (0, 1, 5, len(rows), len(rows) + 3):
            v, md = db.get("t", f, limit=limit)
            want = rows[:limit]
            assert v.shape == (len(want), DIM) and np.array_equal(_bits(v), _bits(vecs[want])) and md == [meta[i] for i in want], (f, limit)


def test_get_before_and_after_writes(vdb):
    rng = np.random.default_rng(61)
    vecs = rng.standard_normal((N, DIM)).astype(np.float32)
    vecs[3, 0] = np.float32("nan")
    vecs[4, 1] = np.float32("-inf")
    vecs[10, 2] = np.float32(-0.0)
    meta = [_meta(i) for i in range(N)]
    db = _fill(vdb, vecs, meta)
    _check_get(db, vecs, meta)
    got = db.get("t", {"tenant": "t3"})[1]
    got[0]["tenant"] = "changed"  # the dicts are copies
    assert db.get("t", {"tenant": "t3"})[1][0]["tenant"] == "t3"
    with pytest.raises(ValueError):
        db.get("t", None, limit=-1)
    with pytest.raises(RuntimeError):
        db.get("nope")

    # delete: the model follows swap_remove in descending order
    assert db.delete("t", {"tenant": "t2"}) == len([m for m in meta if m["tenant"] == "t2"])
    vl, ml = list(vecs), list(meta)
    for i in sorted((i for i, m in enumerate(meta) if m["tenant"] == "t2"), reverse=True):
        vl[i], ml[i] = vl[-1], ml[-1]
        vl.pop()
        ml.pop()
    vecs, meta = np.array(vl, dtype=np.float32), ml
    _check_get(db, vecs, meta)

    new = rng.standard_normal((2, DIM)).astype(np.float32)
    cnt = db.batch_update("t", [{"tenant": "t5"}, {"id": "17"}], new)
    assert cnt == [len([m for m in meta if m["tenant"] == "t5"]), 1]
    for i, m in enumerate(meta):
        if m["tenant"] == "t5":
            vecs[i] = new[0]
        if m["id"] == "17":
            vecs[i] = new[1]
    _check_get(db, vecs, meta)

    add = rng.standard_normal((40, DIM)).astype(np.float32)
    add_meta = [_meta(1000 + i) for i in range(40)]
    db.batch_add("t", add, add_meta)
    vecs, meta = np.concatenate([vecs, add]), meta + add_meta
    _check_get(db, vecs, meta)
    db.delete_table("t")


def test_extract_data_equals_the_per_row_loop(vdb):
    rng = np.random.default_rng(62)
    vecs = rng.standard_normal((N, DIM)).astype(np.float32)
    meta = [_meta(i) for i in range(N)]
    db = _fill(vdb, vecs, meta)
    t = db._t("t")
    ix = t.index
    want = [(ix[i].tolist(), dict(t.metadata[i])) for i in range(len(ix))]  # what extract_data did before: one library call per row
    before = [ix.get_stat(s) for s in ("fetch_calls", "fetch_rows", "fetch_direct")]
    got = db.extract_data("t")
    assert got == want and [type(x) for x in got[0][0]] == [float] * DIM
    assert [ix.get_stat(s) for s in ("fetch_calls", "fetch_rows", "fetch_direct")] == [before[0] + 1, before[1] + N, before[2] + 1]
    empty = vdb.VecDB()
    empty.create_table_if_not_exists("e", DIM, "l2sqr")
    assert empty.extract_data("e") == [] and empty.get("e")[0].shape == (0, DIM) and empty.get("e")[1] == []
    db.delete_table("t")


def test_with_vectors_on_every_search(vdb):
    from lab_1806_vec_db_amd.labels import Ge

    rng = np.random.default_rng(63)
    vecs = rng.standard_normal((N, DIM)).astype(np.float32)
    meta = [_meta(i) for i in range(N)]
    db = _fill(vdb, vecs, meta)
    ix = db._t("t").index
    by_id = {m["id"]: i for i, m in enumerate(meta)}
    qs = vecs[:6] + np.float32(1e-3)
    filters = [{"tenant": f"t{j % 7}"} for j in range(6)]

    def one(call, hits_expected=True):
        """call(with_vectors) -> a flat list of entries, or a list of them per query"""
        plain = call(False)
        before = ix.get_stat("fetch_calls")
        full = call(True)
        nested = bool(plain) and isinstance(plain[0], list) or (not plain and False)
        pl = plain if nested else [plain]
        fl = full if nested else [full]
        assert len(pl) == len(fl)
        total = 0
        for a, b in zip(pl, fl):
            assert [(m, d) for m, d, _ in b] == a  # metadata and distances identical
            for m, _, v in b:
                assert v.dtype == np.float32 and np.array_equal(_bits(v), _bits(vecs[by_id[m["id"]]]))
            total += len(b)
        assert (total > 0) == hits_expected
        assert ix.get_stat("fetch_calls") - before == (1 if total else 0)  # the whole call: one fetch, none without a hit
        return total

    assert one(lambda w: db.search("t", qs[0], 5, with_vectors=w)) == 5
    assert one(lambda w: db.search("t", qs[0], 5, filter={"tenant": "t3"}, with_vectors=w)) == 5
    assert one(lambda w: db.search("t", qs[0], 5, upper_bound=0.5, with_vectors=w)) >= 1
    assert one(lambda w: db.search("t", qs[0], 6, group_by="tenant", group_size=1, with_vectors=w)) == 6
    assert one(lambda w: db.batch_search("t", qs, 4, with_vectors=w)) == 24
    assert one(lambda w: db.batch_search("t", qs, 4, filters=filters, with_vectors=w)) == 24
    assert one(lambda w: db.batch_search("t", qs, 4, filters={"year": Ge(2015)}, group_by="tenant", group_size=2, with_vectors=w)) == 24
    ub = db.search("t", qs[1], 9)[8][1]
    assert one(lambda w: db.search_within("t", qs[1], ub, with_vectors=w)) == 9
    assert one(lambda w: db.search_within("t", qs[1], ub, filter={"tenant": "t1"}, with_vectors=w)) >= 1
    assert one(lambda w: db.batch_search_within("t", qs, ub, with_vectors=w)) >= 9
    assert one(lambda w: db.batch_search_within("t", qs, ub, limit=3, filters=filters, with_vectors=w)) >= 6
    # no hits: no fetch call
    assert one(lambda w: db.batch_search("t", qs, 4, upper_bound=-1.0, with_vectors=w), hits_expected=False) == 0
    assert one(lambda w: db.batch_search("t", qs, 4, filters={"tenant": "nobody"}, with_vectors=w), hits_expected=False) == 0
    assert one(lambda w: db.batch_search_within("t", qs, -1.0, with_vectors=w), hits_expected=False) == 0
    assert one(lambda w: db.search("t", qs[0], 5, upper_bound=-1.0, with_vectors=w), hits_expected=False) == 0
    assert db.batch_search("t", qs[:0], 4, with_vectors=True) == []
    db.delete_table("t")
