"""GPU: VecDB.search(filter=...) / search_within(filter=...) -- exact search restricted to the rows a metadata pattern matches --
against a host computation over extract_data: the oracle's full (distance, index) order of the extracted rows, the pairs whose
metadata matches (as delete matches: every key present with an equal value) kept, then the first k / the cut at the bound."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

DIM = 32
LANGS = ("en", "fr", "de")


def _matches(meta, pattern):
    return all(meta.get(k) == v for k, v in pattern.items())


def _host_answer(db, key, query, pattern, kind):
    """[(row id tag, distance)] of every matching row, nearest first, from the table as extract_data shows it"""
    from oracle import oracle as O

    data = db.extract_data(key)
    rows = np.array([v for v, _ in data], dtype=np.float32).reshape(len(data), DIM)
    oi, od, _ = O.flat_knn_batch(rows, np.asarray(query, dtype=np.float32).reshape(1, -1), len(rows), kind)
    return [(data[int(i)][1]["id"], float(d)) for i, d in zip(oi[0], od[0]) if _matches(data[int(i)][1], pattern)]


def _tags(res):
    return [(m["id"], d) for m, d in res]


@pytest.fixture()
def table():
    from lab_1806_vec_db_amd.vecdb import VecDB

    rng = np.random.default_rng(11)
    rows = rng.random((400, DIM)).astype(np.float32)
    meta = [{"id": str(i), "lang": LANGS[i % 3], "kind": "a" if i % 5 else "b"} for i in range(400)]
    dbs = {}
    for dist in ("l2sqr", "cosine"):
        db = VecDB()
        db.create_table_if_not_exists("t", DIM, dist)
        db.batch_add("t", rows, meta)
        dbs[dist] = db
    yield dbs, rows, rng.random((4, DIM)).astype(np.float32)
    for db in dbs.values():
        db.delete_table("t")


@pytest.mark.parametrize("dist,kind", (("l2sqr", 0), ("cosine", 1)))
def test_search_with_filter(table, dist, kind):
    dbs, rows, qs = table
    db = dbs[dist]
    for pattern in ({"lang": "en"}, {"lang": "fr", "kind": "b"}, {}, {"lang": "xx"}, {"missing": "1"}):
        for q in qs:
            want = _host_answer(db, "t", q, pattern, kind)
            for k in (1, 10, 500):
                assert _tags(db.search("t", q, k, filter=pattern)) == want[:k], (pattern, k)
            assert _tags(db.search("t", q, 10, ef=50, filter=pattern)) == want[:10]  # ef is ignored
            if len(want) >= 6:
                ub = want[5][1]
                assert _tags(db.search("t", q, 50, upper_bound=ub, filter=pattern)) == [w for w in want if w[1] <= np.float32(ub)][:50]
                assert _tags(db.search_within("t", q, ub, filter=pattern)) == [w for w in want if w[1] <= np.float32(ub)]
                assert _tags(db.search_within("t", q, ub, limit=3, filter=pattern)) == want[:3]
    assert db.search("t", qs[0], 10, filter={"lang": "xx"}) == []
    assert db.search_within("t", qs[0], 1e9, filter={"lang": "xx"}) == []


def test_filter_none_is_unchanged(table):
    dbs, rows, qs = table
    db = dbs["l2sqr"]
    want = _host_answer(db, "t", qs[0], {}, 0)
    assert _tags(db.search("t", qs[0], 10)) == want[:10]
    assert _tags(db.search("t", qs[0], 10, filter=None)) == want[:10]
    assert _tags(db.search_within("t", qs[0], want[20][1])) == [w for w in want if w[1] <= np.float32(want[20][1])]
    assert not dbs["l2sqr"]._tables["t"].masks  # no filter, no mask


def test_mask_cache_follows_writes(table):
    dbs, rows, qs = table
    db = dbs["l2sqr"]
    t = db._tables["t"]
    q = qs[1]
    pat = {"lang": "en"}
    first = db.search("t", q, 5, filter=pat)
    assert len(t.masks) == 1
    db.search("t", q, 5, filter=dict(pat))
    assert len(t.masks) == 1  # cached per pattern
    # a row added afterwards is found ...
    db.add("t", q, {"id": "new", "lang": "en", "kind": "a"})
    assert not t.masks
    got = db.search("t", q, 5, filter=pat)
    assert got[0][0]["id"] == "new" and got[0][1] == 0.0
    assert _tags(got) == _host_answer(db, "t", q, pat, 0)[:5]
    # ... and a deleted one is not
    assert db.delete("t", {"id": "new"}) == 1
    assert not t.masks
    assert _tags(db.search("t", q, 5, filter=pat)) == _tags(first)
    gone = first[0][0]["id"]
    assert db.delete("t", {"id": gone}) == 1
    got = db.search("t", q, 5, filter=pat)
    assert gone not in [m["id"] for m, _ in got]
    assert _tags(got) == _host_answer(db, "t", q, pat, 0)[:5]
    assert _tags(db.search_within("t", q, got[-1][1], filter=pat)) == _tags(got)
