"""GPU: VecDB.batch_search_within -- every row within a bound of each query of a batch, each query under a metadata pattern of its own,
in one library call.  Entry q equals what search_within(key, queries[q], upper_bound[q], limit, filter_q) returns (search_within is held
to the oracle by tests/test_vecdb_range_gpu.py and tests/test_vecdb_filtered_gpu.py) and what search(k = len(table), upper_bound) returns."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

DIM = 32
N = 1500
TENANTS = 6


def _patterns():
    from lab_1806_vec_db_amd.labels import Ge, In

    return ({"tenant": "t0"}, {"tenant": "t3", "year": "2004"}, {}, {"tenant": "zz"}, {"tenant": "t0"}, {"tenant": In(["t1", "t4"])},
            {"year": Ge(2005)}, {}, {"tenant": In(["t2", "zz"]), "year": "2001"}, {"tenant": "t5"})


def _make(dist, seed=21):
    from lab_1806_vec_db_amd.vecdb import VecDB

    rng = np.random.default_rng(seed)
    rows = rng.random((N, DIM)).astype(np.float32)
    meta = [{"id": str(i), "tenant": f"t{i % TENANTS}", "year": str(2000 + (i * 7) % 9)} for i in range(N)]
    db = VecDB()
    db.create_table_if_not_exists("t", DIM, dist)
    db.batch_add("t", rows, meta)
    return db, rng.random((len(_patterns()), DIM)).astype(np.float32), rng


def _bounds(db, qs, j=25):
    """per query the distance of its j-th nearest row of the whole table: every slice below is non-trivial and none is the whole table"""
    return np.array([db.search("t", q, j)[-1][1] for q in qs], dtype=np.float32)


def _check(db, qs, bounds, limit, filters):
    """batch_search_within against the list of search_within calls and against search(k = len, upper_bound)"""
    nq = len(qs)
    ub = np.broadcast_to(np.asarray(bounds, dtype=np.float32).reshape(-1), (nq,))
    pats = [filters] * nq if filters is None or isinstance(filters, dict) else list(filters)
    got = db.batch_search_within("t", qs, bounds, limit, filters)
    assert len(got) == nq
    n = len(db.extract_data("t"))
    for q in range(nq):
        assert got[q] == db.search_within("t", qs[q], ub[q], limit, pats[q]), (q, limit, pats[q])
        assert got[q] == db.search("t", qs[q], limit if limit is not None else n, upper_bound=ub[q], filter=pats[q]), (q, limit, pats[q])
    return got


@pytest.mark.parametrize("dist", ("l2sqr", "cosine"))
def test_batch_search_within_equals_the_searches(dist):
    from lab_1806_vec_db_amd.labels import In

    db, qs, _ = _make(dist)
    try:
        bounds = _bounds(db, qs)
        pats = list(_patterns())
        for limit in (None, 3):
            for b in (bounds, float(bounds[0])):  # one bound per query, one for all
                got = _check(db, qs, b, limit, None)  # no filters
                assert all(got), "an unfiltered slice holds at least the j rows its bound was taken from"
                _check(db, qs, b, limit, {"tenant": "t1"})  # one pattern for every query
                _check(db, qs, b, limit, {"tenant": In(["t1", "t2"])})  # an In predicate for every query
                got = _check(db, qs, b, limit, pats)  # a pattern per query: repeated, empty, unmatched and In ones among them
                assert got[3] == [] and got[2]
        # a wide bound: whole tenants
        got = _check(db, qs, 1e9, None, pats)
        assert len(got[0]) == N // TENANTS and len(got[2]) == N and len(got[5]) == 2 * (N // TENANTS)
        assert all(m["tenant"] == "t0" for m, _ in got[0]) and all(m["tenant"] in ("t1", "t4") for m, _ in got[5])
        # a pattern on a key that has no column yet
        _check(db, qs, bounds, None, [{"colour": "red"}] * len(qs))
        _check(db, qs, bounds, None, [{"colour": "red"} if q % 2 else {"tenant": "t2"} for q in range(len(qs))])
        assert db.batch_search_within("t", qs[:0], 1.0, filters=[]) == [] and db.batch_search_within("t", qs[:0], bounds[:0]) == []
        ix = db._tables["t"].index
        assert ix.get_stat("flat_range_multi_calls") > 0 and ix.get_stat("flat_range_grouped_queries") > 0
    finally:
        db.delete_table("t")


def test_batch_search_within_after_add_and_delete():
    db, qs, rng = _make("l2sqr")
    try:
        pats = list(_patterns())
        bounds = _bounds(db, qs)
        before = _check(db, qs, bounds, None, pats)
        assert db._tables["t"].masks
        more = rng.random((77, DIM)).astype(np.float32)
        db.batch_add("t", more, [{"id": f"n{i}", "tenant": f"t{i % TENANTS}", "year": "2004"} for i in range(77)])
        assert not db._tables["t"].masks  # dropped with the rows' generation
        after_add = _check(db, qs, 1e9, None, pats)  # (a stale mask would raise)
        assert len(after_add[0]) == N // TENANTS + 13 and len(after_add[2]) == N + 77
        removed = db.delete("t", {"year": "2004"})
        assert removed > 77 and not db._tables["t"].masks
        after = _check(db, qs, 1e9, None, pats)
        assert after[1] == [] and after_add[1] != []  # {"tenant": "t3", "year": "2004"}: all gone
        assert all(m["year"] != "2004" for g in after for m, _ in g)
        _check(db, qs, bounds, 4, pats)
        assert before[3] == []
    finally:
        db.delete_table("t")


def test_batch_search_within_errors():
    db, qs, _ = _make("l2sqr")
    try:
        with pytest.raises(RuntimeError, match="filters"):
            db.batch_search_within("t", qs, 1.0, filters=[{}] * (len(qs) - 1))
        with pytest.raises(RuntimeError, match="upper_bound"):
            db.batch_search_within("t", qs, np.ones(len(qs) - 1, dtype=np.float32))
        with pytest.raises(RuntimeError, match="Dimension mismatch"):
            db.batch_search_within("t", np.zeros((3, DIM + 1), dtype=np.float32), 1.0)
        with pytest.raises(RuntimeError, match="Dimension mismatch"):
            db.batch_search_within("t", np.zeros(DIM, dtype=np.float32), 1.0)
        with pytest.raises(RuntimeError, match="not found"):
            db.batch_search_within("nope", qs, 1.0)
    finally:
        db.delete_table("t")
