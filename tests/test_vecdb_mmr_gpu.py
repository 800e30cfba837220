"""GPU: VecDB.search / batch_search with mmr_lambda and fetch_k (diversified hits: maximal marginal relevance over the fetch_k nearest
matching rows).  The expected answer of a query comes from a test-local model of the table -- a numpy copy of the vectors and the
metadata, keyed by the "id" tag and changed by the test alongside every batch_add, delete and update -- the CPU oracle's full order over
the rows a Python predicate lets through, and the reference walk of tests/mmr_ref.py; then upper_bound.  Tags, selection order and
distances are compared exactly.  (The vectors are random: no two distances tie, so the table's row order plays no part.)"""
import numpy as np
import pytest

import mmr_ref as R

pytestmark = pytest.mark.gpu

DIM = 16
MSTATS = ("flat_mmr_calls", "flat_mmr_queries")


def _meta(i):
    m = {"id": str(i), "tenant": "t%d" % (i % 4)}
    if i % 9:
        m["doc"] = "d%d" % ((i * 7) % 50) if i % 10 else "big"
    return m


class Model:
    """the table as the test knows it: id tag -> (vector, metadata)"""

    def __init__(self, dist="l2sqr", n=1200, seed=61):
        from lab_1806_vec_db_amd.vecdb import VecDB

        self.rng = np.random.default_rng(seed)
        self.kind = 0 if dist == "l2sqr" else 1
        self.db = VecDB()
        self.db.create_table_if_not_exists("t", DIM, dist)
        self.rows = {}
        self.add([_meta(i) for i in range(n)])

    def add(self, metas):
        # clusters of near-copies around 40 centres: what mmr is for
        centres = np.random.default_rng(7).random((40, DIM)).astype(np.float32)
        vecs = (centres[self.rng.integers(0, 40, len(metas))] + self.rng.standard_normal((len(metas), DIM)).astype(np.float32) * np.float32(0.01)).astype(np.float32)
        self.db.batch_add("t", vecs, metas)
        for v, m in zip(vecs, metas):
            self.rows[m["id"]] = (v, dict(m))

    def expect(self, q, k, lam, fetch_k=None, pred=None, ub=None):
        from oracle import oracle as O

        tags = [t for t, (_, m) in self.rows.items() if pred is None or pred(m)]
        if not tags or k == 0:
            return []
        base = np.stack([self.rows[t][0] for t in tags])
        oi, od = O.flat_knn(base, q, len(base), self.kind)
        fk = min(max(4 * k if fetch_k is None else fetch_k, k), 4096)
        oi, od = oi[:fk].astype(np.int64), od[:fk]
        sel = R.walk_rows(R.RowDist(base, self.kind), oi, od, k, lam)
        return [(tags[int(oi[p])], float(od[p])) for p in sel if ub is None or od[p] <= np.float32(ub)]


def _tags(res):
    return [(e[0]["id"], e[1]) for e in res]


@pytest.mark.parametrize("dist", ("l2sqr", "cosine"))
def test_search_and_batch_search_with_mmr(dist):
    from lab_1806_vec_db_amd.labels import AnyOf

    md = Model(dist)
    db, ix = md.db, md.db._t("t").index
    qs = md.rng.random((5, DIM)).astype(np.float32)
    n_diverse = 0
    for k, lam, fk in ((10, 0.5, None), (10, 0.25, 64), (5, 0.0, 20), (10, 1.0, None), (3, 0.5, 3), (8, 0.75, 100)):
        s0 = ix.get_stat("flat_mmr_calls")
        got = db.batch_search("t", qs, k, mmr_lambda=lam, fetch_k=fk)
        assert ix.get_stat("flat_mmr_calls") == s0 + 1  # the whole batch: ONE call
        exp = [md.expect(q, k, lam, fk) for q in qs]
        assert [_tags(r) for r in got] == exp, (k, lam, fk)
        assert _tags(db.search("t", qs[1], k, mmr_lambda=lam, fetch_k=fk)) == exp[1]
        plain = [_tags(r) for r in db.batch_search("t", qs, k)]
        if lam == 1.0:
            assert [_tags(r) for r in got] == plain  # lambda = 1: the plain search
        else:
            assert all(g[0] == p[0] for g, p in zip(exp, plain))  # the nearest row comes first
            n_diverse += sum(g != p for g, p in zip(exp, plain))
    assert n_diverse >= 5  # (near-copies around 40 centres: diversified answers are not the plain ones)
    # the default fetch_k is 4 k; below k it is raised to k; above 4096 it is clamped
    assert _tags(db.search("t", qs[0], 10, mmr_lambda=0.5)) == _tags(db.search("t", qs[0], 10, mmr_lambda=0.5, fetch_k=40))
    assert _tags(db.search("t", qs[0], 10, mmr_lambda=0.5)) == md.expect(qs[0], 10, 0.5, 40)
    assert _tags(db.search("t", qs[0], 10, mmr_lambda=0.5, fetch_k=2)) == _tags(db.search("t", qs[0], 10, mmr_lambda=0.5, fetch_k=10))
    assert _tags(db.search("t", qs[0], 4, mmr_lambda=0.5, fetch_k=10**6)) == md.expect(qs[0], 4, 0.5, 4096)
    # ef is ignored: the answer is exact, from the Flat rows
    assert _tags(db.search("t", qs[0], 10, ef=7, mmr_lambda=0.5)) == md.expect(qs[0], 10, 0.5)
    # filters: one pattern, one per query, an expression
    filt, pred = {"tenant": "t1"}, (lambda m: m["tenant"] == "t1")
    got = db.search("t", qs[0], 10, filter=filt, mmr_lambda=0.5)
    assert _tags(got) == md.expect(qs[0], 10, 0.5, pred=pred) and all(m["tenant"] == "t1" for m, _ in got)
    expr, epred = AnyOf({"tenant": "t0"}, {"doc": "big"}), (lambda m: m["tenant"] == "t0" or m.get("doc") == "big")
    got = db.batch_search("t", qs, 6, filters=expr, mmr_lambda=0.25, fetch_k=30)
    assert [_tags(r) for r in got] == [md.expect(q, 6, 0.25, 30, pred=epred) for q in qs]
    filters = [{"tenant": "t%d" % (i % 4)} if i % 2 else {"doc": "big", "tenant": "t2"} for i in range(len(qs))]
    preds = [(lambda m, f=f: all(m.get(a) == b for a, b in f.items())) for f in filters]
    s0 = ix.get_stat("flat_mmr_calls")
    got = db.batch_search("t", qs, 10, filters=filters, mmr_lambda=0.5)
    assert ix.get_stat("flat_mmr_calls") == s0 + 1
    assert [_tags(r) for r in got] == [md.expect(q, 10, 0.5, pred=p) for q, p in zip(qs, preds)]
    assert db.search("t", qs[0], 10, filter={"tenant": "nobody"}, mmr_lambda=0.5) == []
    # upper_bound is applied afterwards: the entries of the unbounded answer within the bound, in its order
    full = md.expect(qs[2], 10, 0.5)
    ub = sorted(d for _, d in full)[4]
    got = db.search("t", qs[2], 10, upper_bound=ub, mmr_lambda=0.5)
    assert _tags(got) == md.expect(qs[2], 10, 0.5, ub=ub) == [e for e in full if e[1] <= ub] and len(got) == 5
    got = db.batch_search("t", qs, 10, upper_bound=ub, filters=filt, mmr_lambda=0.5)
    assert [_tags(r) for r in got] == [md.expect(q, 10, 0.5, pred=pred, ub=ub) for q in qs]
    # with_vectors: entries become (metadata, distance, vector)
    got = db.batch_search("t", qs, 5, mmr_lambda=0.5, with_vectors=True)
    assert [_tags(r) for r in got] == [md.expect(q, 5, 0.5) for q in qs]
    assert all(np.array_equal(v, md.rows[m["id"]][0]) for r in got for m, _, v in r)
    m, d, v = db.search("t", qs[0], 5, mmr_lambda=0.5, with_vectors=True)[0]
    assert np.array_equal(v, md.rows[m["id"]][0])


def test_the_two_value_errors_and_none_changes_nothing():
    md = Model(n=300)
    db, ix = md.db, md.db._t("t").index
    qs = md.rng.random((3, DIM)).astype(np.float32)
    s0 = {s: ix.get_stat(s) for s in MSTATS}
    with pytest.raises(ValueError, match="group_by"):
        db.search("t", qs[0], 10, group_by="doc", mmr_lambda=0.5)
    with pytest.raises(ValueError, match="group_by"):
        db.batch_search("t", qs, 10, group_by="doc", mmr_lambda=0.5, fetch_k=40)
    with pytest.raises(ValueError, match="fetch_k"):
        db.search("t", qs[0], 10, fetch_k=40)
    with pytest.raises(ValueError, match="fetch_k"):
        db.batch_search("t", qs, 10, fetch_k=40)
    before = [_tags(r) for r in db.batch_search("t", qs, 10)], _tags(db.search("t", qs[0], 10, upper_bound=0.9))
    after = [_tags(r) for r in db.batch_search("t", qs, 10, mmr_lambda=None, fetch_k=None)], _tags(db.search("t", qs[0], 10, None, 0.9, None, None, 1, False, None, None))
    assert before == after and {s: ix.get_stat(s) for s in MSTATS} == s0


def test_mmr_follows_batch_add_delete_and_update():
    md = Model(n=500)
    db = md.db
    qs = md.rng.random((3, DIM)).astype(np.float32)

    def check(what):
        for lam, fk in ((0.5, None), (0.0, 25)):
            got = db.batch_search("t", qs, 8, mmr_lambda=lam, fetch_k=fk)
            assert [_tags(r) for r in got] == [md.expect(q, 8, lam, fk) for q in qs], (what, lam)
        got = db.search("t", qs[0], 8, filter={"tenant": "t3"}, mmr_lambda=0.5)
        assert _tags(got) == md.expect(qs[0], 8, 0.5, pred=lambda m: m["tenant"] == "t3"), what

    check("fresh")
    md.add([{"id": "n%d" % i, "tenant": "t3", "doc": "new"} for i in range(200)])
    check("after batch_add")
    assert db.delete("t", {"doc": "big"}) > 0
    md.rows = {t: vm for t, vm in md.rows.items() if vm[1].get("doc") != "big"}
    check("after delete")
    # new vectors for a tenth of the rows: near-copies of the first query, so they enter every candidate list
    moved = [t for t in md.rows if t.isdigit() and int(t) % 10 == 3]
    vecs = (qs[0] + md.rng.standard_normal((len(moved), DIM)).astype(np.float32) * np.float32(0.02)).astype(np.float32)
    assert db.batch_update("t", [{"id": t} for t in moved], list(vecs)) == [1] * len(moved)
    for t, v in zip(moved, vecs):
        md.rows[t] = (v, md.rows[t][1])
    check("after update")
    got = _tags(db.search("t", qs[0], 8, mmr_lambda=1.0))
    assert sum(t in set(moved) for t, _ in got) >= 6  # (the updated vectors are the ones found)
