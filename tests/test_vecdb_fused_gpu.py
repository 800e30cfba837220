"""GPU: VecDB.search_fused / batch_search_fused (several searches of one question joined by reciprocal rank fusion or by the smallest
distance).  The expected answer comes from a test-local model of the table -- a list of metadata dicts plus a numpy array of the vectors
in row order, changed by the test alongside every batch_add, delete, update and update_metadata -- the CPU oracle's full order of every
vector of a question over the rows a Python predicate lets through, cut at fetch_k, and tests/fuse_ref.py; then upper_bound.  Tags and
scores are compared exactly.  (The vectors are random: no two distances tie, so the table's row order plays no part in a list; RRF
scores do tie, and the tie order is the table's row order, which is why the model keeps the rows in it.)"""
import numpy as np
import pytest

import fuse_ref as R

pytestmark = pytest.mark.gpu

DIM = 16


def _meta(i):
    m = {"id": str(i), "tenant": "t%d" % (i % 4), "year": str(2000 + i % 30)}
    if i % 9:
        m["doc"] = "d%d" % ((i * 7) % 50) if i % 10 else "big"
    return m


class Model:
    """the table as the test knows it: metadata dicts and vectors in the table's row order"""

    def __init__(self, dist="l2sqr", n=600, seed=81):
        from lab_1806_vec_db_amd.vecdb import VecDB

        self.rng = np.random.default_rng(seed)
        self.kind = 0 if dist == "l2sqr" else 1
        self.db = VecDB()
        self.db.create_table_if_not_exists("t", DIM, dist)
        self.meta, self.vecs = [], np.zeros((0, DIM), dtype=np.float32)
        self.add([_meta(i) for i in range(n)])

    def add(self, metas):
        centres = np.random.default_rng(7).random((40, DIM)).astype(np.float32)
        vecs = (centres[self.rng.integers(0, 40, len(metas))] + self.rng.standard_normal((len(metas), DIM)).astype(np.float32) * np.float32(0.05)).astype(np.float32)
        self.db.batch_add("t", vecs, metas)
        self.meta += [dict(m) for m in metas]
        self.vecs = np.concatenate([self.vecs, vecs])

    def sync_rows(self):
        """after a delete: the table's row order is whatever the removal left -- read it back and check it holds the rows the model kept"""
        vecs, metas = self.db.get("t")
        by_tag = {m["id"]: i for i, m in enumerate(self.meta)}
        assert sorted(m["id"] for m in metas) == sorted(by_tag)
        order = [by_tag[m["id"]] for m in metas]
        self.meta = [self.meta[i] for i in order]
        self.vecs = self.vecs[order]
        assert np.array_equal(vecs, self.vecs) and metas == self.meta

    def expect(self, queries, k, fusion="rrf", weights=None, preds=None, fetch_k=None, c=60.0, ub=None):
        """preds: None, one predicate for every vector, or one (or None) per vector"""
        from oracle import oracle as O

        queries = np.asarray(queries, dtype=np.float32).reshape(-1, DIM)
        fk = min(max(4 * k if fetch_k is None else fetch_k, k), 4096)
        if preds is None or callable(preds):
            preds = [preds] * len(queries)
        lists = []
        for q, pred in zip(queries, preds):
            allowed = [i for i, m in enumerate(self.meta) if pred is None or pred(m)]
            if not allowed:
                lists.append(([], []))
                continue
            oi, od = O.flat_knn(self.vecs[allowed], q, len(allowed), self.kind)
            lists.append(([allowed[int(j)] for j in oi[:fk]], od[:fk]))
        ids, sc = R.fuse(lists, k, fusion, weights, c)
        return [(self.meta[int(i)]["id"], float(s)) for i, s in zip(ids, sc) if ub is None or np.float32(s) <= np.float32(ub)]


def _tags(res):
    return [(e[0]["id"], e[1]) for e in res]


def _questions(md, rng):
    """ragged groups: 1 to 5 vectors near stored rows, some of them repeated inside a group"""
    groups = []
    for s in (3, 1, 5, 2, 4):
        rows = rng.integers(0, len(md.vecs), size=s)
        g = (md.vecs[rows] + rng.standard_normal((s, DIM)).astype(np.float32) * np.float32(0.02)).astype(np.float32)
        groups.append(g)
    groups[2][3] = groups[2][0]
    return groups


@pytest.mark.parametrize("dist", ("l2sqr", "cosine"))
def test_search_fused_and_batch_search_fused(dist):
    from lab_1806_vec_db_amd.labels import AnyOf, Ge

    md = Model(dist)
    db, ix = md.db, md.db._t("t").index
    groups = _questions(md, np.random.default_rng(3))
    for fusion in ("rrf", "min"):
        for k, fetch_k in ((1, None), (10, None), (10, 10), (7, 65)):
            s0 = ix.get_stat("flat_fused_calls")
            got = db.batch_search_fused("t", groups, k, fusion, fetch_k=fetch_k)
            assert ix.get_stat("flat_fused_calls") == s0 + 1  # the whole ragged batch: ONE call
            exp = [md.expect(g, k, fusion, fetch_k=fetch_k) for g in groups]
            assert [_tags(r) for r in got] == exp, (fusion, k, fetch_k)
        for g in groups[:2]:
            assert _tags(db.search_fused("t", list(g), 10, fusion)) == md.expect(g, 10, fusion)
    # one vector: the plain search's rows in its order; under "min" its entries exactly
    plain = db.search("t", groups[1][0], 10)
    assert _tags(db.search_fused("t", groups[1], 10, "min")) == _tags(plain)
    assert [t for t, _ in _tags(db.search_fused("t", groups[1], 10, "rrf"))] == [t for t, _ in _tags(plain)]
    # weights: per question None or one per vector; rrf_c
    w = [[1.0, 0.25, 4.0], None, [0.001, 1000.0, 1.0, 2.0, 3.0], [2.0, 2.0], None]
    got = db.batch_search_fused("t", groups, 10, "rrf", weights=w, rrf_c=1.0)
    assert [_tags(r) for r in got] == [md.expect(g, 10, "rrf", weights=x, c=1.0) for g, x in zip(groups, w)]
    assert _tags(db.search_fused("t", groups[0], 10, weights=w[0], rrf_c=0.0)) == md.expect(groups[0], 10, weights=w[0], c=0.0)
    assert [_tags(r) for r in db.batch_search_fused("t", groups, 10, weights=[None] * 5)] == [md.expect(g, 10) for g in groups]
    # filters of all three kinds: a pattern, a pattern with a predicate, an expression -- one for the batch, per question, per vector
    f_pat, p_pat = {"tenant": "t1"}, (lambda m: m["tenant"] == "t1")
    f_prd, p_prd = {"year": Ge("2020")}, (lambda m: m["year"] >= "2020")
    f_exp, p_exp = AnyOf({"doc": "big"}, {"tenant": "t2"}), (lambda m: m.get("doc") == "big" or m["tenant"] == "t2")
    for fusion in ("rrf", "min"):
        for f, p in ((f_pat, p_pat), (f_prd, p_prd), (f_exp, p_exp)):
            got = db.batch_search_fused("t", groups, 8, fusion, filters=f)
            assert [_tags(r) for r in got] == [md.expect(g, 8, fusion, preds=p) for g in groups], fusion
            assert all(p(m) for r in got for m, _ in r)
        per_q = [f_pat, None, f_exp, [f_prd, f_pat], [None, f_exp, f_pat, {"tenant": "nobody"}]]
        per_p = [p_pat, None, p_exp, [p_prd, p_pat], [None, p_exp, p_pat, lambda m: False]]
        s0 = ix.get_stat("flat_fused_calls")
        got = db.batch_search_fused("t", groups, 8, fusion, filters=per_q)
        assert ix.get_stat("flat_fused_calls") == s0 + 1
        assert [_tags(r) for r in got] == [md.expect(g, 8, fusion, preds=p) for g, p in zip(groups, per_p)], fusion
        # one vector under several filters: "anything" plus "only this tenant"
        one = np.repeat(groups[1], 2, axis=0)
        assert _tags(db.search_fused("t", one, 8, fusion, filters=[None, f_pat])) == md.expect(one, 8, fusion, preds=[None, p_pat])
    assert db.search_fused("t", groups[0], 5, filters={"tenant": "nobody"}) == []
    # upper_bound: "min" only
    full = md.expect(groups[0], 10, "min")
    ub = sorted(d for _, d in full)[4]
    got = db.search_fused("t", groups[0], 10, "min", upper_bound=ub)
    assert _tags(got) == [e for e in full if e[1] <= ub] and len(got) == 5
    with pytest.raises(ValueError, match="upper_bound"):
        db.search_fused("t", groups[0], 10, "rrf", upper_bound=1.0)
    with pytest.raises(ValueError, match="fusion"):
        db.search_fused("t", groups[0], 10, "sum")
    # with_vectors
    got = db.batch_search_fused("t", groups, 5, "min", with_vectors=True)
    assert [_tags(r) for r in got] == [md.expect(g, 5, "min") for g in groups]
    by_tag = {m["id"]: i for i, m in enumerate(md.meta)}
    assert all(np.array_equal(v, md.vecs[by_tag[m["id"]]]) for r in got for m, _, v in r)
    assert db.batch_search_fused("t", [], 5) == []
    with pytest.raises(RuntimeError, match="weights"):
        db.batch_search_fused("t", groups, 5, weights=[[1.0]] * 5)
    with pytest.raises(RuntimeError, match="filters"):
        db.batch_search_fused("t", groups, 5, filters=[None, None])


def test_answers_follow_the_table_after_every_kind_of_write():
    md = Model(n=500)
    db = md.db
    rng = np.random.default_rng(4)
    groups = _questions(md, rng)
    filt, pred = {"tenant": "t3"}, (lambda m: m["tenant"] == "t3")

    def check(what):
        for fusion in ("rrf", "min"):
            got = db.batch_search_fused("t", groups, 8, fusion)
            assert [_tags(r) for r in got] == [md.expect(g, 8, fusion) for g in groups], (what, fusion)
            assert _tags(db.search_fused("t", groups[0], 8, fusion, filters=[filt, None, {"doc": "d7"}])) == \
                md.expect(groups[0], 8, fusion, preds=[pred, None, lambda m: m.get("doc") == "d7"]), (what, fusion)

    check("fresh")
    md.add([{"id": "n%d" % i, "tenant": "t3", "doc": "d7" if i % 20 == 1 else "x"} for i in range(200)])
    check("after batch_add")
    assert db.delete("t", {"doc": "big"}) > 0
    keep = [i for i, m in enumerate(md.meta) if m.get("doc") != "big"]
    md.meta, md.vecs = [md.meta[i] for i in keep], md.vecs[keep]
    md.sync_rows()
    check("after delete")
    moved = [m["id"] for m in md.meta if m.get("doc") == "d7"][:5]
    vecs = (groups[0][0] + rng.standard_normal((len(moved), DIM)).astype(np.float32) * np.float32(0.01)).astype(np.float32)  # right next to a query
    assert db.batch_update("t", [{"id": t} for t in moved], list(vecs)) == [1] * len(moved)
    by_tag = {m["id"]: i for i, m in enumerate(md.meta)}
    for t, v in zip(moved, vecs):
        md.vecs[by_tag[t]] = v
    check("after update")
    assert db.update_metadata("t", {"doc": "d14"}, {"doc": "d7", "tenant": "t3"}) > 0
    for m in md.meta:
        if m.get("doc") == "d14":
            m["doc"], m["tenant"] = "d7", "t3"
    check("after update_metadata")
