"""GPU: VecDB.search_fused / batch_search_fused(group_by=): several searches of one question joined into a ranking of DOCUMENTS, the rows
that share a value of a metadata key.  The expected answer comes from a test-local model of the table -- metadata dicts plus the vectors
in row order, changed by the test alongside every batch_add, delete, update and update_metadata --, the CPU oracle's full order of every
vector of a question over the rows a Python predicate lets through, cut at fetch_k, and tests/fuse_groups_ref.py over the metadata
values; then upper_bound.  Tags, scores and `exact` are compared exactly.  (The vectors are random: no two distances tie.)"""
import numpy as np
import pytest

import fuse_groups_ref as R

pytestmark = pytest.mark.gpu

DIM = 16
MODES = ("rrf", "min", "sum")


def _meta(i):
    m = {"id": str(i), "tenant": "t%d" % (i % 4), "year": str(2000 + i % 30)}
    if i % 9:
        m["doc"] = "d%d" % ((i * 7) % 50) if i % 10 else "big"
    return m


class Model:
    """the table as the test knows it: metadata dicts and vectors in the table's row order"""

    def __init__(self, dist="l2sqr", n=600, seed=82, meta=_meta):
        from lab_1806_vec_db_amd.vecdb import VecDB

        self.rng = np.random.default_rng(seed)
        self.kind = 0 if dist == "l2sqr" else 1
        self.db = VecDB()
        self.db.create_table_if_not_exists("t", DIM, dist)
        self.meta, self.vecs = [], np.zeros((0, DIM), dtype=np.float32)
        self.add([meta(i) for i in range(n)])

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

    def expect(self, queries, k, fusion="rrf", key="doc", weights=None, preds=None, fetch_k=None, c=60.0, ub=None):
        """preds: None, one predicate for every vector, or one (or None) per vector.  -> ([(tag, score)], exact)"""
        from oracle import oracle as O

        queries = np.asarray(queries, dtype=np.float32).reshape(-1, DIM)
        fk = min(max(4 * k if fetch_k is None else fetch_k, k), 4096)
        if preds is None or callable(preds):
            preds = [preds] * len(queries)
        lists, longest = [], 0
        for q, pred in zip(queries, preds):
            allowed = [i for i, m in enumerate(self.meta) if pred is None or pred(m)]
            longest = max(longest, len(allowed))
            if not allowed:
                lists.append(([], []))
                continue
            oi, od = O.flat_knn(self.vecs[allowed], q, len(allowed), self.kind)
            lists.append(([allowed[int(j)] for j in oi[:fk]], od[:fk]))

        def group_of(i):
            v = self.meta[int(i)].get(key)
            return ("r", int(i)) if v is None else ("l", repr(v))

        return lists, group_of, fk, longest

    def answer(self, queries, k, fusion="rrf", key="doc", weights=None, preds=None, fetch_k=None, c=60.0, ub=None, longest=None):
        lists, group_of, fk, lg = self.expect(queries, k, fusion, key, weights, preds, fetch_k, c, ub)
        lg = lg if longest is None else longest
        ids, sc, ex = R.fuse_groups(lists, group_of, k, fusion, weights, c, trunc_len=None if fk >= lg else fk)
        return [(self.meta[int(i)]["id"], float(s)) for i, s in zip(ids, sc) if ub is None or np.float32(s) <= np.float32(ub)], bool(ex)


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


def _batch_longest(md, groups, preds_per_q):
    """the longest allowed set over ALL vectors of a batch: what decides whether fetch_k reaches it (one library call per batch)"""
    longest = 0
    for g, p in zip(groups, preds_per_q):
        ps = [p] * len(g) if p is None or callable(p) else p
        for pred in ps:
            longest = max(longest, sum(1 for m in md.meta if pred is None or pred(m)))
    return longest


@pytest.mark.parametrize("dist", ("l2sqr", "cosine"))
def test_search_fused_by_document(dist):
    from lab_1806_vec_db_amd.labels import AnyOf, Ge

    md = Model(dist)
    db, ix = md.db, md.db._t("t").index
    groups = _questions(md, np.random.default_rng(3))
    for fusion in MODES:
        for k, fetch_k in ((1, None), (10, None), (10, 10), (7, 65), (5, 3000)):
            s0 = ix.get_stat("flat_fused_groups_calls")
            got, exact = db.batch_search_fused("t", groups, k, fusion, fetch_k=fetch_k, group_by="doc", return_exact=True)
            assert ix.get_stat("flat_fused_groups_calls") == s0 + 1  # the whole ragged batch: ONE call
            exp = [md.answer(g, k, fusion, fetch_k=fetch_k) for g in groups]
            assert [_tags(r) for r in got] == [e[0] for e in exp], (fusion, k, fetch_k)
            assert exact == [e[1] for e in exp], (fusion, k, fetch_k)
            docs = [[m.get("doc", m["id"]) for m, _ in r] for r in got]
            assert all(len(set(d)) == len(d) for d in docs)  # a document at most once
        assert all(db.batch_search_fused("t", groups, 5, fusion, fetch_k=3000, group_by="doc", return_exact=True)[1])  # every list whole
        for g in groups[:2]:
            assert _tags(db.search_fused("t", list(g), 10, fusion, group_by="doc")) == md.answer(g, 10, fusion)[0]
            got, ex = db.search_fused("t", list(g), 10, fusion, group_by="doc", return_exact=True)
            assert (_tags(got), ex) == md.answer(g, 10, fusion)
    assert ix.get_stat("flat_fused_calls") == 0  # never the row-level call
    # the default return shape is the row-level one; the row-level call is untouched by the new keywords
    assert isinstance(db.batch_search_fused("t", groups, 5, group_by="doc"), list)
    assert [_tags(r) for r in db.batch_search_fused("t", groups, 5)] != [_tags(r) for r in db.batch_search_fused("t", groups, 5, group_by="doc")]
    # weights: "rrf" only
    w = [[1.0, 0.25, 4.0], None, [0.001, 1000.0, 1.0, 2.0, 3.0], [2.0, 2.0], None]
    got = db.batch_search_fused("t", groups, 10, "rrf", weights=w, rrf_c=1.0, group_by="doc")
    assert [_tags(r) for r in got] == [md.answer(g, 10, "rrf", weights=x, c=1.0)[0] for g, x in zip(groups, w)]
    # another key, and one no row has: every row a document of its own -- the row-level answer, bit for bit
    got = db.batch_search_fused("t", groups, 10, "sum", group_by="tenant")
    assert [_tags(r) for r in got] == [md.answer(g, 10, "sum", key="tenant")[0] for g in groups] and all(len(r) == 4 for r in got)
    for fusion in ("rrf", "min"):
        assert [_tags(r) for r in db.batch_search_fused("t", groups, 10, fusion, group_by="nokey")] == \
            [_tags(r) for r in db.batch_search_fused("t", groups, 10, fusion)]
    # filters of all three kinds: a pattern, a pattern with a predicate, an expression -- one for the batch, per question, per vector
    f_pat, p_pat = {"tenant": "t1"}, (lambda m: m["tenant"] == "t1")
    f_prd, p_prd = {"year": Ge("2020")}, (lambda m: m["year"] >= "2020")
    f_exp, p_exp = AnyOf({"doc": "big"}, {"tenant": "t2"}), (lambda m: m.get("doc") == "big" or m["tenant"] == "t2")
    for fusion in MODES:
        for f, p in ((f_pat, p_pat), (f_prd, p_prd), (f_exp, p_exp)):
            got, exact = db.batch_search_fused("t", groups, 8, fusion, filters=f, group_by="doc", return_exact=True)
            exp = [md.answer(g, 8, fusion, preds=p) for g in groups]
            assert [_tags(r) for r in got] == [e[0] for e in exp] and exact == [e[1] for e in exp], fusion
            assert all(p(m) for r in got for m, _ in r)
        per_q = [f_pat, None, f_exp, [f_prd, f_pat], [None, f_exp, f_pat, {"tenant": "nobody"}]]
        per_p = [p_pat, None, p_exp, [p_prd, p_pat], [None, p_exp, p_pat, lambda m: False]]
        got, exact = db.batch_search_fused("t", groups, 8, fusion, filters=per_q, group_by="doc", return_exact=True)
        lg = _batch_longest(md, groups, per_p)
        exp = [md.answer(g, 8, fusion, preds=p, longest=lg) for g, p in zip(groups, per_p)]
        assert [_tags(r) for r in got] == [e[0] for e in exp] and exact == [e[1] for e in exp], fusion
    assert db.search_fused("t", groups[0], 5, filters={"tenant": "nobody"}, group_by="doc") == []
    # upper_bound: "min" only
    full = md.answer(groups[0], 10, "min")[0]
    ub = sorted(d for _, d in full)[4]
    got = db.search_fused("t", groups[0], 10, "min", upper_bound=ub, group_by="doc")
    assert _tags(got) == [e for e in full if e[1] <= ub] and len(got) == 5
    # with_vectors: the representative's vector
    got = db.batch_search_fused("t", groups, 5, "sum", with_vectors=True, group_by="doc")
    assert [[(m["id"], s) for m, s, _ in r] for r in got] == [md.answer(g, 5, "sum")[0] for g in groups]
    by_tag = {m["id"]: i for i, m in enumerate(md.meta)}
    assert all(np.array_equal(v, md.vecs[by_tag[m["id"]]]) for r in got for m, _, v in r)
    # the argument errors
    for fusion in ("rrf", "sum"):
        with pytest.raises(ValueError, match="upper_bound"):
            db.search_fused("t", groups[0], 10, fusion, upper_bound=1.0, group_by="doc")
    with pytest.raises(ValueError, match="fusion"):
        db.search_fused("t", groups[0], 10, "sum")  # "sum" ranks documents
    with pytest.raises(ValueError, match="fusion"):
        db.search_fused("t", groups[0], 10, "max", group_by="doc")
    with pytest.raises(ValueError, match="return_exact"):
        db.search_fused("t", groups[0], 10, return_exact=True)
    for fusion in ("min", "sum"):
        with pytest.raises(ValueError, match="weights"):
            db.search_fused("t", groups[0], 10, fusion, weights=[1.0, 1.0, 1.0], group_by="doc")
    with pytest.raises(RuntimeError, match="weights"):
        db.batch_search_fused("t", groups, 5, weights=[[1.0]] * 5, group_by="doc")
    with pytest.raises(RuntimeError, match="filters"):
        db.batch_search_fused("t", groups, 5, filters=[None, None], group_by="doc")
    assert db.batch_search_fused("t", [], 5, group_by="doc") == [] and db.batch_search_fused("t", [], 5, group_by="doc", return_exact=True) == ([], [])


def test_answers_follow_the_table_after_every_kind_of_write():
    md = Model(n=500)
    db = md.db
    rng = np.random.default_rng(4)
    groups = _questions(md, rng)
    filt, pred = {"tenant": "t3"}, (lambda m: m["tenant"] == "t3")

    def check(what):
        for fusion in MODES:
            got = db.batch_search_fused("t", groups, 8, fusion, group_by="doc")
            assert [_tags(r) for r in got] == [md.answer(g, 8, fusion)[0] for g in groups], (what, fusion)
            assert _tags(db.search_fused("t", groups[0], 8, fusion, filters=[filt, None, {"doc": "d7"}], group_by="doc")) == \
                md.answer(groups[0], 8, fusion, preds=[pred, None, lambda m: m.get("doc") == "d7"])[0], (what, fusion)

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
    assert db.update_metadata("t", {"doc": "d14"}, {"doc": "d7", "tenant": "t3"}) > 0  # the group key itself changes
    for m in md.meta:
        if m.get("doc") == "d14":
            m["doc"], m["tenant"] = "d7", "t3"
    check("after update_metadata")


def test_the_17th_key_and_unhashable_values_take_the_host_fallback():
    meta = lambda i: {"id": str(i), **{f"k{j}": str((i * (j + 1)) % 5) for j in range(16)}, **({"doc": "d%d" % (i % 60)} if i % 9 else {})}  # noqa: E731
    a, b = Model(n=500, meta=meta), Model(n=500, meta=meta)  # the same table twice
    rng = np.random.default_rng(5)
    groups = _questions(a, rng)
    for j in range(16):
        assert a.db.count("t", {f"k{j}": "1"}) >= 0  # sixteen keys take the sixteen columns of table a
    ia, ib = a.db._t("t").index, b.db._t("t").index
    assert ia.get_stat("label_columns") == 16
    f, p = {"k0": "1"}, (lambda m: m["k0"] == "1")
    for fusion in MODES:
        for k, fetch_k in ((1, None), (10, None), (10, 10), (0, 5), (5, 3000)):
            for filters, preds in ((None, None), (f, p)):
                host = a.db.batch_search_fused("t", groups, k, fusion, filters=filters, fetch_k=fetch_k, group_by="doc", return_exact=True)
                dev = b.db.batch_search_fused("t", groups, k, fusion, filters=filters, fetch_k=fetch_k, group_by="doc", return_exact=True)
                assert ([_tags(r) for r in host[0]], host[1]) == ([_tags(r) for r in dev[0]], dev[1]), (fusion, k, fetch_k)  # as a column would answer
                exp = [a.answer(g, k, fusion, fetch_k=fetch_k, preds=preds) for g in groups]
                assert [_tags(r) for r in host[0]] == [e[0] for e in exp] and host[1] == [e[1] for e in exp], (fusion, k, fetch_k)
    w = [[1.0, 0.25, 4.0], None, None, [2.0, 0.5], None]
    assert [_tags(r) for r in a.db.batch_search_fused("t", groups, 10, weights=w, group_by="doc")] == \
        [_tags(r) for r in b.db.batch_search_fused("t", groups, 10, weights=w, group_by="doc")]
    got = a.db.search_fused("t", groups[0], 6, "sum", group_by="doc", with_vectors=True)
    assert [(m["id"], s) for m, s, _ in got] == a.answer(groups[0], 6, "sum")[0]
    assert ia.get_stat("flat_fused_groups_calls") == 0 and ib.get_stat("flat_fused_groups_calls") > 0
    # values a dictionary cannot keep apart (unhashable): told apart by equality on the host
    c = Model(n=300, meta=lambda i: {"id": str(i), "tags": [i % 3, "x"] if i % 4 else ["y"]})
    g = _questions(c, rng)[0]
    for fusion in MODES:
        got, ex = c.db.search_fused("t", g, 12, fusion, group_by="tags", return_exact=True)
        assert (_tags(got), ex) == c.answer(g, 12, fusion, key="tags") and len(got) <= 4
    assert c.db._t("t").index.get_stat("flat_fused_groups_calls") == 0
