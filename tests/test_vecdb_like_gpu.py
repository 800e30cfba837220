"""GPU: VecDB.search_like / batch_search_like (search by example rows).  The expected answer of a query comes from a test-local model of
the table -- a list of metadata dicts plus a numpy array of the vectors in row order, changed by the test alongside every batch_add,
delete, update and update_metadata -- tests/like_ref.py for the query vector of the rows a Python predicate selects (ascending row
order), and the CPU oracle's full order over the rows another predicate lets through, less the examples; then upper_bound.  Tags and
distances are compared exactly.  (The vectors are random: no two distances tie, so the table's row order plays no part in the order of
the hits; it does in the fold order of the examples, which is why the model keeps the rows in the table's order.)"""
import numpy as np
import pytest

import like_ref as R

pytestmark = pytest.mark.gpu

DIM = 16


def _meta(i):
    m = {"id": str(i), "tenant": "t%d" % (i % 4), "year": str(2000 + i % 30)}
    if i % 9:
        m["doc"] = "d%d" % ((i * 7) % 50) if i % 10 else "big"
    return m


class Model:
    """the table as the test knows it: metadata dicts and vectors in the table's row order"""

    def __init__(self, dist="l2sqr", n=600, seed=71):
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
        """after a delete: the table's row order is whatever the removal left -- read it back (get returns the rows in row order) and
        check that it holds exactly the rows the model kept"""
        vecs, metas = self.db.get("t")
        by_tag = {m["id"]: i for i, m in enumerate(self.meta)}
        assert sorted(m["id"] for m in metas) == sorted(by_tag)
        order = [by_tag[m["id"]] for m in metas]
        self.meta = [self.meta[i] for i in order]
        self.vecs = self.vecs[order]
        assert np.array_equal(vecs, self.vecs) and metas == self.meta

    def expect(self, pos, k, neg=None, pred=None, ub=None, exclude=True):
        from oracle import oracle as O

        p = [i for i, m in enumerate(self.meta) if pos(m)]
        g = [i for i, m in enumerate(self.meta) if neg(m)] if neg is not None else []
        q = R.like_query(self.vecs, p, g)
        allowed = [i for i, m in enumerate(self.meta) if pred is None or pred(m)]
        if not allowed or k == 0:
            return []
        oi, od = O.flat_knn(self.vecs[allowed], q, len(allowed), self.kind)
        out = []
        for j, d in zip(oi, od):
            row = allowed[int(j)]
            if exclude and (row in p or row in g):
                continue
            if len(out) == k:
                break
            out.append((self.meta[row]["id"], float(d)))
        return [e for e in out if ub is None or np.float32(e[1]) <= np.float32(ub)]


def _tags(res):
    return [(e[0]["id"], e[1]) for e in res]


@pytest.mark.parametrize("dist", ("l2sqr", "cosine"))
def test_search_like_and_batch_search_like(dist):
    from lab_1806_vec_db_amd.labels import AnyOf, Ge, In

    md = Model(dist)
    db, ix = md.db, md.db._t("t").index
    # pattern, predicate and expression filters as examples
    cases = [
        ({"doc": "d7"}, lambda m: m.get("doc") == "d7", None, None),
        ({"doc": "d14", "tenant": "t2"}, lambda m: m.get("doc") == "d14" and m["tenant"] == "t2", {"doc": "d21"}, lambda m: m.get("doc") == "d21"),
        ({"doc": In(["d3", "d10"])}, lambda m: m.get("doc") in ("d3", "d10"), {"year": Ge("2029")}, lambda m: m["year"] >= "2029"),
        (AnyOf({"id": "5"}, {"id": "77"}, {"doc": "d28"}), lambda m: m["id"] in ("5", "77") or m.get("doc") == "d28", {"id": "6"}, lambda m: m["id"] == "6"),
        ({"id": "123"}, lambda m: m["id"] == "123", None, None),
    ]
    pos, neg = [c[0] for c in cases], [c[2] for c in cases]
    for k in (1, 10):
        s0 = ix.get_stat("flat_like_calls")
        got = db.batch_search_like("t", pos, k, neg)
        assert ix.get_stat("flat_like_calls") == s0 + 1  # the whole batch: ONE call
        exp = [md.expect(c[1], k, c[3]) for c in cases]
        assert [_tags(r) for r in got] == exp, k
        for c, e in zip(cases, exp):
            assert _tags(db.search_like("t", c[0], k, c[2])) == e
    # the examples are left out -- unless asked for: a single positive row is then its own nearest hit
    got = db.search_like("t", {"id": "123"}, 3, exclude_examples=False)
    assert got[0][0]["id"] == "123" and _tags(got) == md.expect(cases[4][1], 3, exclude=False)
    assert "123" not in [m["id"] for m, _ in db.search_like("t", {"id": "123"}, 50)]
    # filter: one for the batch, one per query, an expression; upper_bound afterwards; with_vectors
    filt, pred = {"tenant": "t1"}, (lambda m: m["tenant"] == "t1")
    s0 = ix.get_stat("flat_like_calls")
    got = db.batch_search_like("t", pos, 8, neg, filters=filt)
    assert ix.get_stat("flat_like_calls") == s0 + 1
    assert [_tags(r) for r in got] == [md.expect(c[1], 8, c[3], pred=pred) for c in cases]
    assert all(m["tenant"] == "t1" for r in got for m, _ in r)
    filters = [{"tenant": "t%d" % (i % 4)} if i % 2 else AnyOf({"doc": "big"}, {"tenant": "t2"}) for i in range(len(cases))]
    preds = [(lambda m, i=i: m["tenant"] == "t%d" % (i % 4)) if i % 2 else (lambda m: m.get("doc") == "big" or m["tenant"] == "t2") for i in range(len(cases))]
    got = db.batch_search_like("t", pos, 8, neg, filters=filters)
    assert [_tags(r) for r in got] == [md.expect(c[1], 8, c[3], pred=p) for c, p in zip(cases, preds)]
    assert db.search_like("t", {"doc": "d7"}, 5, filter={"tenant": "nobody"}) == []
    full = md.expect(cases[1][1], 10, cases[1][3])
    ub = sorted(d for _, d in full)[4]
    got = db.search_like("t", pos[1], 10, neg[1], upper_bound=ub)
    assert _tags(got) == [e for e in full if e[1] <= ub] and len(got) == 5
    got = db.batch_search_like("t", pos, 5, neg, with_vectors=True)
    assert [_tags(r) for r in got] == [md.expect(c[1], 5, c[3]) for c in cases]
    by_tag = {m["id"]: i for i, m in enumerate(md.meta)}
    assert all(np.array_equal(v, md.vecs[by_tag[m["id"]]]) for r in got for m, _, v in r)
    assert db.batch_search_like("t", [], 5) == []


def test_the_two_value_errors_name_the_query():
    md = Model(n=1300)
    db, ix = md.db, md.db._t("t").index
    s0 = ix.get_stat("flat_like_calls")
    with pytest.raises(ValueError, match="query 1: the positive filter matches no row"):
        db.batch_search_like("t", [{"doc": "d7"}, {"doc": "nothing"}], 5)
    with pytest.raises(ValueError, match="matches no row"):
        db.search_like("t", {"tenant": "t9"}, 5)
    with pytest.raises(ValueError, match="query 2 has 1300 example rows"):
        db.batch_search_like("t", [{"doc": "d7"}, {"doc": "d14"}, {}], 5)
    n_d7 = sum(m.get("doc") == "d7" for m in md.meta)
    with pytest.raises(ValueError, match="query 0 has %d example rows" % (n_d7 + 1300)):  # positives plus negatives
        db.batch_search_like("t", [{"doc": "d7"}], 5, [{}])
    assert ix.get_stat("flat_like_calls") == s0
    t0 = sum(m["tenant"] == "t0" for m in md.meta)
    assert t0 <= 1024 and len(db.search_like("t", {"tenant": "t0"}, 5)) == 5  # (325 examples: fine)


def test_examples_follow_the_metadata_after_every_kind_of_write():
    md = Model(n=500)
    db = md.db
    pos, ppred = {"doc": "d7"}, (lambda m: m.get("doc") == "d7")
    neg, npred = {"doc": "d21", "tenant": "t3"}, (lambda m: m.get("doc") == "d21" and m["tenant"] == "t3")

    def check(what):
        got = db.batch_search_like("t", [pos, {"doc": "new"}] if any(m.get("doc") == "new" for m in md.meta) else [pos], 8, None)
        exp = [md.expect(ppred, 8)] + ([md.expect(lambda m: m.get("doc") == "new", 8)] if len(got) == 2 else [])
        assert [_tags(r) for r in got] == exp, what
        assert _tags(db.search_like("t", pos, 8, neg, filter={"tenant": "t3"})) == md.expect(ppred, 8, npred, pred=lambda m: m["tenant"] == "t3"), what

    check("fresh")
    md.add([{"id": "n%d" % i, "tenant": "t3", "doc": "new" if i % 20 == 0 else "d7" if i % 20 == 1 else "x"} for i in range(200)])
    check("after batch_add")
    assert db.delete("t", {"doc": "big"}) > 0
    keep = [i for i, m in enumerate(md.meta) if m.get("doc") != "big"]
    md.meta, md.vecs = [md.meta[i] for i in keep], md.vecs[keep]
    md.sync_rows()
    check("after delete")
    # new vectors for the positive rows: the query vector moves with them
    moved = [m["id"] for m in md.meta if m.get("doc") == "d7"][:5]
    vecs = md.rng.random((len(moved), DIM)).astype(np.float32)
    assert db.batch_update("t", [{"id": t} for t in moved], list(vecs)) == [1] * len(moved)
    by_tag = {m["id"]: i for i, m in enumerate(md.meta)}
    for t, v in zip(moved, vecs):
        md.vecs[by_tag[t]] = v
    check("after update")
    # relabelled rows: they stop being examples, others become examples
    assert db.update_metadata("t", {"doc": "d14"}, {"doc": "d7"}) > 0
    for m in md.meta:
        if m.get("doc") == "d14":
            m["doc"] = "d7"
    check("after update_metadata")
    assert db.update_metadata("t", {"id": moved[0]}, {"doc": "gone"}) == 1
    md.meta[by_tag[moved[0]]]["doc"] = "gone"
    check("after a second update_metadata")
