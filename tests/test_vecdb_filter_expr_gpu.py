"""GPU: VecDB filters that are EXPRESSIONS (labels.py: AnyOf, AllOf, Not over patterns, nested).  Every answer of search / batch_search /
search_within / batch_search_within is compared -- ids and distances exactly -- with the same library call restricted by a HOST-built
mask (GpuIndex.make_mask) of the rows a lambda written in this file selects from the metadata; the "mask_where_any_masks" /
"mask_combine_masks" / "mask_where_set_masks" / "mask_where_masks" counters of the table's index show which path built a mask."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

DIM = 16
N = 3000
LANGS = ("en", "fr", "de", "it", "es")
COUNTERS = ("mask_where_any_masks", "mask_combine_masks", "mask_where_set_masks", "mask_where_masks")


def _meta(i):
    m = {"id": str(i), "tenant": f"t{i % 40}", "year": "n/a" if i % 97 == 0 else str(1990 + (i * 11) % 35)}
    if i % 6:
        m["lang"] = LANGS[i % 5]
    if i % 4:
        m["source"] = ("web", "mail", "scan")[i % 3]
    if i % 50 == 0:
        m["shared"] = "yes"
    return m


def _year(m):
    try:
        return float(m["year"]) if "year" in m else None
    except ValueError:
        return None


def _cases():
    """(expression, the same thing as a lambda on a row's metadata)"""
    from lab_1806_vec_db_amd.labels import AllOf, AnyOf, Between, Exists, Ge, In, Lt, Ne, Not

    y = _year
    return (
        (AllOf({"tenant": "t3"}, AnyOf({"source": "web"}, {"year": Ge(2010)})),
         lambda m: m["tenant"] == "t3" and (m.get("source") == "web" or (y(m) is not None and y(m) >= 2010))),
        (Not(AllOf({"source": "web"}, {"lang": "de"})), lambda m: not (m.get("source") == "web" and m.get("lang") == "de")),
        (AnyOf({"tenant": In(["t1", "t2", "t39"])}, {"shared": "yes"}), lambda m: m["tenant"] in ("t1", "t2", "t39") or m.get("shared") == "yes"),
        (AnyOf({"lang": "en", "source": "mail"}, {"lang": "fr", "year": Lt(2000)}, {"lang": None}),
         lambda m: (m.get("lang") == "en" and m.get("source") == "mail") or (m.get("lang") == "fr" and y(m) is not None and y(m) < 2000) or "lang" not in m),
        (Not({"lang": In(["en", "de"]), "year": Between(1995, 2015)}),
         lambda m: not (m.get("lang") in ("en", "de") and y(m) is not None and 1995 <= y(m) <= 2015)),
        (Not(Not({"tenant": "t7"})), lambda m: m["tenant"] == "t7"),
        (AllOf(Not({"source": Exists()}), AnyOf({"lang": Ne("it")}, Not({"year": Ge(2000)}))),
         lambda m: "source" not in m and (m.get("lang") != "it" or not (y(m) is not None and y(m) >= 2000))),
        (AnyOf(AllOf({"tenant": In(["t0", "t10", "t20"])}, Not(AnyOf({"lang": "es"}, {"source": "scan"}))), AllOf({"shared": "yes"}, {"year": Ge(2005)})),
         lambda m: (m["tenant"] in ("t0", "t10", "t20") and not (m.get("lang") == "es" or m.get("source") == "scan"))
         or (m.get("shared") == "yes" and y(m) is not None and y(m) >= 2005)),
        (AnyOf(), lambda m: False),
        (AllOf(), lambda m: True),
        (AnyOf({"tenant": "nobody"}, {"lang": "xx"}), lambda m: False),
        (AllOf({"lang": "de"}), lambda m: m.get("lang") == "de"),
    )


def _make(n=N, seed=31):
    from lab_1806_vec_db_amd.vecdb import VecDB

    rng = np.random.default_rng(seed)
    db = VecDB()
    db.create_table_if_not_exists("t", DIM, "l2sqr")
    db.batch_add("t", rng.random((n, DIM)).astype(np.float32), [_meta(i) for i in range(n)])
    return db, rng


def _tags(res):
    return [(m["id"], d) for m, d in res]


class _Ref:
    """the reference answers of one table state: the library's own filtered calls under host-built masks of the rows the lambdas select"""

    def __init__(self, db):
        self.t = db._tables["t"]
        self.ix = self.t.index
        self.meta = [dict(m) for m in self.t.metadata]

    def allow(self, want):
        return np.array([bool(want(m)) for m in self.meta], dtype=np.bool_)

    def _out(self, idx, dist):
        return [(self.meta[int(i)]["id"], float(d)) for i, d in zip(idx, dist)]

    def search(self, q, k, want):
        hm = self.ix.make_mask(self.allow(want))
        idx, dist = self.ix.flat_knn_filtered(q, k, hm)
        hm.close()
        return self._out(idx, dist)

    def within(self, q, ub, want):
        hm = self.ix.make_mask(self.allow(want))
        _, idx, dist = self.ix.range_search(q, np.float32(ub), None, mask=hm)
        hm.close()
        return self._out(idx, dist)

    def batch(self, qs, k, wants):
        masks = [self.ix.make_mask(self.allow(w)) for w in wants]
        idx, dist, cnt = self.ix.flat_knn_filtered_multi(qs, k, masks, np.arange(len(wants), dtype=np.uint32))
        for mk in masks:
            mk.close()
        return [self._out(idx[j, :int(cnt[j])], dist[j, :int(cnt[j])]) for j in range(len(wants))]

    def batch_within(self, qs, ub, wants):
        masks = [self.ix.make_mask(self.allow(w)) for w in wants]
        lims, idx, dist = self.ix.range_search_multi(qs, np.full(len(wants), ub, dtype=np.float32), masks, np.arange(len(wants), dtype=np.uint32), None)
        for mk in masks:
            mk.close()
        return [self._out(idx[int(lims[j]):int(lims[j + 1])], dist[int(lims[j]):int(lims[j + 1])]) for j in range(len(wants))]


def _stats(ix):
    return [ix.get_stat(s) for s in COUNTERS]


def _check_all(db, qs, what):
    ref = _Ref(db)
    cases = _cases()
    for j, (e, want) in enumerate(cases):
        q = qs[j % len(qs)]
        for k in (1, 10):
            assert _tags(db.search("t", q, k, filter=e)) == ref.search(q, k, want), (what, e, k)
        assert _tags(db.search_within("t", q, 1.2, filter=e)) == ref.within(q, 1.2, want), (what, e)
    # one filter per query: expressions mixed with patterns; repeated expressions share a mask
    mixed = list(cases) + [({"lang": "en"}, lambda m: m.get("lang") == "en"), ({}, lambda m: True)] + list(cases[:3])
    bq = np.concatenate([qs] * (len(mixed) // len(qs) + 1))[:len(mixed)]
    got = db.batch_search("t", bq, 10, filters=[e for e, _ in mixed])
    for (e, _), g, w in zip(mixed, got, ref.batch(bq, 10, [w for _, w in mixed])):
        assert _tags(g) == w, (what, e)
    got = db.batch_search_within("t", bq, 1.2, filters=[e for e, _ in mixed])
    for (e, _), g, w in zip(mixed, got, ref.batch_within(bq, 1.2, [w for _, w in mixed])):
        assert _tags(g) == w, (what, e)
    one = db.batch_search("t", bq[:3], 5, filters=cases[0][0])  # ONE expression for every query
    assert [_tags(g) for g in one] == [ref.search(q, 5, cases[0][1]) for q in bq[:3]], what


def test_answers_and_counters_before_and_after_writes():
    db, rng = _make()
    try:
        t = db._tables["t"]
        ix = t.index
        qs = rng.random((4, DIM)).astype(np.float32)
        cases = _cases()
        assert ix.get_stat("label_columns") == 0
        _check_all(db, qs, "fresh table")
        assert sorted(t.codec.keys()) == ["lang", "shared", "source", "tenant", "year"] and ix.get_stat("label_columns") == 5
        # every expression's mask was built by the any call, once; the two patterns of the batch by the equality call; nothing combined
        assert _stats(ix) == [len(cases), 0, 0, 2] and len(t.masks) == len(cases) + 2
        ref = _Ref(db)
        sizes = [int(ref.allow(w).sum()) for _, w in cases]
        assert all(0 < s < N for s in sizes[:8]) and sizes[8:11] == [0, N, 0], sizes  # the lambdas select proper subsets
        # after a batch_add: masks are dropped and rebuilt; values first seen among the new rows take part
        new_meta = [{"id": f"n{i}", "tenant": ("t3", "t99")[i % 2], "lang": ("pt", "en", "de")[i % 3], "year": str(2008 + i % 6), "source": "web"} if i % 5
                    else {"id": f"n{i}", "tenant": "t1"} for i in range(61)]
        db.batch_add("t", rng.random((61, DIM)).astype(np.float32), new_meta)
        assert not t.masks
        s0 = _stats(ix)
        _check_all(db, qs, "after batch_add")
        assert _stats(ix) == [s0[0] + len(cases), s0[1], s0[2], s0[3] + 2]
        db.delete("t", {"lang": "it"})
        assert not t.masks
        _check_all(db, qs, "after delete")
    finally:
        db.delete_table("t")


def test_batch_builds_its_expression_masks_in_one_call():
    from lab_1806_vec_db_amd.labels import AnyOf, Ge, In, Not

    db, rng = _make(n=600)
    try:
        t = db._tables["t"]
        ix = t.index
        qs = rng.random((13, DIM)).astype(np.float32)
        exprs = [AnyOf({"lang": In([LANGS[j % 5], LANGS[(j + 2) % 5]])}, Not({"year": Ge(1990 + j)})) for j in range(10)]
        filters = exprs + [{"lang": "en"}, {}, exprs[4]]
        calls = []
        real = ix.make_masks_where_any
        ix.make_masks_where_any = lambda lists: calls.append(len(lists)) or real(lists)
        got = db.batch_search("t", qs, 5, filters=filters)
        assert calls == [10] and _stats(ix) == [10, 0, 0, 2]
        assert got[12] == db.search("t", qs[12], 5, filter=exprs[4]) and calls == [10]  # (the repeated expression: the cached mask)
        assert db.batch_search("t", qs, 5, filters=filters) == got and calls == [10]    # cached: no call
        assert db.batch_search_within("t", qs, 0.9, filters=filters) is not None and calls == [10]
    finally:
        db.delete_table("t")


def test_a_dict_filter_keeps_its_path():
    from lab_1806_vec_db_amd.labels import AnyOf, Ge, In

    db, rng = _make(n=400)
    try:
        ix = db._tables["t"].index
        q = rng.random(DIM).astype(np.float32)
        db.search("t", q, 3, filter={"lang": "en", "tenant": "t4"})
        assert _stats(ix) == [0, 0, 0, 1]
        db.search_within("t", q, 1.0, filter={"lang": In(["en", "fr"]), "year": Ge(2000)})
        assert _stats(ix) == [0, 0, 1, 1]
        db.batch_search("t", q.reshape(1, -1), 3, filters=[{"year": Ge(2001)}])
        db.batch_search_within("t", q.reshape(1, -1), 1.0, filters={"lang": "de"})
        assert _stats(ix) == [0, 0, 2, 2]
        with pytest.raises(TypeError):
            db.delete("t", AnyOf({"lang": "en"}))  # delete keeps taking a pattern only
        assert db.delete("t", {"id": "5"}) == 1
        assert _stats(ix) == [0, 0, 2, 2]  # (a delete gives no key a column: "id" stays on the host)
        assert len(db._tables["t"].metadata) == 399
    finally:
        db.delete_table("t")


def test_what_the_columns_cannot_express_is_assembled_from_masks():
    from lab_1806_vec_db_amd.labels import AllOf, AnyOf, In, Ne, Not
    from lab_1806_vec_db_amd.vecdb import VecDB

    n = 300
    rng = np.random.default_rng(5)
    db = VecDB()
    db.create_table_if_not_exists("t", DIM, "l2sqr")
    vals = rng.integers(0, 4, size=(n, 17))
    meta = [{"id": str(i), **{f"k{j}": str(vals[i, j]) for j in range(17)}} for i in range(n)]
    db.batch_add("t", rng.random((n, DIM)).astype(np.float32), meta)
    try:
        t = db._tables["t"]
        ix = t.index
        q = rng.random(DIM).astype(np.float32)
        for j in range(16):
            db.search("t", q, 1, filter={f"k{j}": Ne("0")})
        assert len(t.codec.keys()) == 16 and _stats(ix) == [0, 0, 16, 0]
        ref = _Ref(db)
        # a 17th key: its pattern is matched by the host loop, the other operands on the device, and the masks are joined
        e1 = AnyOf({"k0": "2"}, {"k16": In(["1", "3"])})
        w1 = lambda m: m["k0"] == "2" or m["k16"] in ("1", "3")  # noqa: E731
        s0 = _stats(ix)
        assert _tags(db.search("t", q, 40, filter=e1)) == ref.search(q, 40, w1)
        assert _stats(ix) == [s0[0], s0[1] + 1, s0[2], s0[3] + 1]  # one join; {"k0": "2"} through the equality call, k16 on the host
        e2 = AllOf(Not({"k16": "0"}), AnyOf({"k1": "1"}, {"k2": Ne("3")}), Not(e1))
        w2 = lambda m: m["k16"] != "0" and (m["k1"] == "1" or m["k2"] != "3") and not w1(m)  # noqa: E731
        s0 = _stats(ix)
        assert _tags(db.search_within("t", q, 1.5, filter=e2)) == ref.within(q, 1.5, w2)
        assert _tags(db.batch_search("t", q.reshape(1, -1), 40, filters=[e2])[0]) == ref.search(q, 40, w2)
        # one join for e2 (e1's mask is cached, Not operands are complemented inside the join); its expressible operand through the any call
        assert _stats(ix) == [s0[0] + 1, s0[1] + 1, s0[2], s0[3]]
        # a normal form past 64 clauses: seven 2-way ORs under an AND, all on columns -- its operands are built by ONE any call, then joined
        e3 = AllOf(*[AnyOf({f"k{j}": In(["1", "2"])}, {f"k{j + 7}": "2"}) for j in range(7)])
        w3 = lambda m: all(m[f"k{j}"] in ("1", "2") or m[f"k{j + 7}"] == "2" for j in range(7))  # noqa: E731
        assert t.codec.compile_any(e3) is None
        calls = []
        real = ix.make_masks_where_any
        ix.make_masks_where_any = lambda lists: calls.append(len(lists)) or real(lists)
        s0 = _stats(ix)
        assert _tags(db.search("t", q, 40, filter=e3)) == ref.search(q, 40, w3)
        assert calls == [7] and _stats(ix) == [s0[0] + 7, s0[1] + 1, s0[2], s0[3]]
        # nine operands: two joins (eight, then the result with the ninth)
        e4 = AnyOf(*[{"k16": str(v % 4), f"k{v}": "0"} for v in range(9)])
        w4 = lambda m: any(m["k16"] == str(v % 4) and m[f"k{v}"] == "0" for v in range(9))  # noqa: E731
        s0 = _stats(ix)
        assert _tags(db.search("t", q, 40, filter=e4)) == ref.search(q, 40, w4)
        assert _stats(ix) == [s0[0], s0[1] + 2, s0[2], s0[3]]
        for w in (w1, w2, w3, w4):
            assert 0 < int(ref.allow(w).sum()) < n
        # writes drop every cached mask, the operands' included
        db.batch_add("t", rng.random((1, DIM)).astype(np.float32), [dict(meta[0], id="new")])
        assert not t.masks
        ref = _Ref(db)
        assert _tags(db.search("t", q, 40, filter=e2)) == ref.search(q, 40, w2)
    finally:
        db.delete_table("t")
