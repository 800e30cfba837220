"""GPU: VecDB filters that hold predicates (labels.py: In, NotIn, Ne, Exists, Lt, Le, Gt, Ge, Between).  Every answer of search /
search_within / batch_search is compared -- ids and distances exactly -- with the same library call restricted by a HOST-built mask
(GpuIndex.make_mask) of the rows a lambda written in this file selects from the metadata; the "mask_where_set_masks" /
"mask_where_masks" counters of the table's index show which path built a mask."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

DIM = 16
N = 2000
LANGS = ("en", "fr", "de", "it", "es")


def _meta(i):
    m = {"id": str(i), "year": "n/a" if i % 97 == 0 else str(1990 + (i * 11) % 35)}
    if i % 6:
        m["lang"] = LANGS[i % 5]
    return m


def _num(x):
    try:
        return float(x) if isinstance(x, str) else None
    except ValueError:
        return None


def _cases():
    """(pattern, the same thing as a lambda on a row's metadata)"""
    from lab_1806_vec_db_amd.labels import Between, Exists, Ge, Gt, In, Le, Lt, Ne, NotIn

    year = lambda m: _num(m.get("year"))  # noqa: E731
    return (
        ({"lang": In(["en", "de"])}, lambda m: m.get("lang") in ("en", "de")),
        ({"lang": In(["fr", None])}, lambda m: m.get("lang") in ("fr", None)),
        ({"lang": In(["xx"])}, lambda m: False),
        ({"lang": NotIn(["en", "de"])}, lambda m: m.get("lang") not in ("en", "de")),
        ({"lang": NotIn(["it", None])}, lambda m: m.get("lang") not in ("it", None)),
        ({"lang": Ne("fr")}, lambda m: m.get("lang") != "fr"),
        ({"lang": Exists()}, lambda m: "lang" in m),
        ({"lang": Exists(False)}, lambda m: "lang" not in m),
        ({"lang": Lt("es")}, lambda m: "lang" in m and m["lang"] < "es"),
        ({"lang": Between("en", "fr")}, lambda m: "lang" in m and "en" <= m["lang"] <= "fr"),
        ({"year": Ge(2010)}, lambda m: year(m) is not None and year(m) >= 2010),
        ({"year": Gt(2010)}, lambda m: year(m) is not None and year(m) > 2010),
        ({"year": Le(1995.5)}, lambda m: year(m) is not None and year(m) <= 1995.5),
        ({"year": Lt(2000)}, lambda m: year(m) is not None and year(m) < 2000),
        ({"year": Between(2001, 2003)}, lambda m: year(m) is not None and 2001 <= year(m) <= 2003),
        ({"year": Ge("2")}, lambda m: isinstance(m.get("year"), str) and m["year"] >= "2"),  # string order: "n/a" >= "2"
        ({"lang": In(["en", "fr"]), "year": Ge(2010)}, lambda m: m.get("lang") in ("en", "fr") and year(m) is not None and year(m) >= 2010),
        ({"lang": "de", "year": Ne("2003")}, lambda m: m.get("lang") == "de" and m.get("year") != "2003"),
    )


PLAIN = (({"lang": "en"}, lambda m: m.get("lang") == "en"), ({}, lambda m: True), ({"lang": None}, lambda m: "lang" not in m))


def _make(n=N, seed=21):
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


def _check_all(db, qs, what):
    ref = _Ref(db)
    cases = _cases()
    for j, (p, want) in enumerate(cases):
        q = qs[j % len(qs)]
        for k in (1, 10):
            assert _tags(db.search("t", q, k, filter=p)) == ref.search(q, k, want), (what, p, k)
        assert _tags(db.search_within("t", q, 1.5, filter=p)) == ref.within(q, 1.5, want), (what, p)
    # one pattern per query, predicates mixed with plain equalities and {}
    mixed = list(cases) + list(PLAIN)
    bq = np.concatenate([qs] * (len(mixed) // len(qs) + 1))[:len(mixed)]
    got = db.batch_search("t", bq, 10, filters=[p for p, _ in mixed])
    for (p, _), g, w in zip(mixed, got, ref.batch(bq, 10, [w for _, w in mixed])):
        assert _tags(g) == w, (what, p)


def test_answers_and_counters_before_and_after_writes():
    db, rng = _make()
    try:
        t = db._tables["t"]
        ix = t.index
        qs = rng.random((4, DIM)).astype(np.float32)
        cases = _cases()
        assert ix.get_stat("label_columns") == 0
        _check_all(db, qs, "fresh table")
        assert t.codec.keys() == ["lang", "year"] and ix.get_stat("label_columns") == 2  # columns through prepare, first named by predicates
        # every predicate pattern's mask was built by the set call, every plain one's by the equality call, once each
        assert ix.get_stat("mask_where_set_masks") == len(cases) and ix.get_stat("mask_where_masks") == len(PLAIN)
        assert len(t.masks) == len(cases) + len(PLAIN)
        # not degenerate: the lambdas select proper subsets
        ref = _Ref(db)
        sizes = [int(ref.allow(w).sum()) for _, w in cases]
        assert sizes[2] == 0 and all(0 < s < N for s in sizes[:2] + sizes[3:]), sizes
        # after a batch_add: masks are dropped and rebuilt; values first seen among the new rows take part
        new_meta = [{"id": f"n{i}", "lang": ("pt", "en", "it")[i % 3], "year": str(2030 + i % 4)} if i % 5 else {"id": f"n{i}"} for i in range(61)]
        db.batch_add("t", rng.random((61, DIM)).astype(np.float32), new_meta)
        assert not t.masks
        s0, e0 = ix.get_stat("mask_where_set_masks"), ix.get_stat("mask_where_masks")
        _check_all(db, qs, "after batch_add")
        assert ix.get_stat("mask_where_set_masks") == s0 + len(cases) and ix.get_stat("mask_where_masks") == e0 + len(PLAIN)
        # after a delete with a plain pattern
        db.delete("t", {"lang": "it"})
        assert not t.masks
        _check_all(db, qs, "after delete")
    finally:
        db.delete_table("t")


def test_batch_search_builds_its_set_masks_in_one_call():
    from lab_1806_vec_db_amd.labels import Ge, In

    db, rng = _make(n=600)
    try:
        t = db._tables["t"]
        ix = t.index
        qs = rng.random((12, DIM)).astype(np.float32)
        pats = [{"lang": In([LANGS[j % 5], LANGS[(j + 2) % 5]]), "year": Ge(1990 + j)} for j in range(10)] + [{"lang": "en"}, {}]
        calls = []
        real = ix.make_masks_where_sets
        ix.make_masks_where_sets = lambda lists: calls.append(len(lists)) or real(lists)
        got = db.batch_search("t", qs, 5, filters=pats)
        assert calls == [10] and ix.get_stat("mask_where_set_masks") == 10 and ix.get_stat("mask_where_masks") == 2
        assert db.batch_search("t", qs, 5, filters=pats) == got and calls == [10]  # cached: no call
    finally:
        db.delete_table("t")


def test_predicate_on_a_seventeenth_key_takes_the_host_loop():
    from lab_1806_vec_db_amd.labels import In, Ne
    from lab_1806_vec_db_amd.vecdb import VecDB

    n = 150
    rng = np.random.default_rng(5)
    db = VecDB()
    db.create_table_if_not_exists("t", DIM, "l2sqr")
    meta = [{"id": str(i), **{f"k{j}": str((i + j) % 4) for j in range(17)}} for i in range(n)]
    db.batch_add("t", rng.random((n, DIM)).astype(np.float32), meta)
    try:
        t = db._tables["t"]
        q = rng.random(DIM).astype(np.float32)
        for j in range(16):
            db.search("t", q, 1, filter={f"k{j}": Ne("0")})
        assert len(t.codec.keys()) == 16 and t.index.get_stat("mask_where_set_masks") == 16
        ref = _Ref(db)
        for p, want in (({"k16": In(["1", "3"])}, lambda m: m["k16"] in ("1", "3")),
                        ({"k0": "2", "k16": Ne("1")}, lambda m: m["k0"] == "2" and m["k16"] != "1")):
            s0, e0 = t.index.get_stat("mask_where_set_masks"), t.index.get_stat("mask_where_masks")
            assert _tags(db.search("t", q, 40, filter=p)) == ref.search(q, 40, want), p
            assert _tags(db.batch_search("t", q.reshape(1, -1), 40, filters=[p])[0]) == ref.search(q, 40, want), p
            assert _tags(db.search_within("t", q, 1.5, filter=p)) == ref.within(q, 1.5, want), p
            assert (t.index.get_stat("mask_where_set_masks"), t.index.get_stat("mask_where_masks")) == (s0, e0)  # the host loop built it
            assert 0 < int(ref.allow(want).sum()) < n
    finally:
        db.delete_table("t")


def test_delete_with_a_predicate():
    from lab_1806_vec_db_amd.labels import Ge, In, Lt

    db, rng = _make(n=500)
    try:
        t = db._tables["t"]
        ix = t.index
        q = rng.random(DIM).astype(np.float32)
        year = lambda m: _num(m.get("year"))  # noqa: E731
        # keys without columns: the delete stays on the host and gives no key a column
        for use_columns, p, want in ((False, {"year": Ge(2015)}, lambda m: year(m) is not None and year(m) >= 2015),
                                     (True, {"lang": In(["fr", None]), "year": Lt(2000)}, lambda m: m.get("lang") in ("fr", None) and year(m) is not None and year(m) < 2000)):
            if use_columns:
                db.search("t", q, 1, filter=p)  # the keys get their columns
                assert t.codec.keys() == ["lang", "year"]
            data = db.extract_data("t")
            replay = list(data)
            hits = [i for i, (_, m) in enumerate(data) if want(m)]
            for i in reversed(hits):  # swap_remove in descending order, on a Python list
                replay[i] = replay[-1]
                replay.pop()
            s0 = ix.get_stat("mask_where_set_masks")
            assert 0 < len(hits) < len(data)
            assert db.delete("t", p) == len(hits), p
            assert ix.get_stat("mask_where_set_masks") == s0 + (1 if use_columns else 0)
            if not use_columns:
                assert t.codec.keys() == [] and ix.get_stat("label_columns") == 0
            assert db.extract_data("t") == replay, p
    finally:
        db.delete_table("t")
