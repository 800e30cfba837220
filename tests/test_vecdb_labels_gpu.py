"""GPU: VecDB keeps the keys its filter patterns use as label columns on the device and builds the patterns' masks there
(lab_1806_vec_db_amd/labels.py, GpuIndex.make_masks_where).  The answers of search / search_within / batch_search are held to a host
computation over extract_data -- the oracle's full (distance, index) order, the pairs whose metadata matches kept -- before and after
writes; the "mask_where_masks" counter of the table's index shows which path built a mask."""
import threading

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

DIM = 32
LANGS = ("en", "fr", "de")
PATTERNS = ({"lang": "en"}, {"lang": "fr", "kind": "b"}, {}, {"lang": "xx"}, {"missing": "1"}, {"kind": "a", "lang": "de"})


def _matches(meta, pattern):
    return all(meta.get(k) == v for k, v in pattern.items())


def _full_order(db, key, queries, kind):
    """per query [(row id tag, distance, metadata)] of EVERY row, nearest first, from the table as extract_data shows it: computed once per
    table state and shared by the patterns compared against it"""
    from oracle import oracle as O

    data = db.extract_data(key)
    rows = np.array([v for v, _ in data], dtype=np.float32).reshape(len(data), DIM)
    oi, od, _ = O.flat_knn_batch(rows, np.asarray(queries, dtype=np.float32).reshape(-1, DIM), len(rows), kind)
    return [[(data[int(i)][1]["id"], float(d), data[int(i)][1]) for i, d in zip(oi[q], od[q])] for q in range(len(oi))]


def _want(order, pattern):
    return [(tag, d) for tag, d, meta in order if _matches(meta, pattern)]


def _tags(res):
    return [(m["id"], d) for m, d in res]


def _meta(i):
    m = {"id": str(i), "body": f"text of row {i} " * 8, "lang": LANGS[i % 3], "kind": "a" if i % 5 else "b"}
    if i % 7 == 0:
        del m["kind"]
    return m


def _make(dist, n=400, seed=11):
    from lab_1806_vec_db_amd.vecdb import VecDB

    rng = np.random.default_rng(seed)
    db = VecDB()
    db.create_table_if_not_exists("t", DIM, dist)
    db.batch_add("t", rng.random((n, DIM)).astype(np.float32), [_meta(i) for i in range(n)])
    return db, rng.random((len(PATTERNS), DIM)).astype(np.float32), rng


def _check_all(db, qs, kind, what):
    """search, search_within and batch_search under every pattern against the host computation"""
    orders = _full_order(db, "t", qs, kind)
    for p in PATTERNS:
        for q, order in zip(qs[:2], orders[:2]):
            want = _want(order, p)
            for k in (1, 10, 500):
                assert _tags(db.search("t", q, k, filter=p)) == want[:k], (what, p, k)
            if len(want) >= 6:
                ub = want[5][1]
                assert _tags(db.search_within("t", q, ub, filter=p)) == [w for w in want if w[1] <= np.float32(ub)], (what, p)
    got = db.batch_search("t", qs, 10, filters=list(PATTERNS))
    for p, order, g in zip(PATTERNS, orders, got):
        assert _tags(g) == _want(order, p)[:10], (what, p)


@pytest.mark.parametrize("dist,kind", (("l2sqr", 0), ("cosine", 1)))
def test_answers_before_and_after_writes(dist, kind):
    db, qs, rng = _make(dist)
    try:
        t = db._tables["t"]
        ix = t.index
        assert ix.get_stat("label_columns") == 0 and t.codec.keys() == []  # nothing is interned because it exists
        _check_all(db, qs, kind, "fresh table")
        assert t.codec.keys() == ["lang", "kind", "missing"]  # in order of first use; never "id" or "body"
        assert ix.get_stat("label_columns") == 3
        assert ix.get_stat("mask_where_masks") == len(PATTERNS) == len(t.masks)  # every pattern's mask was built on the device, once
        # after a batch_add: the new rows' labels are encoded incrementally, values first seen among them included
        new_meta = [{"id": f"n{i}", "lang": ("xx", "en", "it")[i % 3], "kind": "b"} for i in range(37)]
        db.batch_add("t", rng.random((37, DIM)).astype(np.float32), new_meta)
        assert not t.masks and ix.get_stat("label_columns") == 3
        s0 = ix.get_stat("mask_where_masks")
        _check_all(db, qs, kind, "after batch_add")
        assert ix.get_stat("mask_where_masks") == s0 + len(PATTERNS)
        assert len(db.search("t", qs[0], 500, filter={"lang": "xx"})) == 13  # unseen before the add, 13 rows now
        # after a delete: the matches come from the device mask, the columns follow the removal
        for p in ({"kind": "b", "lang": "fr"}, {"lang": "zz"}, {"lang": "de"}):
            want = sum(1 for _, m in db.extract_data("t") if _matches(m, p))
            s0 = ix.get_stat("mask_where_masks")
            assert db.delete("t", p) == want, p
            assert ix.get_stat("mask_where_masks") == s0 + 1  # (the delete's own mask)
            assert db.get_len("t") == len(t.metadata) and not any(_matches(m, p) for m in t.metadata)
            _check_all(db, qs, kind, ("after delete", p))
        # a delete by a key that is no column stays on the host and interns nothing
        s0 = ix.get_stat("mask_where_masks")
        assert db.delete("t", {"id": "7"}) == 1 and ix.get_stat("mask_where_masks") == s0 and "id" not in t.codec.keys()
        _check_all(db, qs, kind, "after delete by id")
    finally:
        db.delete_table("t")


def test_seventeenth_key_falls_back_to_the_host_loop():
    from lab_1806_vec_db_amd.vecdb import VecDB

    n = 120
    rng = np.random.default_rng(5)
    db = VecDB()
    db.create_table_if_not_exists("t", DIM, "l2sqr")
    meta = [{"id": str(i), **{f"k{j}": str((i + j) % 3) for j in range(17)}} for i in range(n)]
    db.batch_add("t", rng.random((n, DIM)).astype(np.float32), meta)
    try:
        t = db._tables["t"]
        q = rng.random((1, DIM)).astype(np.float32)
        order = _full_order(db, "t", q, 0)[0]
        for j in range(17):
            s0 = t.index.get_stat("mask_where_masks")
            p = {f"k{j}": "1"}
            assert _tags(db.search("t", q[0], 50, filter=p)) == _want(order, p)[:50], j
            assert t.index.get_stat("mask_where_masks") == s0 + (1 if j < 16 else 0), j  # the 17th through the host path
        assert len(t.codec.keys()) == 16 and t.index.get_stat("label_columns") == 16
        # a pattern with a 17th key next to a column key, and one of nine keys: the host loop, same answers
        for p in ({"k0": "0", "k16": "1"}, {f"k{j}": str(j % 3) for j in range(9)}):
            s0 = t.index.get_stat("mask_where_masks")
            assert _tags(db.search("t", q[0], 50, filter=p)) == _want(order, p)[:50], p
            assert _tags(db.batch_search("t", q, 50, filters=[p])[0]) == _want(order, p)[:50], p
            assert t.index.get_stat("mask_where_masks") == s0
        assert db.delete("t", {"k16": "2"}) == sum(1 for m in meta if m["k16"] == "2")
    finally:
        db.delete_table("t")


def test_two_threads_first_use_the_same_key():
    db, qs, rng = _make("l2sqr")
    try:
        orders = _full_order(db, "t", qs[:2], 0)
        t = db._tables["t"]
        barrier = threading.Barrier(2)
        out, errs = {}, []

        def worker(w):
            try:
                barrier.wait()
                out[w] = (_tags(db.search("t", qs[w], 20, filter={"lang": "fr"})),
                          _tags(db.batch_search("t", qs[w:w + 1], 20, filters=[{"kind": "b", "lang": "en"}])[0]))
            except BaseException as e:  # noqa: BLE001
                errs.append(e)

        threads = [threading.Thread(target=worker, args=(w,)) for w in range(2)]
        for th in threads:
            th.start()
        for th in threads:
            th.join()
        assert not errs, errs
        for w in range(2):
            assert out[w][0] == _want(orders[w], {"lang": "fr"})[:20]
            assert out[w][1] == _want(orders[w], {"kind": "b", "lang": "en"})[:20]
        assert sorted(t.codec.keys()) == ["kind", "lang"] and t.index.get_stat("label_columns") == 2  # one column per key, made once
        assert len(t.masks) == 2
    finally:
        db.delete_table("t")


def test_batch_search_builds_its_masks_in_one_call():
    from lab_1806_vec_db_amd.vecdb import VecDB

    n = 400
    rng = np.random.default_rng(8)
    db = VecDB()
    db.create_table_if_not_exists("t", DIM, "l2sqr")
    db.batch_add("t", rng.random((n, DIM)).astype(np.float32), [{"id": str(i), "tenant": str(i % 50), "tier": "ab"[i % 2]} for i in range(n)])
    try:
        t = db._tables["t"]
        ix = t.index
        qs = rng.random((60, DIM)).astype(np.float32)
        pats = [{"tenant": str(j % 50)} for j in range(60)]  # 50 distinct new patterns, 10 of them repeated
        calls = []
        real = ix.make_masks_where
        ix.make_masks_where = lambda lists: calls.append(len(lists)) or real(lists)
        s0 = ix.get_stat("mask_where_masks")
        got = db.batch_search("t", qs, 5, filters=pats)
        assert calls == [50] and ix.get_stat("mask_where_masks") == s0 + 50 and len(t.masks) == 50
        orders = _full_order(db, "t", qs, 0)
        for p, order, g in zip(pats, orders, got):
            assert _tags(g) == _want(order, p)[:5], p
        # everything is cached now: no call; ten new two-key patterns beside cached ones: one call for the ten
        assert db.batch_search("t", qs, 5, filters=pats) == got and calls == [50]
        pats2 = pats[:50] + [{"tenant": str(j), "tier": "a"} for j in range(10)]
        got2 = db.batch_search("t", qs, 5, filters=pats2)
        assert calls == [50, 10] and ix.get_stat("mask_where_masks") == s0 + 60
        for p, order, g in zip(pats2, orders, got2):
            assert _tags(g) == _want(order, p)[:5], p
    finally:
        db.delete_table("t")
