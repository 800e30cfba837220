"""GPU: VecDB.count / VecDB.count_by, and the routing of one-key patterns of a batch_search through GpuIndex.make_masks_partition.
count and count_by are compared with a lambda and a collections.Counter over the metadata written in this file; the routed
batch_search with the same batch built by make_masks_where (vecdb.PARTITION_MIN huge), ids and distances exactly."""
import collections
import threading

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

DIM = 8
N = 3000
LANGS = ("en", "fr", "de", "it", "es")
HUGE = 1 << 60


def _meta(i):
    m = {"id": str(i), "tenant": f"t{i % 40}", "year": str(1990 + (i * 11) % 35)}
    if i % 6:
        m["lang"] = LANGS[i % 5]
    if i % 4:
        m["source"] = ("web", "mail", "scan")[i % 3]
    return m


def _make(n=N, seed=31):
    from lab_1806_vec_db_amd.vecdb import VecDB

    rng = np.random.default_rng(seed)
    db = VecDB()
    db.create_table_if_not_exists("t", DIM, "l2sqr")
    db.batch_add("t", rng.random((n, DIM)).astype(np.float32), [_meta(i) for i in range(n)])
    return db, rng


def _filters():
    """(filter, the same thing as a lambda on a row's metadata): none, a pattern, a predicate, an AnyOf / Not expression"""
    from lab_1806_vec_db_amd.labels import AnyOf, Ge, Not

    return (
        (None, lambda m: True),
        ({"tenant": "t3"}, lambda m: m["tenant"] == "t3"),
        ({"lang": "de", "source": "web"}, lambda m: m.get("lang") == "de" and m.get("source") == "web"),
        ({"year": Ge(2010)}, lambda m: float(m["year"]) >= 2010),
        (AnyOf({"tenant": "t1"}, Not({"lang": "en"})), lambda m: m["tenant"] == "t1" or m.get("lang") != "en"),
        ({"tenant": "nobody"}, lambda m: False),
    )


def _check_all(db, meta):
    for f, fn in _filters():
        rows = [m for m in meta if fn(m)]
        assert db.count("t", f) == len(rows), f
        for field in ("tenant", "lang", "source"):  # lang and source: fields some rows lack, counted under None
            want = dict(collections.Counter(m.get(field) for m in rows))
            assert db.count_by("t", field, f) == want, (f, field)


def test_count_and_count_by_before_and_after_writes():
    db, rng = _make()
    meta = [_meta(i) for i in range(N)]
    ix = db._t("t").index
    assert db.count("t") == db.get_len("t") == N
    c0 = ix.get_stat("label_count_calls")
    _check_all(db, meta)
    assert ix.get_stat("label_count_calls") == c0 + 3 * len(_filters())  # every count_by was one pass on the device
    extra = [_meta(i) for i in range(N, N + 500)]
    db.batch_add("t", rng.random((500, DIM)).astype(np.float32), extra)
    meta += extra
    _check_all(db, meta)
    assert db.delete("t", {"tenant": "t7"}) == sum(1 for m in meta if m["tenant"] == "t7")
    # the table's rows after the delete, whatever order the removal left them in
    meta = [m for _, m in db.extract_data("t")]
    assert len(meta) == db.count("t") and all(m["tenant"] != "t7" for m in meta)
    _check_all(db, meta)
    assert "t7" not in db.count_by("t", "tenant")


def test_a_field_no_filter_has_named_gets_its_column():
    db, _ = _make(500)
    meta = [_meta(i) for i in range(500)]
    t = db._t("t")
    assert t.codec.column_of("year") is None and t.index.get_stat("label_columns") == 0
    want = dict(collections.Counter(m.get("year") for m in meta))
    assert db.count_by("t", "year") == want
    assert t.codec.column_of("year") == 0 and t.index.get_stat("label_columns") == 1 and t.index.get_stat("label_count_calls") == 1
    assert db.count_by("t", "no such field") == {None: 500}
    assert db.count_by("t", "year", {"lang": "fr"}) == dict(collections.Counter(m.get("year") for m in meta if m.get("lang") == "fr"))


def test_the_17th_key_and_unhashable_values_take_the_host_loop():
    from lab_1806_vec_db_amd.vecdb import VecDB

    rng = np.random.default_rng(2)
    n = 300
    meta = [{f"k{j}": str((i * (j + 1)) % 5) for j in range(17)} for i in range(n)]
    db = VecDB()
    db.create_table_if_not_exists("t", DIM, "l2sqr")
    db.batch_add("t", rng.random((n, DIM)).astype(np.float32), meta)
    t = db._t("t")
    for j in range(16):
        assert db.count_by("t", f"k{j}") == dict(collections.Counter(m[f"k{j}"] for m in meta)), j
    assert t.index.get_stat("label_columns") == 16 and t.index.get_stat("label_count_calls") == 16
    assert db.count_by("t", "k16") == dict(collections.Counter(m["k16"] for m in meta))  # no column left: the host loop
    assert db.count_by("t", "k16", {"k0": "1"}) == dict(collections.Counter(m["k16"] for m in meta if m["k0"] == "1"))
    assert t.index.get_stat("label_columns") == 16 and t.index.get_stat("label_count_calls") == 16
    assert db.count("t", {"k16": "2"}) == sum(1 for m in meta if m["k16"] == "2")
    # a column whose dictionary holds values it cannot keep apart: the host loop again (which refuses to hash them, as Counter does)
    db2 = VecDB()
    db2.create_table_if_not_exists("t", DIM, "l2sqr")
    db2.batch_add("t", rng.random((4, DIM)).astype(np.float32), [{"a": "x"}, {"a": ["u"]}, {"a": "x"}, {}])
    with pytest.raises(TypeError):
        db2.count_by("t", "a")
    assert db2._t("t").index.get_stat("label_count_calls") == 0


def test_two_threads_count():
    db, _ = _make()
    meta = [_meta(i) for i in range(N)]
    errors = []

    def work(field):
        try:
            for _ in range(5):
                for f, fn in _filters():
                    rows = [m for m in meta if fn(m)]
                    assert db.count("t", f) == len(rows)
                    assert db.count_by("t", field, f) == dict(collections.Counter(m.get(field) for m in rows))
        except BaseException as e:  # noqa: BLE001 -- reported by the main thread
            errors.append(e)

    ts = [threading.Thread(target=work, args=(f,)) for f in ("tenant", "lang")]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert not errors, errors


def _with_partition_min(value, fn):
    from lab_1806_vec_db_amd import vecdb

    old = vecdb.PARTITION_MIN
    vecdb.PARTITION_MIN = value
    try:
        return fn()
    finally:
        vecdb.PARTITION_MIN = old


def test_batch_search_routes_one_key_patterns_through_the_partition():
    qs = np.random.default_rng(9).random((40, DIM)).astype(np.float32)
    filters = [{"tenant": f"t{(7 * q) % 40}"} for q in range(40)]
    answers, stats = {}, {}
    for pm in (1, HUGE, None):
        db, _ = _make()
        ix = db._t("t").index
        db.search("t", qs[0], 1, filter={"tenant": "t0"})  # the column exists and the counters start from a searched table
        db.batch_add("t", np.zeros((1, DIM), dtype=np.float32), [{"tenant": "t0"}])  # a write drops the cached masks
        s0 = (ix.get_stat("mask_partition_masks"), ix.get_stat("mask_where_masks"))
        answers[pm] = _with_partition_min(pm, lambda: db.batch_search("t", qs, 10, filters=filters))
        stats[pm] = (ix.get_stat("mask_partition_masks") - s0[0], ix.get_stat("mask_where_masks") - s0[1])
    assert stats[1] == (40, 0) and stats[HUGE] == (0, 40) and stats[None] == (0, 40)
    assert answers[1] == answers[HUGE] == answers[None]
    assert all(len(a) == 10 and all(m["tenant"] == f["tenant"] for m, _ in a) for a, f in zip(answers[1], filters))


def test_a_mixed_batch_routes_only_the_one_key_patterns():
    from lab_1806_vec_db_amd.labels import AnyOf, Ge

    qs = np.random.default_rng(10).random((12, DIM)).astype(np.float32)
    filters = [{"tenant": "t1"}, {"tenant": "t2"}, {"lang": "de"}, {"lang": None}, {"tenant": "t3", "lang": "fr"}, {}, AnyOf({"tenant": "t4"}, {"source": "web"}),
               {"year": Ge(2015)}, {"tenant": "never seen"}, {"lang": "en"}, {"tenant": "t1"}, {"source": "scan"}]
    answers, stats = {}, {}
    for pm in (1, 2, HUGE):
        db, _ = _make()
        ix = db._t("t").index
        names = ("mask_partition_masks", "mask_where_masks", "mask_where_set_masks", "mask_where_any_masks")
        answers[pm] = _with_partition_min(pm, lambda: db.batch_search("t", qs, 5, filters=filters))
        stats[pm] = tuple(ix.get_stat(s) for s in names)
    # one-key plain patterns with a known value: tenant t1, t2 | lang de, None, en | source scan.  {"tenant": "never seen"} compiles to
    # the two-term empty conjunction, the two-key pattern and {} are no one-term patterns: make_masks_where, as before
    assert stats[1] == (6, 3, 1, 1), stats
    assert stats[2] == (5, 4, 1, 1), stats  # the group of one on `source` stays with make_masks_where
    assert stats[HUGE] == (0, 9, 1, 1), stats
    assert answers[1] == answers[2] == answers[HUGE]
