"""GPU: VecDB.delete over the bulk removal path -- one remove_rows call for all matches, the metadata permuted by the moves it returns.
The resulting row and metadata order is MetadataVecTable::delete's (swap_remove in descending match order, metadata_vec_table.rs:176-186),
replayed here in numpy."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def test_delete_by_pattern_is_one_bulk_call():
    from lab_1806_vec_db_amd.vecdb import VecDB

    n, dim = 3000, 64
    rng = np.random.default_rng(7)
    rows = rng.standard_normal((n, dim)).astype(np.float32)
    meta = [{"id": str(i), "par": str(i % 3)} for i in range(n)]
    db = VecDB()
    db.create_table_if_not_exists("t", dim, "l2sqr")
    db.batch_add("t", rows, meta)
    ix = db._t("t").index
    db.search("t", rows[5], 3)
    db.search("t", rows[5], 3, filter={"par": "2"})  # (a cached mask of the old state: dropped by the delete)

    calls = []
    real = ix._lib.vdb_index_swap_remove

    class Counting:  # the binding, with vdb_index_swap_remove counted
        def __init__(self, lib):
            self._lib = lib

        def __getattr__(self, name):
            if name == "vdb_index_swap_remove":
                def counted(*a):
                    calls.append(a)
                    return real(*a)
                return counted
            return getattr(self._lib, name)

    ix._lib = Counting(ix._lib)
    try:
        assert db.delete("t", {"par": "1"}) == 1000
        assert calls == []
        ix.swap_remove(len(ix) - 1)  # (the counter does see a call that is made; the last row's metadata go with it)
        db._t("t").metadata.pop()
        assert len(calls) == 1
    finally:
        ix._lib = ix._lib._lib
    # numpy replay of swap_remove in descending match order, then of the removal of the last row made by hand above
    order = list(range(n))
    for i in reversed([i for i in range(n) if i % 3 == 1]):
        order[i] = order[-1]
        order.pop()
    order.pop()
    assert db.get_len("t") == len(order) == 1999
    data = db.extract_data("t")
    assert [int(m["id"]) for _, m in data] == order
    assert all(m == meta[o] for (_, m), o in zip(data, order))
    assert np.array_equal(np.asarray([v for v, _ in data], dtype=np.float32), rows[order])
    # searches name rows whose metadata are the rows' own
    for probe in (order[1], order[4], order[1500]):  # slots 1 and 4 were refilled from the tail
        res = db.search("t", rows[probe], 4)
        assert res[0][0] == meta[probe] and res[0][1] == 0.0 and all(m["par"] != "1" for m, _ in res)
        for m, d in res:  # the metadata of a hit are those of the row at that distance (f32 folds: a loose numeric check)
            assert abs(d - ((rows[int(m["id"])].astype(np.float64) - rows[probe]) ** 2).sum()) < 1e-3
        fres = db.search("t", rows[probe], 4, filter={"par": meta[probe]["par"]})
        assert fres[0][0] == meta[probe] and all(m["par"] == meta[probe]["par"] for m, _ in fres)
        want = [r for r in db.search("t", rows[probe], len(order)) if r[0]["par"] == meta[probe]["par"]][:4]
        assert fres == want
    assert db.search("t", rows[1], 1)[0][0]["id"] != "1"  # a deleted row does not come back
    assert db.delete("t", {"par": "1"}) == 0 and db.delete("t", {"par": "nope"}) == 0
    assert db.get_len("t") == 1999
