"""GPU: exact range search behind the multi-GPU context (ShardedIndex.range_search / vdb_sharded_flat_range).

A test box has ONE GPU, so the exchange runs with one rank: without a communicator (the local result is the answer) and with
VDB_CTX_FORCE_RCCL=1, where both phases are real 1-rank ncclAllGather calls and the device merge runs with S = 1 (ROWS layout) or the
block is copied out of the receive buffer (REPLICA layout).  Expected answers come from the oracle -- oracle.flat_knn_batch(base, qs,
k = len) cut after the last pair with distance <= r, then after `limit` -- bit for bit; equality with GpuIndex.range_search is asserted in
addition.  The call with more queries than one exchange chunk holds (2048) derives its expectation from the oracle's top-64 lists: with
the radius at the 10th distance and the 64th distance asserted to lie outside it, the pairs inside the radius are a prefix of that list.

More than one rank on the one GPU: under VDB_CTX_LOOPBACK=1 the context takes device 0 three or eight times and exchanges with device
copies (modes loop3, loop8; the 40000x96 table only).  Phase 1 with short and empty replica blocks padded, phase 2 at the largest rank
total, k_range_merge over S received blocks (ROWS), the concatenation of the blocks in query order (REPLICA), the status words of a rank
whose local search failed and the merged-total check against the smallest ceiling then run with S > 1 -- same oracle, same equality."""
import numpy as np
import pytest

from conftest import gist_like

pytestmark = pytest.mark.gpu

TABLES = {"40000x96": (40000, 96, 91, 92), "30000x960": (30000, 960, 1806, 1807)}
ROWS_MODES = [("rows", m) for m in ("nocomm", "comm_all", "comm_rank")]
REPLICA_MODES = [("replica", m) for m in ("nocomm", "comm_all")]
LOOP_MODES = [(layout, m) for layout in ("rows", "replica") for m in ("loop3", "loop8")]  # S = 3, S = 8 through the loopback exchange
NQ_CHUNKED = 2500  # more than one exchange chunk (2048 queries)


def _full_order(base, qs, kind=0):
    from oracle import oracle as O

    oi, od, oc = O.flat_knn_batch(base, qs, len(base), kind, nthreads=16)
    assert (oc == len(base)).all()
    return oi.astype(np.uint64), od


def _expect(full, radii, limit=None):
    oi, od = full
    lims, ids, ds = [0], [], []
    for q in range(len(oi)):
        with np.errstate(invalid="ignore"):
            inside = od[q] <= np.float32(radii[q])  # NaN distance / NaN radius: False
        cut = int(inside.sum())
        assert inside[:cut].all()  # sorted ascending, NaN last: the pairs inside are a prefix
        if limit is not None:
            cut = min(cut, limit)
        ids.append(oi[q, :cut])
        ds.append(od[q, :cut])
        lims.append(lims[-1] + cut)
    return np.array(lims, dtype=np.uint64), np.concatenate(ids), np.concatenate(ds)


def _same(got, exp, what=""):
    gl, gi, gd = got
    el, ei, ed = exp
    assert np.array_equal(gl, el), (what, gl, el)
    assert gi.dtype == np.uint64 and np.array_equal(gi, ei), what
    assert gd.dtype == np.float32 and np.array_equal(gd.view(np.uint32), ed.astype(np.float32).view(np.uint32)), what


def _kth(full, k):
    return full[1][:, k - 1].copy()


def _below(r):
    return np.nextafter(r.astype(np.float32), np.float32(-np.inf))


def _radius_cases(full):
    nq = len(full[0])
    cases = {"kth10": _kth(full, 10), "below10": _below(_kth(full, 10)), "kth64": _kth(full, 64), "below1": _below(_kth(full, 1)),
             "nan": np.full(nq, np.nan, dtype=np.float32)}
    mixed = _kth(full, 10)
    mixed[1::4] = np.inf
    mixed[2::4] = np.nan
    mixed[3::8] = _kth(full, 64)[3::8]
    cases["mixed"] = mixed
    return cases


@pytest.fixture(scope="module")
def tables():
    out = {}
    for name, (n, dim, s_base, s_q) in TABLES.items():
        base = gist_like(n, dim=dim, seed=s_base)
        base[n // 2:n // 2 + 10] = base[:10]  # exact distance ties
        qs = gist_like(24, dim=dim, seed=s_q)
        out[name] = (base, qs, _full_order(base, qs))
    return out


@pytest.fixture(scope="module")
def chunked(tables):
    """the call with more queries than one exchange chunk, on the 40000x96 table: queries, the oracle's top-64 lists, the radii"""
    from oracle import oracle as O

    base = tables["40000x96"][0]
    many = gist_like(NQ_CHUNKED, dim=base.shape[1], seed=93)
    oi, od, oc = O.flat_knn_batch(base, many, 64, 0, nthreads=16)
    assert (oc == 64).all()
    top = (oi.astype(np.uint64), od)
    r = _kth(top, 10)
    assert (od[:, 63] > r).all()  # the 64th pair is outside: the pairs inside the radius are a prefix of the top-64
    return many, top, r


def _loop_shards(mode):
    return int(mode[4:]) if mode.startswith("loop") else 0


def _make(layout, mode, dim, monkeypatch):
    from lab_1806_vec_db_amd.sharded import ShardedIndex

    S = _loop_shards(mode)
    if S:
        monkeypatch.setenv("VDB_CTX_LOOPBACK", "1")
        monkeypatch.delenv("VDB_CTX_FORCE_RCCL", raising=False)
        sh = ShardedIndex(dim, "l2sqr", devices=[0] * S)
        assert sh.info() == {"world": S, "n_local": S, "first_rank": 0, "has_comm": False}
        return sh
    if mode != "nocomm":
        monkeypatch.setenv("VDB_CTX_FORCE_RCCL", "1")
    if mode == "comm_rank":
        sh = ShardedIndex(dim, "l2sqr", device=0, rank=0, world=1, uid=ShardedIndex.unique_id())
    else:
        sh = ShardedIndex(dim, "l2sqr", devices=[0])
    info = sh.info()
    assert info["world"] == 1 and info["n_local"] == 1 and info["has_comm"] == (mode != "nocomm")
    return sh


@pytest.mark.parametrize("table", list(TABLES))
@pytest.mark.parametrize("layout,mode", ROWS_MODES + REPLICA_MODES)
def test_sharded_range_search_one_gpu(tables, chunked, table, layout, mode, monkeypatch):
    _range_search_cases(tables, chunked, table, layout, mode, monkeypatch)


@pytest.mark.parametrize("layout,mode", LOOP_MODES)
def test_sharded_range_search_many_shards(tables, chunked, layout, mode, monkeypatch):
    _range_search_cases(tables, chunked, "40000x96", layout, mode, monkeypatch)


def _range_search_cases(tables, chunked, table, layout, mode, monkeypatch):
    import lab_1806_vec_db_amd as vdb

    base, qs, full = tables[table]
    n, dim = base.shape
    sh = _make(layout, mode, dim, monkeypatch)
    ref = vdb.GpuIndex(dim, "l2sqr")
    try:
        # no rows yet: empty results, like an empty index
        lims, idx, dist = sh.range_search(qs[:5], 1.0)
        assert lims.tolist() == [0] * 6 and len(idx) == 0 and len(dist) == 0
        (sh.set_rows if layout == "rows" else sh.set_rows_replica)(base)
        assert sh.layout == layout and len(sh) == n
        ref.batch_add(base)
        cases = _radius_cases(full)
        for name, limit in [(c, None) for c in cases] + [("kth64", 10), ("mixed", 10), ("mixed", 1)]:
            got = sh.range_search(qs, cases[name], limit)
            _same(got, _expect(full, cases[name], limit), (table, layout, mode, name, limit, "oracle"))
            _same(got, ref.range_search(qs, cases[name], limit), (table, layout, mode, name, limit, "plain index"))
        # a scalar radius, one query
        r = float(np.median(_kth(full, 10)))
        _same(sh.range_search(qs, r), _expect(full, np.full(len(qs), r, np.float32)), "scalar radius")
        _same(sh.range_search(qs[3], _kth(full, 10)[3]), _expect((full[0][3:4], full[1][3:4]), _kth(full, 10)[3:4]), "one query")
        # nq = 0
        lims, idx, dist = sh.range_search(np.zeros((0, dim), dtype=np.float32), 1.0)
        assert lims.tolist() == [0] and len(idx) == 0 and len(dist) == 0
        # a dim mismatch raises; limit <= 0 is the caller's mistake
        with pytest.raises(vdb.VdbError, match="dimension mismatch"):
            sh.range_search(np.zeros((2, dim + 1), dtype=np.float32), 1.0)
        with pytest.raises(ValueError):
            sh.range_search(qs, 1.0, limit=0)
        # the local index's ceiling: an ordinary error, no poison, and the next (smaller) call succeeds
        loc = sh.local_index(0)
        loc.set_param("flat_range_max_results", 100)
        with pytest.raises(vdb.VdbError, match="flat_range_max_results"):
            sh.range_search(qs, cases["kth64"])  # 24 x >= 64 pairs
        assert not sh.poisoned
        _same(sh.range_search(qs, cases["below1"]), _expect(full, cases["below1"]), "after the failed call")
        _same(sh.range_search(qs[:5], cases["kth10"][:5]), _expect((full[0][:5], full[1][:5]), cases["kth10"][:5]), "after the failed call")
        loc.set_param("flat_range_max_results", 0)
        _same(sh.range_search(qs, cases["kth64"]), _expect(full, cases["kth64"]), "ceiling lifted")
        if table == "30000x960":
            assert sh.local_stat(0, "flat_range_i8_queries") > 0  # the tier answered, not only the scan
            sh.local_index(0).set_flat_mode(1)  # vdb_flat_set_mode of the local index applies
            s0 = sh.local_stat(0, "flat_range_scan_queries")
            _same(sh.range_search(qs, cases["kth10"]), _expect(full, cases["kth10"]), "scan mode")
            assert sh.local_stat(0, "flat_range_scan_queries") - s0 == len(qs)
        else:
            # more queries in one call than one exchange chunk holds
            many, top, r = chunked
            for limit in (None, 4):
                got = sh.range_search(many, r, limit)
                _same(got, _expect(top, r, limit), (layout, mode, "chunked", limit, "oracle"))
                _same(got, ref.range_search(many, r, limit), (layout, mode, "chunked", limit, "plain index"))
    finally:
        ref.close()
        sh.close()


@pytest.mark.parametrize("layout", ["rows", "replica"])
def test_sharded_range_on_an_index_with_zero_rows(layout):
    from lab_1806_vec_db_amd.sharded import ShardedIndex

    sh = ShardedIndex(16, "cosine", devices=[0])
    try:
        (sh.set_rows if layout == "rows" else sh.set_rows_replica)(np.zeros((0, 16), dtype=np.float32))
        lims, idx, dist = sh.range_search(np.ones((7, 16), dtype=np.float32), np.inf)
        assert lims.tolist() == [0] * 8 and len(idx) == 0 and len(dist) == 0
        assert not sh.poisoned
    finally:
        sh.close()


def _rank_totals(layout, S, n, exp):
    """pairs every rank holds of the expected answer `exp` (no limit): ROWS -- the ids of its row block; REPLICA -- its query block"""
    lims, ids, _ = exp
    nq = len(lims) - 1
    if layout == "rows":
        per = -(-n // S)
        return [int(((ids >= r * per) & (ids < (r + 1) * per)).sum()) for r in range(S)]
    per = -(-nq // S)
    return [int(lims[min(nq, (r + 1) * per)] - lims[min(nq, r * per)]) for r in range(S)]


@pytest.mark.parametrize("layout", ["rows", "replica"])
def test_sharded_range_ceilings_with_three_ranks(tables, layout, monkeypatch):
    """S = 3: (a) the ceiling of ONE rank's local search -- its status word reaches every rank in phase 1, the error names that rank;
    (b) every rank within its own ceiling but the merged (ROWS) / concatenated (REPLICA) total above the smallest one -- the check
    between the phases.  Both fail without poisoning the object, and the next call is correct."""
    import lab_1806_vec_db_amd as vdb

    base, qs, full = tables["40000x96"]
    n, dim = base.shape
    cases = _radius_cases(full)
    sh = _make(layout, "loop3", dim, monkeypatch)
    try:
        (sh.set_rows if layout == "rows" else sh.set_rows_replica)(base)
        exp64 = _expect(full, cases["kth64"])
        totals = _rank_totals(layout, 3, n, exp64)
        merged = int(exp64[0][-1])
        assert sum(totals) == merged and min(totals) > 0

        def small_calls(what):
            assert not sh.poisoned
            _same(sh.range_search(qs, cases["below1"]), _expect(full, cases["below1"]), what)
            _same(sh.range_search(qs[:2], cases["kth10"][:2]), _expect((full[0][:2], full[1][:2]), cases["kth10"][:2]), what)

        # (a) rank 1 alone has a ceiling, below its share of the answer
        small = 40
        assert totals[1] > small >= int(_expect((full[0][:2], full[1][:2]), cases["kth10"][:2])[0][-1])
        sh.local_index(1).set_param("flat_range_max_results", small)
        with pytest.raises(vdb.VdbError, match=r"failed on rank 1; rank 1: .*flat_range_max_results"):
            sh.range_search(qs, cases["kth64"])
        small_calls("after rank 1's ceiling")
        sh.local_index(1).set_param("flat_range_max_results", 0)
        _same(sh.range_search(qs, cases["kth64"]), exp64, "ceiling lifted")
        # (b) a ceiling every rank's own total passes, set on the last rank only: the smallest one bounds the merged total
        ceiling = (max(totals) + merged) // 2
        assert max(totals) < ceiling < merged
        sh.local_index(2).set_param("flat_range_max_results", ceiling)
        with pytest.raises(vdb.VdbError, match=rf"{merged} results for a chunk of {len(qs)} queries, more than {ceiling} "):
            sh.range_search(qs, cases["kth64"])
        small_calls("after the merged-total check")
        sh.local_index(2).set_param("flat_range_max_results", merged)  # exactly the total: allowed
        _same(sh.range_search(qs, cases["kth64"]), exp64, "ceiling == total")
    finally:
        sh.close()
