"""GPU: exact Flat range search (GpuIndex.range_search / vdb_flat_range) against the CPU oracle.

The expected answer of a query is derived from the oracle as it stands: oracle.flat_knn(base, q, k = len) -- every row in the
reference's (distance, index) order -- cut after the last pair with distance <= r (with a limit: its first `limit` pairs).  Every
case is bit-exact: ids equal, distances equal as f32 bit patterns, CSR offsets equal.  Tables of 30 000 rows run the 8-bit tier
(mode 2) and the strict-order scan (mode 1), which must agree with each other too; the 1000-row golden table takes the scan."""
import threading

import numpy as np
import pytest

from conftest import gist_like

pytestmark = pytest.mark.gpu

DISTS = (("l2sqr", 0), ("cosine", 1))
CAND_CAP = 8192
STATS = ("flat_range_queries", "flat_range_i8_queries", "flat_range_scan_queries", "flat_range_hits", "flat_range_results")


def _full_order(base, qs, kind):
    """(ids, distances) of every row per query in the reference's order (NaN distances last)"""
    from oracle import oracle as O

    oi, od, oc = O.flat_knn_batch(base, qs, len(base), kind, nthreads=16)
    assert (oc == len(base)).all()
    return oi.astype(np.uint64), od


def _expect(full, radii, limit=None, id_offset=0):
    oi, od = full
    lims, ids, ds = [0], [], []
    for q in range(len(oi)):
        with np.errstate(invalid="ignore"):
            inside = od[q] <= np.float32(radii[q])  # NaN distance / NaN radius: False
        cut = int(inside.sum())
        assert inside[:cut].all()  # sorted ascending, NaN last: the pairs inside are a prefix
        if limit is not None:
            cut = min(cut, limit)
        ids.append(oi[q, :cut] + np.uint64(id_offset))
        ds.append(od[q, :cut])
        lims.append(lims[-1] + cut)
    return np.array(lims, dtype=np.uint64), np.concatenate(ids), np.concatenate(ds)


def _same(got, exp, what=""):
    gl, gi, gd = got
    el, ei, ed = exp
    assert np.array_equal(gl, el), (what, gl, el)
    assert np.array_equal(gi, ei), what
    assert gd.dtype == np.float32 and np.array_equal(gd.view(np.uint32), ed.astype(np.float32).view(np.uint32)), what


def _stats(ix):
    return {s: ix.get_stat(s) for s in STATS}


def _kth(full, k):
    return full[1][:, k - 1].copy()


def _below(r):
    return np.nextafter(r.astype(np.float32), np.float32(-np.inf))


@pytest.fixture(scope="module")
def big():
    """30 000 x 960 gist-like rows, 24 queries, with both metrics' full orders"""
    base = gist_like(30000, seed=1806)
    qs = gist_like(24, seed=1807)
    return base, qs, {kind: _full_order(base, qs, kind) for _, kind in DISTS}


def _index(dist, base, mode=None, **kw):
    import lab_1806_vec_db_amd as vdb

    ix = vdb.GpuIndex(base.shape[1], dist, **kw)
    ix.batch_add(base)
    if mode is not None:
        ix.set_flat_mode(mode)
    return ix


def _radius_cases(full):
    nq = len(full[0])
    cases = {}
    for k in (1, 10, 64):
        cases[f"kth{k}"] = _kth(full, k)             # boundary row included: top-k plus ties
        cases[f"below{k}"] = _below(_kth(full, k))   # boundary row excluded
    cases["nan"] = np.full(nq, np.nan, dtype=np.float32)
    mixed = _kth(full, 10)
    mixed[1::4] = np.inf
    mixed[2::4] = np.nan
    mixed[3::8] = _kth(full, 64)[3::8]
    cases["mixed"] = mixed
    return cases


@pytest.mark.parametrize("dist,kind", DISTS)
def test_golden_table_scan_tier(gist_base, gist_test, dist, kind):
    qs = gist_test[:32]
    full = _full_order(gist_base, qs, kind)
    ix = _index(dist, gist_base)
    try:
        cases = _radius_cases(full)
        cases["inf"] = np.full(len(qs), np.inf, dtype=np.float32)  # all len rows = flat_knn(k = len)
        for name, r in cases.items():
            s0 = _stats(ix)
            got = ix.range_search(qs, r)
            exp = _expect(full, r)
            _same(got, exp, (dist, name))
            s1 = _stats(ix)
            assert s1["flat_range_queries"] - s0["flat_range_queries"] == len(qs)
            assert s1["flat_range_scan_queries"] - s0["flat_range_scan_queries"] == len(qs)  # 1000 rows: below the tier's tables
            assert s1["flat_range_i8_queries"] == s0["flat_range_i8_queries"]
            assert s1["flat_range_results"] - s0["flat_range_results"] == int(exp[0][-1])
        assert int(_expect(full, cases["inf"])[0][-1]) == len(qs) * len(gist_base)
        # one radius for all queries; one query
        r = float(np.median(_kth(full, 10)))
        _same(ix.range_search(qs, r), _expect(full, np.full(len(qs), r, np.float32)), "scalar radius")
        one = ix.range_search(qs[3], _kth(full, 10)[3])
        _same(one, _expect((full[0][3:4], full[1][3:4]), _kth(full, 10)[3:4]), "one query")
        # forced mode on this small table: whichever tier answers, the answer is the same
        ix.set_flat_mode(2)
        for name in ("kth10", "below64", "mixed"):
            _same(ix.range_search(qs, cases[name]), _expect(full, cases[name]), ("forced tier on 1000 rows", name))
    finally:
        ix.close()


@pytest.mark.parametrize("dist,kind", DISTS)
def test_tier_and_scan_agree_with_oracle(big, dist, kind):
    base, qs, fulls = big
    full = fulls[kind]
    tier, scan = _index(dist, base, 2), _index(dist, base, 1)
    try:
        for name, r in _radius_cases(full).items():
            exp = _expect(full, r)
            s0 = _stats(tier)
            got_t = tier.range_search(qs, r)
            s1 = _stats(tier)
            got_s = scan.range_search(qs, r)
            _same(got_t, exp, (dist, name, "tier"))
            _same(got_s, exp, (dist, name, "scan"))
            _same(got_t, got_s, (dist, name, "tier vs scan"))
            d = {s: s1[s] - s0[s] for s in STATS}
            print(dist, name, d)
            assert d["flat_range_queries"] == len(qs) and d["flat_range_i8_queries"] + d["flat_range_scan_queries"] == len(qs)
            assert d["flat_range_results"] == int(exp[0][-1])
            finite = int(np.isfinite(r).sum())
            if name == "nan":
                assert d["flat_range_i8_queries"] == 0
            else:  # per-query routing: the finite radii stay in the tier, +inf / NaN leave it
                assert d["flat_range_i8_queries"] == finite, (dist, name, d)
                # every pair the tier returned was a hit
                assert d["flat_range_hits"] >= int(_expect(full, np.where(np.isfinite(r), r, np.nan))[0][-1])
        assert scan.get_stat("flat_range_i8_queries") == 0
        # k-NN counters: range calls neither read nor write them
        assert tier.get_stat("flat_i8_queries") == 0 and tier.get_stat("flat_i8_redo") == 0
        # +inf: every row, in flat_knn(k = len) order (two queries: 60 000 pairs)
        r = np.full(2, np.inf, dtype=np.float32)
        f2 = (full[0][:2], full[1][:2])
        _same(tier.range_search(qs[:2], r), _expect(f2, r), "inf")
        # auto mode: a table of 30 000 rows takes the tier
        tier.set_flat_mode(0)
        s0 = _stats(tier)
        _same(tier.range_search(qs, _kth(full, 10)), _expect(full, _kth(full, 10)), "auto")
        assert _stats(tier)["flat_range_i8_queries"] - s0["flat_range_i8_queries"] == len(qs)
    finally:
        tier.close()
        scan.close()


@pytest.mark.parametrize("dist,kind", DISTS)
def test_overflowing_query_goes_to_scan(big, dist, kind):
    """radius at the table's median distance: ~15 000 rows inside, more than the 8192-slot hit lists hold"""
    base, qs, fulls = big
    full = (fulls[kind][0][:4], fulls[kind][1][:4])
    r = full[1][:, len(base) // 2].copy()
    r[3] = _kth(full, 10)[3]  # ... next to one that fits
    exp = _expect(full, r)
    assert int(exp[0][1]) > CAND_CAP
    ix = _index(dist, base, 2)
    try:
        got = ix.range_search(qs[:4], r)
        _same(got, exp, dist)
        st = _stats(ix)
        assert st["flat_range_scan_queries"] == 3 and st["flat_range_i8_queries"] == 1
    finally:
        ix.close()


@pytest.mark.parametrize("dist,kind", DISTS)
def test_self_queries_duplicates_and_ties(dist, kind):
    base = gist_like(20000, dim=128, seed=11)
    base[100:110] = base[7]          # duplicates of row 7
    base[15000] = base[19999]        # ... and of the last row
    rows = [7, 105, 19999, 3, 12345]
    qs = base[rows].copy()
    full = _full_order(base, qs, kind)
    r0 = np.zeros(len(rows), dtype=np.float32) if kind == 0 else full[1][:, 0].copy()
    exp = _expect(full, r0)
    if kind == 0:  # the row itself at distance exactly 0, plus its duplicates
        assert (exp[2] == 0.0).all()
    assert exp[1][:11].tolist() == [7] + list(range(100, 110)) and [int(x) for x in np.diff(exp[0])][:3] == [11, 11, 2]
    # the 11th distance: for the duplicated rows still the tie at the smallest distance, for the others a boundary of their own
    r_tie = full[1][:, 10].copy()
    for mode in (2, 1):
        ix = _index(dist, base, mode)
        try:
            _same(ix.range_search(qs, r0), exp, (dist, mode, "r = d0"))
            _same(ix.range_search(qs, r_tie), _expect(full, r_tie), (dist, mode, "ties"))
            _same(ix.range_search(qs, _below(r_tie)), _expect(full, _below(r_tie)), (dist, mode, "below ties"))
            if mode == 2:
                assert ix.get_stat("flat_range_i8_queries") > 0
        finally:
            ix.close()


@pytest.mark.parametrize("dist,kind", DISTS)
def test_rows_with_nan_and_inf(dist, kind):
    base = gist_like(20000, dim=128, seed=12)
    base[5, 3] = np.nan
    base[17000, 0] = np.inf
    base[17001, 9] = -np.inf
    base[9, :] = 0.0  # a zero row (Cosine: the clamp)
    qs = gist_like(8, dim=128, seed=13)
    full = _full_order(base, qs, kind)
    for name, r in (("kth10", _kth(full, 10)), ("kth64", _kth(full, 64)), ("huge", np.full(8, 3.0e38, np.float32))):
        exp = _expect(full, r)
        for mode in (2, 1):
            ix = _index(dist, base, mode)
            try:
                _same(ix.range_search(qs, r), exp, (dist, name, mode))
            finally:
                ix.close()
    # +inf keeps the +inf distances and drops the NaN ones
    r = np.full(2, np.inf, dtype=np.float32)
    ix = _index(dist, base, 2)
    try:
        got = ix.range_search(qs[:2], r)
        _same(got, _expect((full[0][:2], full[1][:2]), r), "inf radius")
        assert not np.isnan(got[2]).any() and int(got[0][1]) < len(base)
    finally:
        ix.close()


def test_limit_offset_mutation_and_edges(big):
    import lab_1806_vec_db_amd as vdb

    base, qs, fulls = big
    full = fulls[0]
    ix = _index("l2sqr", base, 2)
    scan = _index("l2sqr", base, 1)
    try:
        r = _kth(full, 64)
        for limit in (1, 10, 64, 100):  # = flat_knn(k = limit) cut at r
            exp = _expect(full, r, limit=limit)
            _same(ix.range_search(qs, r, limit=limit), exp, ("limit", limit))
            _same(scan.range_search(qs, r, limit=limit), exp, ("limit scan", limit))
            gi, gd, gc = ix.flat_knn(qs, limit)
            for q in range(len(qs)):
                keep = gd[q] <= r[q]
                assert np.array_equal(exp[1][exp[0][q]:exp[0][q + 1]], gi[q][keep])
        with pytest.raises(ValueError):
            ix.range_search(qs, r, limit=0)
        # a ceiling on the result size: an error of the call, the handle stays usable
        total = int(_expect(full, r)[0][-1])
        for x in (ix, scan):
            x.set_param("flat_range_max_results", total - 1)
            with pytest.raises(vdb.VdbError, match="flat_range_max_results"):
                x.range_search(qs, r)
            _same(x.range_search(qs, r, limit=10), _expect(full, r, limit=10), "limit under the ceiling")
            x.set_param("flat_range_max_results", total)
            _same(x.range_search(qs, r), _expect(full, r), "at the ceiling")
            x.set_param("flat_range_max_results", 0)
        # id_offset
        ix.set_id_offset(1 << 33)
        _same(ix.range_search(qs, r), _expect(full, r, id_offset=1 << 33), "id_offset")
        ix.set_id_offset(0)
        # nq = 0, dim mismatch
        l0, i0, d0 = ix.range_search(np.zeros((0, 960), np.float32), np.zeros(0, np.float32))
        assert l0.tolist() == [0] and len(i0) == 0 and len(d0) == 0
        with pytest.raises(vdb.VdbError, match="dimension"):
            ix.range_search(np.zeros((2, 64), np.float32), 1.0)
        # swap_remove / add between calls: the mirrors follow
        cur = base.copy()
        for i in (int(full[0][0, 0]), 17, None):  # a query's nearest row, an early row, the last row
            i = len(cur) - 1 if i is None else i
            ix.swap_remove(i)
            scan.swap_remove(i)
            cur[i] = cur[-1]
            cur = cur[:-1]
        f2 = _full_order(cur, qs[:8], 0)
        r2 = _kth(f2, 10)
        _same(ix.range_search(qs[:8], r2), _expect(f2, r2), "after swap_remove")
        _same(scan.range_search(qs[:8], r2), _expect(f2, r2), "after swap_remove, scan")
        extra = np.concatenate([qs[:3], gist_like(40, seed=99)])  # three queries become rows: distance 0
        ix.batch_add(extra)
        cur = np.concatenate([cur, extra])
        f3 = _full_order(cur, qs[:8], 0)
        r3 = _kth(f3, 10)
        s0 = _stats(ix)
        got = ix.range_search(qs[:8], r3)
        _same(got, _expect(f3, r3), "after add")
        assert _stats(ix)["flat_range_i8_queries"] - s0["flat_range_i8_queries"] == 8
        assert got[2][0] == 0.0 and int(got[1][0]) == len(cur) - len(extra)
    finally:
        ix.close()
        scan.close()
    # empty index
    e = vdb.GpuIndex(960, "cosine")
    l0, i0, d0 = e.range_search(qs[:3], np.inf)
    assert l0.tolist() == [0, 0, 0, 0] and len(i0) == 0 and len(d0) == 0
    e.close()


@pytest.mark.parametrize("dist,kind", DISTS)
def test_u8_index_equals_widened_f32_index(dist, kind):
    import lab_1806_vec_db_amd as vdb

    rng = np.random.Generator(np.random.PCG64(8))
    rows = rng.integers(0, 256, (20000, 128), dtype=np.uint8)
    rows[40:44] = rows[3]
    qs = rng.integers(0, 256, (9, 128), dtype=np.uint8).astype(np.float32)
    qs[0] = rows[3]
    wide = rows.astype(np.float32)
    full = _full_order(wide, qs, kind)
    u8 = vdb.GpuIndex(128, dist, scalar="u8")
    u8.batch_add_u8(rows)
    f32 = _index(dist, wide, 2)
    try:
        for r in (_kth(full, 1), _kth(full, 10), _below(_kth(full, 64))):
            exp = _expect(full, r)
            s0 = _stats(u8)
            got = u8.range_search(qs, r)
            _same(got, exp, (dist, "u8"))
            assert _stats(u8)["flat_range_scan_queries"] - s0["flat_range_scan_queries"] == len(qs)  # u8 rows: the scan
            _same(f32.range_search(qs, r), got, (dist, "u8 vs f32"))
    finally:
        u8.close()
        f32.close()


@pytest.mark.parametrize("dim", (66, 64, 1000))
def test_dimensions_outside_the_tier(dim):
    """dim % 4 != 0 and a single 64-column block (no 8-bit pass: the scan answers), and 1000 columns (padded to 1024: the tier):
    whatever the 8-bit pass says about the shape, forced mode answers exactly"""
    base = gist_like(17000, dim=dim, seed=21)
    qs = gist_like(5, dim=dim, seed=22)
    full = _full_order(base, qs, 0)
    ix = _index("l2sqr", base, 2)
    try:
        for r in (_kth(full, 10), _below(_kth(full, 10))):
            _same(ix.range_search(qs, r), _expect(full, r), dim)
        st = _stats(ix)
        if dim in (66, 64):
            assert st["flat_range_i8_queries"] == 0 and st["flat_range_scan_queries"] == 10
    finally:
        ix.close()


def test_two_threads_range_and_knn_on_one_handle(big):
    base, qs, fulls = big
    full = fulls[0]
    ix = _index("l2sqr", base, 0)
    try:
        ix.set_param("flat_i8", 2)  # every k-NN call counts in flat_i8_queries, whatever the auto rule has seen
        radii = [_kth(full, 10), _kth(full, 64), _below(_kth(full, 1))]
        want_r = [ix.range_search(qs, r) for r in radii]
        for w, r in zip(want_r, radii):
            _same(w, _expect(full, r), "single thread")
        assert ix.get_stat("flat_i8_queries") == 0 and ix.get_stat("flat_i8_redo") == 0  # range calls do not move them
        want_k = [ix.flat_knn(qs, k) for k in (10, 33)]
        q1, r1 = ix.get_stat("flat_i8_queries"), ix.get_stat("flat_i8_redo")
        assert q1 == 2 * len(qs)
        rounds, errs = 6, []

        def ranger():
            try:
                for _ in range(rounds):
                    for w, r in zip(want_r, radii):
                        _same(ix.range_search(qs, r), w, "threaded range")
            except BaseException as e:  # noqa: BLE001
                errs.append(e)

        def knner():
            try:
                for _ in range(rounds):
                    for (wi, wd, wc), k in zip(want_k, (10, 33)):
                        gi, gd, gc = ix.flat_knn(qs, k)
                        assert np.array_equal(gi, wi) and np.array_equal(gd, wd) and np.array_equal(gc, wc)
            except BaseException as e:  # noqa: BLE001
                errs.append(e)

        ts = [threading.Thread(target=ranger), threading.Thread(target=knner)]
        for t in ts:
            t.start()
        for t in ts:
            t.join()
        assert not errs, errs
        # the k-NN tier's counters moved by the k-NN calls alone
        assert ix.get_stat("flat_i8_queries") == q1 + rounds * 2 * len(qs)
        assert ix.get_stat("flat_i8_redo") == r1 + rounds * r1
        assert ix.get_stat("flat_range_queries") == (1 + rounds) * len(radii) * len(qs)
    finally:
        ix.close()


def test_device_entry_point(big):
    import torch

    base, qs, fulls = big
    full = fulls[1]
    ix = _index("cosine", base, 2)
    try:
        r = _kth(full, 10)
        dq = torch.from_numpy(qs).cuda()
        dr = torch.from_numpy(r).cuda()
        torch.cuda.synchronize()
        _same(ix.range_search_device(dq.data_ptr(), len(qs), dr.data_ptr()), _expect(full, r), "device")
        _same(ix.range_search_device(dq.data_ptr(), len(qs), dr.data_ptr(), limit=3), _expect(full, r, limit=3), "device, limit")
    finally:
        ix.close()


def test_many_queries_cross_the_tier_rounds():
    """more queries than one round of the tier takes (1024): rounds, pool growth, offsets"""
    base = gist_like(17000, dim=128, seed=31)
    qs = gist_like(1100, dim=128, seed=32)
    ix, scan = _index("l2sqr", base, 2), _index("l2sqr", base, 1)
    try:
        gi, gd, _ = scan.flat_knn(qs, 5)
        r = gd[:, 4].copy()
        r[::7] = np.nan
        got = ix.range_search(qs, r)
        lims = got[0]
        for q in range(len(qs)):
            a, b = int(lims[q]), int(lims[q + 1])
            if np.isnan(r[q]):
                assert a == b
            else:
                assert b - a >= 5 and np.array_equal(got[1][a:a + 5], gi[q]) and np.array_equal(got[2][a:a + 5], gd[q])
                assert (got[2][a:b] <= r[q]).all()
        _same(got, scan.range_search(qs, r), "1100 queries: tier vs scan")
        assert ix.get_stat("flat_range_i8_queries") == int((~np.isnan(r)).sum())
    finally:
        ix.close()
        scan.close()
