"""GPU: the device merge of range results (GpuIndex.range_merge_device / vdb_range_merge_device, k_range_merge.hip).

One GPU stands in for S: a 40 000 x 960 gist-like table is split by shard_bounds into S GpuIndex objects with set_id_offset, their
range_search results are packed into device tensors the way phase 2 of the exchange delivers them ([S][stride] ids / distances, [S][nq + 1]
offsets) and merged on the device.  The expected answer is the oracle's UNSHARDED one -- oracle.flat_knn_batch(base, qs, k = len) cut after the
last pair with distance <= r, then after `limit` -- and every comparison is bit-exact (offsets, ids, distance bit patterns).  The host
utility range_merge must give the same on the same input."""
import numpy as np
import pytest

from conftest import gist_like

pytestmark = pytest.mark.gpu

DISTS = (("l2sqr", 0), ("cosine", 1))
N = 40000


def _full_order(base, qs, kind):
    """(ids, distances) of every row per query in the reference's order (NaN distances last)"""
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


@pytest.fixture(scope="module")
def table():
    base = gist_like(N, seed=1806)
    qs = gist_like(24, seed=1807)
    return base, qs, {kind: _full_order(base, qs, kind) for _, kind in DISTS}


def _shards(dist, base, bounds, mode):
    import lab_1806_vec_db_amd as vdb

    out = []
    for r0, r1 in bounds:
        ix = vdb.GpuIndex(base.shape[1], dist)
        if r1 > r0:
            ix.batch_add(base[r0:r1])
        ix.set_id_offset(r0)
        ix.set_flat_mode(mode)
        out.append(ix)
    return out


def _merge_both(shards, qs, radii, limit):
    """every shard's range_search, packed as phase 2 delivers it, merged on the device and by the host utility"""
    import torch

    import lab_1806_vec_db_amd as vdb

    S, nq = len(shards), len(qs)
    res = [ix.range_search(qs, radii, limit) for ix in shards]
    stride = max(max(int(r[0][nq]) for r in res), 1)
    lims = np.stack([r[0] for r in res])
    ids = np.zeros((S, stride), dtype=np.uint64)
    ds = np.zeros((S, stride), dtype=np.float32)
    for s, (l, i, d) in enumerate(res):
        ids[s, :len(i)] = i
        ds[s, :len(d)] = d
    d_lims = torch.from_numpy(lims.view(np.int64)).cuda()
    d_ids = torch.from_numpy(ids.view(np.int64)).cuda()
    d_ds = torch.from_numpy(ds).cuda()
    torch.cuda.synchronize()
    dev = shards[0].range_merge_device(d_lims.data_ptr(), d_ids.data_ptr(), d_ds.data_ptr(), S, nq, stride, limit)
    host = vdb.range_merge(lims, ids, ds, limit)
    return dev, host, res


@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("S", [2, 3, 8])
@pytest.mark.parametrize("dist,kind", DISTS)
def test_device_merge_of_shards_equals_unsharded_oracle(table, dist, kind, S, mode):
    from lab_1806_vec_db_amd.shard import shard_bounds

    base, qs, fulls = table
    full = fulls[kind]
    shards = _shards(dist, base, [shard_bounds(N, S, r) for r in range(S)], mode)
    try:
        cases = _radius_cases(full)
        plan = [(name, None) for name in cases] + [(name, limit) for name in ("kth64", "mixed") for limit in (1, 10, 1000)]
        for name, limit in plan:
            dev, host, res = _merge_both(shards, qs, cases[name], limit)
            exp = _expect(full, cases[name], limit)
            _same(dev, exp, (dist, S, mode, name, limit, "device merge vs oracle"))
            _same(host, exp, (dist, S, mode, name, limit, "host merge vs oracle"))
            _same(dev, host, (dist, S, mode, name, limit, "device vs host"))
            assert sum(int(r[0][-1]) for r in res) >= int(exp[0][-1])
        if mode == 2 and S == 2:  # 20 000 rows per shard: above the 8-bit tier's 16 384
            for ix in shards:
                assert ix.get_stat("flat_range_i8_queries") > 0
    finally:
        for ix in shards:
            ix.close()


def test_long_lists_take_the_global_memory_path(table):
    """radius = the 20 000th distance: 240 KB of pairs per query, more than a workgroup's LDS -- the slices search in global memory"""
    from lab_1806_vec_db_amd.shard import shard_bounds

    base, qs, fulls = table
    full = (fulls[0][0][:4], fulls[0][1][:4])
    r = _kth(full, 20000)
    shards = _shards("l2sqr", base, [shard_bounds(N, 3, s) for s in range(3)], 0)
    try:
        for limit in (None, 5000, 3):
            dev, host, res = _merge_both(shards, qs[:4], r, limit)
            exp = _expect(full, r, limit)
            if limit is None:
                assert (np.diff(exp[0].astype(np.int64)) >= 20000).all()
            _same(dev, exp, ("long", limit, "device"))
            _same(host, exp, ("long", limit, "host"))
    finally:
        for ix in shards:
            ix.close()


@pytest.mark.parametrize("dist,kind", DISTS)
def test_uneven_split_with_a_tiny_and_an_empty_shard(table, dist, kind):
    """a shard of 40 rows (fewer than a wave), one without rows, ids past 2^32 by id_offset arithmetic left to the caller"""
    base, qs, fulls = table
    full = fulls[kind]
    shards = _shards(dist, base, [(0, 40), (40, 40), (40, 25000), (25000, N)], 0)
    try:
        cases = _radius_cases(full)
        for name, limit in (("kth10", None), ("below64", None), ("mixed", None), ("mixed", 10), ("kth64", 1)):
            dev, host, _ = _merge_both(shards, qs, cases[name], limit)
            exp = _expect(full, cases[name], limit)
            _same(dev, exp, (dist, name, limit, "device"))
            _same(host, exp, (dist, name, limit, "host"))
    finally:
        for ix in shards:
            ix.close()


def test_ids_above_2_pow_32_ties_ceiling_and_bad_lims():
    """synthetic lists straight into the device merge: 64-bit ids, ties across shards, -0.0 / +0.0, the per-index ceiling, inconsistent lims"""
    import torch

    import lab_1806_vec_db_amd as vdb

    ix = vdb.GpuIndex(8, "l2sqr")
    try:
        big = 1 << 40
        lims = np.array([[0, 3, 3, 5], [0, 2, 2, 4], [0, 0, 0, 0]], dtype=np.uint64)
        ids = np.array([[7, big + 1, big + 9, 5, 9], [3, big, 2, 7, 0], [0, 0, 0, 0, 0]], dtype=np.uint64)
        ds = np.array([[1.5, 1.5, 2.0, -0.0, 0.0], [1.5, 1.5, 0.0, -0.0, 0.0], [0, 0, 0, 0, 0]], dtype=np.float32)
        t = [torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a).cuda() for a in (lims, ids, ds)]
        torch.cuda.synchronize()
        ol, oi, od = ix.range_merge_device(t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), 3, 3, 5)
        assert ol.tolist() == [0, 5, 5, 9]
        assert oi.tolist() == [3, 7, big, big + 1, big + 9, 2, 5, 7, 9]
        assert od.view(np.uint32).tolist() == [0x3FC00000] * 4 + [0x40000000, 0, 0x80000000, 0x80000000, 0]
        hl, hi, hd = vdb.range_merge(lims, ids, ds)
        assert np.array_equal(hl, ol) and np.array_equal(hi, oi) and np.array_equal(hd.view(np.uint32), od.view(np.uint32))
        ol, oi, od = ix.range_merge_device(t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), 3, 3, 5, limit=2)
        assert ol.tolist() == [0, 2, 2, 4] and oi.tolist() == [3, 7, 2, 5]
        ix.set_param("flat_range_max_results", 8)
        with pytest.raises(vdb.VdbError, match="flat_range_max_results"):
            ix.range_merge_device(t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), 3, 3, 5)
        ix.set_param("flat_range_max_results", 0)
        for bad in ([[1, 3, 3, 5], [0, 2, 2, 4], [0, 0, 0, 0]], [[0, 3, 2, 5], [0, 2, 2, 4], [0, 0, 0, 0]], [[0, 3, 3, 6], [0, 2, 2, 4], [0, 0, 0, 0]]):
            tb = torch.from_numpy(np.array(bad, dtype=np.int64)).cuda()
            torch.cuda.synchronize()
            with pytest.raises(vdb.VdbError, match="range merge"):
                ix.range_merge_device(tb.data_ptr(), t[1].data_ptr(), t[2].data_ptr(), 3, 3, 5)
        assert ix.range_merge_device(t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), 3, 3, 5)[0].tolist() == [0, 5, 5, 9]
        # one shard: its lims must fit its block like any other's (the call fails before anything is launched)
        one = ix.range_merge_device(t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), 1, 3, 5)
        assert one[0].tolist() == [0, 3, 3, 5] and one[1].tolist() == ids[0].tolist()
        for bad in ([[0, 3, 3, 6]], [[0, 3, 3, 3_000_000]], [[1, 3, 3, 5]], [[0, 3, 2, 5]]):
            tb = torch.from_numpy(np.array(bad, dtype=np.int64)).cuda()
            torch.cuda.synchronize()
            with pytest.raises(vdb.VdbError, match="range merge"):
                ix.range_merge_device(tb.data_ptr(), t[1].data_ptr(), t[2].data_ptr(), 1, 3, 5)
        with pytest.raises(ValueError):
            ix.range_merge_device(t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), 3, 3, 5, limit=0)
    finally:
        ix.close()
