"""GPU: exact filtered Flat k-NN with ONE ROW MASK PER QUERY (GpuIndex.flat_knn_filtered_multi) against the CPU oracle.

The expected answer of query q comes from the oracle as tests/test_flat_filtered_gpu.py derives it: oracle.flat_knn_batch(base, qs,
len(base), kind) -- every row in the reference's (distance, index) order -- keeping the pairs whose id masks[mask_of[q]] allows and
taking the first k.  Every case is bit-exact: ids equal, distances equal as f32 bit patterns, counts min(k, m), slots past the count
zero.  "Equals the loop of per-mask flat_knn_filtered calls" is an additional comparison wherever it is made, never the only one --
except in the property test, which has no oracle by design.

Variants of the grouped kernel (k_scan_gather_grouped) and the case that reaches each:
  float4 fold (dim % 4 == 0), L2 and dot   -- test_grouped_path (dim 960), test_odd_dimensions[100]
  element fold (dim % 4 != 0), L2 and dot  -- test_odd_dimensions[21]
  query groups of nb = 1 .. 8              -- test_grouped_path: buckets of 1, 7, 8, 9 (8 + 1) and 15 (8 + 7); test_odd_dimensions: buckets
                                              of 4 and 5; test_property_multi_equals_loop: random bucket sizes (2, 3, 6 among them)
There is no LDS-staged variant."""
import threading

import numpy as np
import pytest

from conftest import gist_like

pytestmark = pytest.mark.gpu

DISTS = (("l2sqr", 0), ("cosine", 1))
FSTATS = ("flat_filtered_queries", "flat_filtered_direct_queries", "flat_filtered_i8_queries", "flat_filtered_fallback_queries",
          "flat_filtered_multi_calls", "flat_filtered_grouped_queries")


# (copies of the helpers of tests/test_flat_filtered_gpu.py)
def _full_order(base, qs, kind):
    """(ids, distances) of every row per query in the reference's order (NaN distances last)"""
    from oracle import oracle as O

    oi, od, oc = O.flat_knn_batch(base, qs, len(base), kind, nthreads=16)
    assert (oc == len(base)).all()
    return oi.astype(np.uint64), od


def _allow(n, ids):
    a = np.zeros(n, dtype=np.bool_)
    a[np.asarray(ids, dtype=np.int64)] = True
    return a


def _expect_knn(full, allow, k, id_offset=0):
    """[nq][k] ids / distances / counts: the first k allowed pairs of the full order, zero past the count"""
    oi, od = full
    nq = len(oi)
    idx = np.zeros((nq, k), dtype=np.uint64)
    dist = np.zeros((nq, k), dtype=np.float32)
    cnt = np.zeros(nq, dtype=np.uint64)
    for q in range(nq):
        keep = allow[oi[q].astype(np.int64)]
        c = min(k, int(keep.sum()))
        idx[q, :c] = oi[q][keep][:c] + np.uint64(id_offset)
        dist[q, :c] = od[q][keep][:c]
        cnt[q] = c
    return idx, dist, cnt


def _same_knn(got, exp, what=""):
    gi, gd, gc = got
    ei, ed, ec = exp
    assert np.array_equal(gc, ec), (what, gc, ec)
    assert np.array_equal(gi, ei), what
    assert gd.dtype == np.float32 and np.array_equal(np.isnan(gd), np.isnan(ed)), what  # (a NaN's payload is not part of the contract)
    ok = ~np.isnan(ed)
    assert np.array_equal(gd[ok].view(np.uint32), ed[ok].view(np.uint32)), what


def _expect_multi(full, allows, mask_of, k, id_offset=0):
    """_expect_knn with the allow-list of every query's own mask"""
    oi, od = full
    nq = len(oi)
    idx = np.zeros((nq, k), dtype=np.uint64)
    dist = np.zeros((nq, k), dtype=np.float32)
    cnt = np.zeros(nq, dtype=np.uint64)
    for q in range(nq):
        i1, d1, c1 = _expect_knn((oi[q:q + 1], od[q:q + 1]), allows[int(mask_of[q])], k, id_offset)
        idx[q], dist[q], cnt[q] = i1[0], d1[0], c1[0]
    return idx, dist, cnt


def _loop(ix, qs, k, masks, mask_of):
    """the batch as a loop of single-mask calls, one per mask that has queries"""
    kk = int(k)
    idx = np.zeros((len(qs), kk), dtype=np.uint64)
    dist = np.zeros((len(qs), kk), dtype=np.float32)
    cnt = np.zeros(len(qs), dtype=np.uint64)
    mask_of = np.asarray(mask_of)
    for g in np.unique(mask_of):
        sel = np.flatnonzero(mask_of == g)
        i1, d1, c1 = ix.flat_knn_filtered(qs[sel], k, masks[int(g)])
        idx[sel], dist[sel], cnt[sel] = i1, d1, c1
    return idx, dist, cnt


def _interleave(sizes):
    """mask_of with bucket g holding sizes[g] queries, round-robin over the buckets (not sorted), then rotated"""
    out = [g for r in range(max(sizes)) for g in range(len(sizes)) if r < sizes[g]]
    return np.array(out[3:] + out[:3], dtype=np.uint32)


def _stats(ix, names=FSTATS):
    return {s: ix.get_stat(s) for s in names}


def _delta(ix, s0, names=FSTATS):
    s1 = _stats(ix, names)
    return {s: s1[s] - s0[s] for s in names}


def _index(dist, base, mode=None):
    import lab_1806_vec_db_amd as vdb

    ix = vdb.GpuIndex(base.shape[1], dist)
    ix.batch_add(base)
    if mode is not None:
        ix.set_flat_mode(mode)
    return ix


# ---- 1. grouped path --------------------------------------------------------------------------------------------------------------------
N_SMALL = 3000


@pytest.fixture(scope="module")
def small():
    """3000 x 960 gist-like rows with rows 10 and 2000 equal, 40 queries, both metrics' full orders"""
    base = gist_like(N_SMALL, seed=3101)
    base[2000] = base[10]
    qs = gist_like(40, seed=3102)
    qs[5] = base[10]  # a query AT the duplicated row: ids 10 and 2000 tie at the top
    return base, qs, {kind: _full_order(base, qs, kind) for _, kind in DISTS}


def _small_allows():
    rng = np.random.default_rng(41)
    n = N_SMALL

    def pick(m):
        return _allow(n, rng.choice(n, m, replace=False)) if m else np.zeros(n, dtype=np.bool_)

    a = [pick(0), pick(1), pick(255), pick(256), pick(257), pick(700), np.ones(n, dtype=np.bool_)]
    ov1 = _allow(n, np.concatenate([[10, 2000], np.arange(500, 900)]))
    ov2 = _allow(n, np.concatenate([[10, 2000], np.arange(700, 1300)]))
    return a + [ov1, ov2]  # m = 0, 1, 255, 256, 257, 700, 3000, 402, 602


# which masks hold the buckets of 1, 7, 8, 9 and 15 queries: both assignments together give every mask queries
ASSIGN = ((0, 1, 2, 3, 4), (8, 7, 6, 5, 4))
SIZES = (1, 7, 8, 9, 15)


def _assignment(a):
    mo = _interleave(SIZES)
    return np.array([ASSIGN[a][g] for g in mo], dtype=np.uint32)


@pytest.mark.parametrize("dist,kind", DISTS)
def test_grouped_path(small, dist, kind):
    base, qs, fulls = small
    full = fulls[kind]
    allows = _small_allows()
    ix = _index(dist, base)
    try:
        masks = [ix.make_mask(a) for a in allows]
        assert [len(m) for m in masks] == [0, 1, 255, 256, 257, 700, 3000, 402, 602]
        ix.prof_enable(True)
        for a in (0, 1):
            mask_of = _assignment(a)
            assert len(mask_of) == 40 and sorted(np.bincount(mask_of)[np.bincount(mask_of) > 0]) == sorted(SIZES)
            assert (np.diff(mask_of.astype(np.int64)) < 0).any()  # not sorted
            nonempty = int(sum(len(masks[int(g)]) > 0 for g in mask_of))
            for k in (1, 10, 300):
                ix.prof_reset()
                s0 = _stats(ix)
                got = ix.flat_knn_filtered_multi(qs, k, masks, mask_of)
                d = _delta(ix, s0)
                _same_knn(got, _expect_multi(full, allows, mask_of, k), (dist, a, k))
                assert np.array_equal(got[2], np.minimum(k, [len(masks[int(g)]) for g in mask_of]).astype(np.uint64))
                for q in range(40):
                    assert not got[0][q, int(got[2][q]):].any() and not got[1][q, int(got[2][q]):].any()
                # ONE launch of the grouped kernel serves all buckets; the per-mask scan is never launched
                assert ix.prof_get("flat_filtered_scan_grouped")["launches"] == 1, ix.prof_get("flat_filtered_scan_grouped")
                assert ix.prof_get("flat_filtered_scan")["launches"] == 0
                assert d["flat_filtered_multi_calls"] == 1 and d["flat_filtered_grouped_queries"] >= nonempty, d
                assert d["flat_filtered_queries"] == 40 and d["flat_filtered_direct_queries"] == 40 and d["flat_filtered_i8_queries"] == 0, d
                _same_knn(got, _loop(ix, qs, k, masks, mask_of), (dist, a, k, "vs loop"))
        # the tie: query 5 IS rows 10 and 2000; under both overlapping masks they come first, in id order
        mask_of = _assignment(1)
        mask_of[5] = 7
        mask_of[6] = 8
        got = ix.flat_knn_filtered_multi(qs, 10, masks, mask_of)
        _same_knn(got, _expect_multi(full, allows, mask_of, 10), "tie")
        assert list(got[0][5, :2]) == [10, 2000] and got[1][5, 0].view(np.uint32) == got[1][5, 1].view(np.uint32)
        # one query
        gi, gd = ix.flat_knn_filtered_multi(qs[7], 10, masks, [5])
        ei, ed, ec = _expect_knn((full[0][7:8], full[1][7:8]), allows[5], 10)
        assert np.array_equal(gi, ei[0]) and np.array_equal(gd.view(np.uint32), ed[0].view(np.uint32))
        for m in masks:
            m.close()
    finally:
        ix.close()


def test_grouped_path_id_offset(small):
    base, qs, fulls = small
    allows = _small_allows()
    ix = _index("l2sqr", base)
    try:
        ix.set_id_offset(10**6)
        masks = [ix.make_mask(a) for a in allows]
        mask_of = _assignment(1)
        _same_knn(ix.flat_knn_filtered_multi(qs, 10, masks, mask_of), _expect_multi(fulls[0], allows, mask_of, 10, id_offset=10**6), "id offset")
        for m in masks:
            m.close()
    finally:
        ix.close()


# ---- 2. odd dimensions ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", (21, 100))  # 21: the element-by-element fold; 100: the float4 fold at a dim that is no multiple of 32
@pytest.mark.parametrize("dist,kind", DISTS)
def test_odd_dimensions(dim, dist, kind):
    rng = np.random.default_rng(50 + dim)
    base = rng.standard_normal((3000, dim)).astype(np.float32)
    qs = rng.standard_normal((9, dim)).astype(np.float32)
    full = _full_order(base, qs, kind)
    allows = [_allow(3000, rng.choice(3000, 300, replace=False)), _allow(3000, rng.choice(3000, 257, replace=False))]
    mask_of = np.array([0, 1, 1, 0, 1, 0, 1, 0, 1], dtype=np.uint32)  # buckets of 4 and 5
    ix = _index(dist, base)
    try:
        masks = [ix.make_mask(a) for a in allows]
        ix.prof_enable(True)
        for k in (1, 10, 280):
            got = ix.flat_knn_filtered_multi(qs, k, masks, mask_of)
            _same_knn(got, _expect_multi(full, allows, mask_of, k), (dim, dist, k))
        assert ix.prof_get("flat_filtered_scan_grouped")["launches"] == 3 and ix.prof_get("flat_filtered_scan")["launches"] == 0
        for m in masks:
            m.close()
    finally:
        ix.close()


# ---- 3. mixed routing -------------------------------------------------------------------------------------------------------------------
NB = 30000


@pytest.fixture(scope="module")
def big():
    """30 000 x 960 gist-like rows, 64 queries, both metrics' full orders"""
    base = gist_like(NB, seed=3201)
    qs = gist_like(64, seed=3202)
    return base, qs, {kind: _full_order(base, qs, kind) for _, kind in DISTS}


@pytest.mark.parametrize("dist,kind", DISTS)
def test_mixed_routing(big, dist, kind):
    base, qs, fulls = big
    full = fulls[kind]
    rng = np.random.default_rng(60)
    allows = [_allow(NB, rng.choice(NB, m, replace=False)) for m in (100, 512, 513, 10000)] + [np.ones(NB, dtype=np.bool_)]
    mask_of = _interleave((11, 13, 12, 14, 14))  # 64 queries: 24 on the grouped path, 40 on the three long masks
    assert len(mask_of) == 64
    n_long = int((mask_of >= 2).sum())
    exp = _expect_multi(full, allows, mask_of, 10)
    ix = _index(dist, base, 2)
    try:
        ix.set_param("flat_filtered_direct_max", 512)
        masks = [ix.make_mask(a) for a in allows]
        s0 = _stats(ix)
        got = ix.flat_knn_filtered_multi(qs, 10, masks, mask_of)
        d = _delta(ix, s0)
        print(dist, d)
        _same_knn(got, exp, (dist, "mode 2"))
        assert d["flat_filtered_i8_queries"] == n_long == 40, d
        assert d["flat_filtered_grouped_queries"] == 64 - n_long and d["flat_filtered_queries"] == 64, d
        _same_knn(got, _loop(ix, qs, 10, masks, mask_of), (dist, "mode 2 vs loop"))
        ix.set_flat_mode(1)
        s0 = _stats(ix)
        got1 = ix.flat_knn_filtered_multi(qs, 10, masks, mask_of)
        d = _delta(ix, s0)
        _same_knn(got1, exp, (dist, "mode 1"))
        _same_knn(got1, got, (dist, "mode 1 vs mode 2"))
        assert d["flat_filtered_i8_queries"] == 0 and d["flat_filtered_direct_queries"] == 64, d
        for m in masks:
            m.close()
    finally:
        ix.close()


# ---- 4. k beyond the register-resident select ---------------------------------------------------------------------------------------------
def test_k_1500_takes_the_per_mask_route(small):
    base, qs, fulls = small
    allows = _small_allows()
    allows = [allows[6], allows[5]]  # m = 3000, 700
    mask_of = np.array([0, 1] * 6 + [1], dtype=np.uint32)
    ix = _index("l2sqr", base)
    try:
        masks = [ix.make_mask(a) for a in allows]
        s0 = _stats(ix)
        got = ix.flat_knn_filtered_multi(qs[:13], 1500, masks, mask_of)
        d = _delta(ix, s0)
        full = (fulls[0][0][:13], fulls[0][1][:13])
        _same_knn(got, _expect_multi(full, allows, mask_of, 1500), "k = 1500")
        assert got[2].tolist() == [1500, 700] * 6 + [700]
        assert d["flat_filtered_grouped_queries"] == 0 and d["flat_filtered_direct_queries"] == 13, d
        for m in masks:
            m.close()
    finally:
        ix.close()


# ---- 5. property test without the oracle --------------------------------------------------------------------------------------------------
def test_property_multi_equals_loop():
    import torch

    rng = np.random.default_rng(70)
    n, dim, nq, k = 5000, 64, 200, 10
    base = rng.standard_normal((n, dim)).astype(np.float32)
    qs = rng.standard_normal((nq, dim)).astype(np.float32)
    ms = rng.integers(0, 601, 50)
    ms[:3] = (0, 600, 1)
    allows = [_allow(n, rng.choice(n, int(m), replace=False)) if m else np.zeros(n, dtype=np.bool_) for m in ms]
    mask_of = rng.integers(0, 50, nq).astype(np.uint32)
    ix = _index("l2sqr", base)
    try:
        masks = [ix.make_mask(a) for a in allows]
        got = ix.flat_knn_filtered_multi(qs, k, masks, mask_of)
        _same_knn(got, _loop(ix, qs, k, masks, mask_of), "multi vs loop")
        assert np.array_equal(got[2], np.minimum(k, ms[mask_of]).astype(np.uint64))
        # the device form through torch tensors
        tq = torch.from_numpy(qs).cuda()
        ti = torch.full((nq, k), -1, dtype=torch.int64, device="cuda")
        td = torch.full((nq, k), -1.0, dtype=torch.float32, device="cuda")
        tc = torch.full((nq,), -1, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        ix.flat_knn_filtered_multi_device(tq.data_ptr(), nq, k, masks, mask_of, ti.data_ptr(), td.data_ptr(), tc.data_ptr())
        dev = (ti.cpu().numpy().astype(np.uint64), td.cpu().numpy(), tc.cpu().numpy().astype(np.uint64))
        _same_knn(dev, got, "device form vs host form")
        for m in masks:
            m.close()
    finally:
        ix.close()


# ---- 6. errors, empty calls, two threads ----------------------------------------------------------------------------------------------------
def test_errors_leave_the_outputs_untouched(small):
    import lab_1806_vec_db_amd as vdb
    from lab_1806_vec_db_amd import _lib as L

    base, qs, _ = small
    qs = np.ascontiguousarray(qs[:6])
    ix, other = _index("l2sqr", base[:500]), _index("l2sqr", base[:500])

    def raw(masks, mask_of):
        """the C call with sentinel-filled outputs -> (return code, outputs)"""
        idx = np.full((6, 5), 0xABABABABABABABAB, dtype=np.uint64)
        dist = np.full((6, 5), -7.0, dtype=np.float32)
        cnt = np.full(6, 0xCDCDCDCD, dtype=np.uint64)
        arr = (L.vp * len(masks))(*[m._h for m in masks])
        mo = np.asarray(mask_of, dtype=np.uint32)
        rc = ix._lib.vdb_flat_knn_filtered_multi(ix._h, qs.ctypes.data_as(L.f32p), 6, 960, 5, arr, len(masks), mo.ctypes.data_as(L.u32p),
                                                 idx.ctypes.data_as(L.u64p), dist.ctypes.data_as(L.f32p), cnt.ctypes.data_as(L.u64p))
        untouched = (idx == 0xABABABABABABABAB).all() and (dist == -7.0).all() and (cnt == 0xCDCDCDCD).all()
        return rc, untouched

    try:
        good = ix.make_mask(np.ones(500, dtype=np.bool_))
        foreign = other.make_mask(np.ones(500, dtype=np.bool_))
        assert raw([good], [0] * 6) == (0, False)
        # a mask of another index, even one no query uses
        assert raw([good, foreign], [0] * 6) == (1, True)
        with pytest.raises(vdb.VdbError, match="error 1.*another index"):
            ix.flat_knn_filtered_multi(qs, 5, [good, foreign], [0] * 6)
        # mask_of out of range
        assert raw([good], [0, 0, 1, 0, 0, 0]) == (1, True)
        with pytest.raises(vdb.VdbError, match="error 1.*mask_of"):
            ix.flat_knn_filtered_multi(qs, 5, [good], [0, 0, 1, 0, 0, 0])
        with pytest.raises(vdb.VdbError, match="error 1"):
            ix.flat_knn_filtered_multi(qs, 5, [], [0] * 6)
        # empty calls
        gi, gd, gc = ix.flat_knn_filtered_multi(qs, 0, [good], [0] * 6)
        assert gi.shape == (6, 0) and gd.shape == (6, 0) and not gc.any()
        gi, gd, gc = ix.flat_knn_filtered_multi(qs[:0], 5, [good], [])
        assert gi.shape == (0, 5) and gc.shape == (0,)
        gi, gd, gc = ix.flat_knn_filtered_multi(qs[:0], 5, [], [])
        assert gi.shape == (0, 5) and gc.shape == (0,)
        # a mask made before a batch_add is stale
        ix.batch_add(base[500:510])
        fresh = ix.make_mask(np.ones(510, dtype=np.bool_))
        assert raw([fresh, good], [0] * 6) == (3, True)
        with pytest.raises(vdb.VdbError, match="error 3.*stale"):
            ix.flat_knn_filtered_multi(qs, 5, [fresh, good], [0] * 6)
        with pytest.raises(vdb.VdbError, match="error 3.*stale"):  # ... also in a call without queries
            ix.flat_knn_filtered_multi(qs[:0], 5, [fresh, good], [])
        assert raw([fresh], [0] * 6) == (0, False)
        for m in (good, foreign, fresh):
            m.close()
    finally:
        ix.close()
        other.close()
    u8 = vdb.GpuIndex(64, "l2sqr", scalar="u8")
    try:
        u8.batch_add_u8(np.random.default_rng(1).integers(0, 256, (100, 64), dtype=np.uint8))
        mk = u8.make_mask(np.ones(100, dtype=np.bool_))
        with pytest.raises(vdb.VdbError, match="error 1.*f32 rows"):
            u8.flat_knn_filtered_multi(np.zeros((2, 64), dtype=np.float32), 5, [mk], [0, 0])
        mk.close()
    finally:
        u8.close()


def test_two_threads_agree_with_the_serial_answer(small):
    base, qs, fulls = small
    allows = _small_allows()
    mask_of = _assignment(1)
    ix = _index("l2sqr", base)
    try:
        masks = [ix.make_mask(a) for a in allows]
        serial = ix.flat_knn_filtered_multi(qs, 10, masks, mask_of)
        _same_knn(serial, _expect_multi(fulls[0], allows, mask_of, 10), "serial")
        out, errs = [None] * 2, []
        bar = threading.Barrier(2)

        def work(t):
            try:
                bar.wait()
                for _ in range(3):
                    out[t] = ix.flat_knn_filtered_multi(qs, 10, masks, mask_of)
            except Exception as e:  # noqa: BLE001
                errs.append(e)

        ths = [threading.Thread(target=work, args=(t,)) for t in range(2)]
        for th in ths:
            th.start()
        for th in ths:
            th.join()
        assert not errs, errs
        for t in range(2):
            _same_knn(out[t], serial, ("thread", t))
        for m in masks:
            m.close()
    finally:
        ix.close()
