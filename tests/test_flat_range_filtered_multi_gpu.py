"""GPU: exact filtered Flat RANGE search with ONE ROW MASK PER QUERY (GpuIndex.range_search_multi) against the CPU oracle.

The expected slice of query q comes from the oracle as tests/test_flat_filtered_gpu.py derives it: oracle.flat_knn_batch(base, qs,
len(base), kind) -- every row in the reference's (distance, index) order -- keeping the pairs whose id masks[mask_of[q]] allows and
whose distance is <= the query's radius, and taking the first `limit`.  Every comparison is bit-exact: lims equal, ids equal, distances
equal as f32 bit patterns.  "Equals the loop of range_search(mask=...) calls" is an additional comparison wherever it is made, never the
only one -- except in the property test, which has no oracle by design.

Variants of the grouped kernel (k_range_gather_grouped) and the case that reaches each:
  float4 fold (dim % 4 == 0), L2 and dot   -- test_grouped_path (dim 960), test_odd_dimensions[100]
  element fold (dim % 4 != 0), L2 and dot  -- test_odd_dimensions[21]
  query groups of nb = 1 .. 8              -- test_grouped_path: buckets of 1, 7, 8, 9 (8 + 1) and 15 (8 + 7); test_odd_dimensions: buckets
                                              of 4 and 5; test_property_multi_equals_loop: random bucket sizes
  a last tile that is not full             -- m = 1, 255, 257, 700 (test_grouped_path)"""
import threading

import numpy as np
import pytest

from conftest import gist_like

pytestmark = pytest.mark.gpu

DISTS = (("l2sqr", 0), ("cosine", 1))
RSTATS = ("flat_range_queries", "flat_range_i8_queries", "flat_range_scan_queries", "flat_range_hits", "flat_range_results",
          "flat_range_multi_calls", "flat_range_grouped_queries")
INF = np.float32(np.inf)


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


def _expect_range(full, allow, radii, limit=None):
    oi, od = full
    lims, ids, ds = [0], [], []
    for q in range(len(oi)):
        keep = allow[oi[q].astype(np.int64)]
        fi, fd = oi[q][keep], od[q][keep]
        with np.errstate(invalid="ignore"):
            inside = fd <= np.float32(radii[q])
        cut = int(inside.sum())
        assert inside[:cut].all()
        if limit is not None:
            cut = min(cut, limit)
        ids.append(fi[:cut])
        ds.append(fd[:cut])
        lims.append(lims[-1] + cut)
    return np.array(lims, dtype=np.uint64), np.concatenate(ids), np.concatenate(ds)


def _same_range(got, exp, what=""):
    gl, gi, gd = got
    el, ei, ed = exp
    assert np.array_equal(gl, el), (what, gl, el)
    assert np.array_equal(gi, ei), what
    assert gd.dtype == np.float32 and np.array_equal(gd.view(np.uint32), ed.astype(np.float32).view(np.uint32)), what


def _expect_multi(full, allows, mask_of, radii, limit=None, id_offset=0):
    """_expect_range with the allow-list of every query's own mask"""
    oi, od = full
    lims, ids, ds = [0], [], []
    for q in range(len(oi)):
        _, i1, d1 = _expect_range((oi[q:q + 1], od[q:q + 1]), allows[int(mask_of[q])], radii[q:q + 1], limit)
        ids.append(i1 + np.uint64(id_offset))
        ds.append(d1)
        lims.append(lims[-1] + len(i1))
    return np.array(lims, dtype=np.uint64), np.concatenate(ids).astype(np.uint64), np.concatenate(ds).astype(np.float32)


def _allowed_dists(full, allows, mask_of, q):
    """the distances of query q's allowed rows in the reference's order"""
    oi, od = full
    return od[q][allows[int(mask_of[q])][oi[q].astype(np.int64)]]


def _radii_jth(full, allows, mask_of, j):
    """per query its own j-th allowed distance; +inf where its mask has fewer than j rows (then all m rows are inside)"""
    r = np.full(len(mask_of), INF, dtype=np.float32)
    for q in range(len(mask_of)):
        d = _allowed_dists(full, allows, mask_of, q)
        if len(d) >= j and not np.isnan(d[j - 1]):
            r[q] = d[j - 1]
    return r


def _loop(ix, qs, radii, masks, mask_of, limit=None):
    """the batch as a loop of single-mask calls, one per query"""
    lims, ids, ds = [0], [np.zeros(0, dtype=np.uint64)], [np.zeros(0, dtype=np.float32)]
    for q in range(len(qs)):
        _, i1, d1 = ix.range_search(qs[q], radii[q], limit, mask=masks[int(mask_of[q])])
        ids.append(i1)
        ds.append(d1)
        lims.append(lims[-1] + len(i1))
    return np.array(lims, dtype=np.uint64), np.concatenate(ids), np.concatenate(ds)


def _interleave(sizes):
    """mask_of with bucket g holding sizes[g] queries, round-robin over the buckets (not sorted), then rotated"""
    out = [g for r in range(max(sizes)) for g in range(len(sizes)) if r < sizes[g]]
    return np.array(out[3:] + out[:3], dtype=np.uint32)


def _stats(ix, names=RSTATS):
    return {s: ix.get_stat(s) for s in names}


def _delta(ix, s0, names=RSTATS):
    s1 = _stats(ix, names)
    return {s: s1[s] - s0[s] for s in names}


def _index(dist, base, mode=None):
    import lab_1806_vec_db_amd as vdb

    ix = vdb.GpuIndex(base.shape[1], dist)
    ix.batch_add(base)
    if mode is not None:
        ix.set_flat_mode(mode)
    return ix


def _counts(lims):
    return np.diff(lims.astype(np.int64))


# ---- 1. grouped path --------------------------------------------------------------------------------------------------------------------
N_SMALL = 3000


@pytest.fixture(scope="module")
def small():
    """3000 x 960 gist-like rows with rows 10 and 2000 equal, 40 queries, both metrics' full orders"""
    base = gist_like(N_SMALL, seed=3101)
    base[2000] = base[10]
    qs = gist_like(40, seed=3102)
    qs[5] = base[10]  # a query AT the duplicated row: ids 10 and 2000 tie at distance zero
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


def _check_grouped_call(ix, qs, full, allows, masks, mask_of, radii, limit, what, id_offset=0):
    """one multi call against the oracle and the loop; all of it on the grouped path"""
    s0 = _stats(ix)
    got = ix.range_search_multi(qs, radii, masks, mask_of, limit)
    d = _delta(ix, s0)
    exp = _expect_multi(full, allows, mask_of, radii, limit, id_offset)
    _same_range(got, exp, what)
    assert d["flat_range_multi_calls"] == 1 and d["flat_range_queries"] == len(qs) and d["flat_range_grouped_queries"] == len(qs), (what, d)
    assert d["flat_range_i8_queries"] == 0 and d["flat_range_scan_queries"] == 0 and d["flat_range_results"] == int(exp[0][-1]), (what, d)
    _same_range(got, _loop(ix, qs, radii, masks, mask_of, limit), (what, "vs loop"))
    return got


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
            ms = np.array([len(masks[int(g)]) for g in mask_of])
            # the query's own j-th allowed distance: the boundary is inclusive, so at least j rows (all m where the mask is shorter)
            for j in (1, 10, 64):
                radii = _radii_jth(full, allows, mask_of, j)
                ix.prof_reset()
                got = _check_grouped_call(ix, qs, full, allows, masks, mask_of, radii, None, (dist, a, j))
                # ONE launch of the grouped kernel serves all buckets (the loop that follows launches none)
                assert ix.prof_get("flat_range_gather_grouped")["launches"] == 1, ix.prof_get("flat_range_gather_grouped")
                assert (_counts(got[0]) >= np.minimum(j, ms)).all(), (dist, a, j)
                assert (_counts(got[0])[radii == INF] == ms[radii == INF]).all()  # +inf: every row of a short mask
            # limits, and the radii just below the 10th allowed distance: the count must drop below 10
            r10 = _radii_jth(full, allows, mask_of, 10)
            for limit in (1, 5):
                got = _check_grouped_call(ix, qs, full, allows, masks, mask_of, r10, limit, (dist, a, "limit", limit))
                assert (_counts(got[0]) == np.minimum(limit, ms)).all()
            below = np.where(np.isfinite(r10), np.nextafter(r10, -INF), r10).astype(np.float32)
            got = _check_grouped_call(ix, qs, full, allows, masks, mask_of, below, None, (dist, a, "below the 10th"))
            assert (_counts(got[0])[np.isfinite(r10)] < 10).all()
            # NaN and -1 radii give empty slices, +inf on a short mask every one of its rows
            special = r10.copy()
            special[0], special[1], special[2] = np.float32(np.nan), np.float32(-1.0), INF
            got = _check_grouped_call(ix, qs, full, allows, masks, mask_of, special, None, (dist, a, "NaN, -1, +inf"))
            c = _counts(got[0])
            assert c[0] == 0 and c[1] == 0 and c[2] == ms[2]
        # the tie: query 5 IS rows 10 and 2000; under both overlapping masks they come first, in id order
        mask_of = _assignment(1)
        mask_of[5] = 7
        mask_of[6] = 8
        radii = _radii_jth(full, allows, mask_of, 1)
        got = _check_grouped_call(ix, qs, full, allows, masks, mask_of, radii, None, "tie")
        l5 = int(got[0][5])
        assert int(got[0][6]) - l5 == 2 and list(got[1][l5:l5 + 2]) == [10, 2000]
        assert got[2][l5].view(np.uint32) == got[2][l5 + 1].view(np.uint32)
        # one radius for all queries, one query
        r = np.float32(np.median(r10[np.isfinite(r10)]))
        _same_range(ix.range_search_multi(qs, r, masks, mask_of), _expect_multi(full, allows, mask_of, np.full(40, r, dtype=np.float32)), "scalar")
        _same_range(ix.range_search_multi(qs[7], r, masks, [5]), _expect_range((full[0][7:8], full[1][7:8]), allows[5], [r]), "one query")
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
        radii = _radii_jth(fulls[0], allows, mask_of, 10)
        for limit in (None, 5):
            got = ix.range_search_multi(qs, radii, masks, mask_of, limit)
            _same_range(got, _expect_multi(fulls[0], allows, mask_of, radii, limit, id_offset=10**6), ("id offset", limit))
        for m in masks:
            m.close()
    finally:
        ix.close()


# ---- 2. odd dimensions ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", (21, 100))  # 21: the element-by-element fold; 100: the float4 fold at a dim that is no multiple of 32
@pytest.mark.parametrize("dist,kind", DISTS)
def test_odd_dimensions(dim, dist, kind):
    rng = np.random.default_rng(50 + dim)
    base = rng.standard_normal((2000, dim)).astype(np.float32)
    qs = rng.standard_normal((9, dim)).astype(np.float32)
    full = _full_order(base, qs, kind)
    allows = [_allow(2000, rng.choice(2000, 300, replace=False)), _allow(2000, rng.choice(2000, 257, replace=False))]
    mask_of = np.array([0, 1, 1, 0, 1, 0, 1, 0, 1], dtype=np.uint32)  # buckets of 4 and 5
    ix = _index(dist, base)
    try:
        masks = [ix.make_mask(a) for a in allows]
        for j, limit in ((1, None), (10, None), (64, None), (64, 5), (257, None)):
            radii = _radii_jth(full, allows, mask_of, j)
            got = _check_grouped_call(ix, qs, full, allows, masks, mask_of, radii, limit, (dim, dist, j, limit))
            if limit is None:
                assert (_counts(got[0]) >= j).all()
        for m in masks:
            m.close()
    finally:
        ix.close()


# ---- 3. NaN and zero rows -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dist,kind", DISTS)
def test_nan_and_zero_rows(dist, kind):
    rng = np.random.default_rng(77)
    n, dim = 600, 32
    base = rng.standard_normal((n, dim)).astype(np.float32)
    base[17, 3] = np.nan  # its distance to every query is NaN: never inside
    base[300] = 0.0       # Cosine: |x| = 0, the reference's distance is 1
    qs = rng.standard_normal((6, dim)).astype(np.float32)
    full = _full_order(base, qs, kind)
    allows = [_allow(n, np.concatenate([[17, 300], np.arange(100, 140)])), _allow(n, np.concatenate([[17, 300], np.arange(250, 520)]))]
    mask_of = np.array([0, 1, 1, 0, 1, 0], dtype=np.uint32)
    ix = _index(dist, base)
    try:
        masks = [ix.make_mask(a) for a in allows]
        ms = np.array([len(masks[int(g)]) for g in mask_of])
        got = _check_grouped_call(ix, qs, full, allows, masks, mask_of, np.full(6, INF, dtype=np.float32), None, (dist, "+inf"))
        assert (_counts(got[0]) == ms - 1).all() and 17 not in got[1].tolist() and (got[1] == 300).sum() == 6
        assert not np.isnan(got[2]).any()
        radii = _radii_jth(full, allows, mask_of, 20)
        got = _check_grouped_call(ix, qs, full, allows, masks, mask_of, radii, None, (dist, "20th"))
        assert 17 not in got[1].tolist()
        for m in masks:
            m.close()
    finally:
        ix.close()


# ---- 4. mixed routing -------------------------------------------------------------------------------------------------------------------
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
    radii = _radii_jth(full, allows, mask_of, 64)
    assert np.isfinite(radii).all()
    exp = _expect_multi(full, allows, mask_of, radii)
    assert (_counts(exp[0]) >= 64).all()
    ix = _index(dist, base, 2)
    try:
        ix.set_param("flat_filtered_direct_max", 512)
        masks = [ix.make_mask(a) for a in allows]
        s0 = _stats(ix)
        got = ix.range_search_multi(qs, radii, masks, mask_of)
        d = _delta(ix, s0)
        print(dist, d)
        _same_range(got, exp, (dist, "mode 2"))
        assert d["flat_range_grouped_queries"] == 64 - n_long == 24 and d["flat_range_queries"] == 64 and d["flat_range_multi_calls"] == 1, d
        assert d["flat_range_i8_queries"] + d["flat_range_scan_queries"] == n_long == 40, d
        assert d["flat_range_results"] == int(exp[0][-1]), d
        _same_range(got, _loop(ix, qs, radii, masks, mask_of), (dist, "mode 2 vs loop"))
        _same_range(ix.range_search_multi(qs, radii, masks, mask_of, 5), _expect_multi(full, allows, mask_of, radii, 5), (dist, "limit"))
        ix.set_flat_mode(1)
        s0 = _stats(ix)
        got1 = ix.range_search_multi(qs, radii, masks, mask_of)
        d = _delta(ix, s0)
        _same_range(got1, exp, (dist, "mode 1"))
        _same_range(got1, got, (dist, "mode 1 vs mode 2"))
        assert d["flat_range_i8_queries"] == 0 and d["flat_range_scan_queries"] == n_long and d["flat_range_grouped_queries"] == 24, d
        for m in masks:
            m.close()
    finally:
        ix.close()


# ---- 5. u8 index ------------------------------------------------------------------------------------------------------------------------
def test_u8_index_takes_the_per_mask_route():
    import lab_1806_vec_db_amd as vdb

    rng = np.random.default_rng(9)
    n = 2000
    rows = rng.integers(0, 256, (n, 64), dtype=np.uint8)
    qs = rng.integers(0, 256, (9, 64)).astype(np.float32)
    full = _full_order(rows.astype(np.float32), qs, 0)  # (the u8 distance is the f32 fold over the widened bytes)
    allows = [rng.random(n) < 0.4, _allow(n, rng.choice(n, 100, replace=False)), np.zeros(n, dtype=np.bool_)]
    mask_of = np.array([0, 1, 0, 2, 1, 0, 1, 0, 2], dtype=np.uint32)
    ix = vdb.GpuIndex(64, "l2sqr", scalar="u8")
    try:
        ix.batch_add_u8(rows)
        masks = [ix.make_mask(a) for a in allows]
        radii = _radii_jth(full, allows, mask_of, 64)
        for limit in (None, 7):
            s0 = _stats(ix)
            got = ix.range_search_multi(qs, radii, masks, mask_of, limit)
            d = _delta(ix, s0)
            _same_range(got, _expect_multi(full, allows, mask_of, radii, limit), ("u8", limit))
            assert d["flat_range_grouped_queries"] == 0 and d["flat_range_queries"] == 9 and d["flat_range_multi_calls"] == 1, d
            assert d["flat_range_i8_queries"] + d["flat_range_scan_queries"] == 9, d
            _same_range(got, _loop(ix, qs, radii, masks, mask_of, limit), ("u8 vs loop", limit))
        assert _counts(got[0])[3] == 0 and _counts(got[0])[8] == 0  # the empty mask
        for m in masks:
            m.close()
    finally:
        ix.close()


# ---- 6. property test without the oracle --------------------------------------------------------------------------------------------------
def test_property_multi_equals_loop():
    import torch

    rng = np.random.default_rng(70)
    for draw in range(20):
        n = int(rng.integers(1, 4001))
        dim = int(rng.choice((8, 21, 64)))
        dist = ("l2sqr", "cosine")[draw % 2]
        nq = int(rng.integers(1, 41))
        n_masks = int(rng.integers(1, 9))
        base = rng.standard_normal((n, dim)).astype(np.float32)
        qs = rng.standard_normal((nq, dim)).astype(np.float32)
        ms = rng.integers(0, min(n, 700) + 1, n_masks)
        allows = [_allow(n, rng.choice(n, int(m), replace=False)) if m else np.zeros(n, dtype=np.bool_) for m in ms]
        mask_of = rng.integers(0, n_masks, nq).astype(np.uint32)  # random bucket sizes, some masks without queries
        # radii around the distances the metric produces, with a NaN, a negative and a +inf one thrown in
        centre = 2.0 * dim if dist == "l2sqr" else 1.0
        radii = (centre * rng.uniform(0.5, 1.3, nq)).astype(np.float32)
        radii[rng.integers(0, nq)] = rng.choice(np.array([np.nan, -1.0, np.inf], dtype=np.float32))
        limit = None if draw % 3 == 0 else int(rng.integers(1, 30))
        ix = _index(dist, base)
        try:
            masks = [ix.make_mask(a) for a in allows]
            got = ix.range_search_multi(qs, radii, masks, mask_of, limit)
            _same_range(got, _loop(ix, qs, radii, masks, mask_of, limit), ("multi vs loop", draw, n, dim, dist, limit))
            if draw < 2:  # the device form through torch tensors
                tq, tr = torch.from_numpy(qs).cuda(), torch.from_numpy(radii).cuda()
                torch.cuda.synchronize()
                dev = ix.range_search_multi_device(tq.data_ptr(), nq, tr.data_ptr(), masks, mask_of, limit)
                _same_range(dev, got, ("device form vs host form", draw))
            for m in masks:
                m.close()
        finally:
            ix.close()


# ---- 7. errors, empty calls, two threads ----------------------------------------------------------------------------------------------------
def test_errors_return_nothing_and_leave_the_counters(small):
    import ctypes as C

    import lab_1806_vec_db_amd as vdb
    from lab_1806_vec_db_amd import _lib as L

    base, qs, fulls = small
    qs = np.ascontiguousarray(qs[:6])
    ix, other = _index("l2sqr", base[:500]), _index("l2sqr", base[:500])
    radii = np.full(6, INF, dtype=np.float32)

    def raw(masks, mask_of, dim=960):
        """the C call -> (return code, whether *out was left NULL, whether every counter is where it was)"""
        s0 = _stats(ix)
        h = L.vp(0xDEAD)
        arr = (L.vp * max(len(masks), 1))(*[m._h for m in masks])
        mo = np.asarray(mask_of, dtype=np.uint32)
        rc = ix._lib.vdb_flat_range_filtered_multi(ix._h, qs.ctypes.data_as(L.f32p), 6, dim, radii.ctypes.data_as(L.f32p), 0, arr, len(masks),
                                                   mo.ctypes.data_as(L.u32p), C.byref(h))
        null = not h.value
        if rc == 0:
            ix._lib.vdb_range_destroy(h)
        return rc, null, not any(_delta(ix, s0).values())

    def good_call(mk, n_rows):
        lims, idx, _ = ix.range_search_multi(qs, radii, [mk], [0] * 6)
        assert _counts(lims).tolist() == [n_rows] * 6 and sorted(idx[:n_rows].tolist()) == list(range(n_rows))

    try:
        good = ix.make_mask(np.ones(500, dtype=np.bool_))
        foreign = other.make_mask(np.ones(500, dtype=np.bool_))
        assert raw([good], [0] * 6) == (0, False, False)
        # a mask of another index, even one no query uses
        assert raw([good, foreign], [0] * 6) == (1, True, True)
        with pytest.raises(vdb.VdbError, match="error 1.*another index"):
            ix.range_search_multi(qs, radii, [good, foreign], [0] * 6)
        good_call(good, 500)
        # mask_of out of range
        assert raw([good], [0, 0, 1, 0, 0, 0]) == (1, True, True)
        with pytest.raises(vdb.VdbError, match="error 1.*mask_of"):
            ix.range_search_multi(qs, radii, [good], [0, 0, 1, 0, 0, 0])
        with pytest.raises(vdb.VdbError, match="error 1"):
            ix.range_search_multi(qs, radii, [], [0] * 6)
        good_call(good, 500)
        # a dim mismatch
        assert raw([good], [0] * 6, dim=959) == (1, True, True)
        with pytest.raises(vdb.VdbError, match="error 1.*dimension"):
            ix.range_search_multi(qs[:, :959], radii, [good], [0] * 6)
        good_call(good, 500)
        # flat_range_max_results below the result size: the whole call fails, nothing is returned, nothing was counted
        ix.set_param("flat_range_max_results", 2999)
        assert raw([good], [0] * 6) == (1, True, True)
        with pytest.raises(vdb.VdbError, match="error 1.*flat_range_max_results"):
            ix.range_search_multi(qs, radii, [good], [0] * 6)
        ix.set_param("flat_range_max_results", 3000)
        good_call(good, 500)
        ix.set_param("flat_range_max_results", 0)
        # ... and on the per-mask route (every mask is "long")
        ix.set_param("flat_filtered_direct_max", 0)
        ix.set_param("flat_range_max_results", 2999)
        assert raw([good], [0] * 6) == (1, True, True)
        ix.set_param("flat_range_max_results", 0)
        assert raw([good], [0] * 6) == (0, False, False)
        ix.set_param("flat_filtered_direct_max", 8192)
        # empty calls
        lims, idx, dist = ix.range_search_multi(qs[:0], radii[:0], [good], [])
        assert lims.tolist() == [0] and len(idx) == 0 and len(dist) == 0
        lims, idx, dist = ix.range_search_multi(qs[:0], radii[:0], [], [])
        assert lims.tolist() == [0] and len(idx) == 0
        # a mask made before a batch_add is stale
        ix.batch_add(base[500:510])
        fresh = ix.make_mask(np.ones(510, dtype=np.bool_))
        assert raw([fresh, good], [0] * 6) == (3, True, True)
        with pytest.raises(vdb.VdbError, match="error 3.*stale"):
            ix.range_search_multi(qs, radii, [fresh, good], [0] * 6)
        good_call(fresh, 510)
        for m in (good, foreign, fresh):
            m.close()
    finally:
        ix.close()
        other.close()


def test_two_threads_agree_with_the_serial_answer(small):
    base, qs, fulls = small
    allows = _small_allows()
    mask_of = _assignment(1)
    ix = _index("l2sqr", base)
    try:
        masks = [ix.make_mask(a) for a in allows]
        radii = _radii_jth(fulls[0], allows, mask_of, 64)
        serial = ix.range_search_multi(qs, radii, masks, mask_of)
        _same_range(serial, _expect_multi(fulls[0], allows, mask_of, radii), "serial")
        out, errs = [None] * 2, []
        bar = threading.Barrier(2)

        def work(t):
            try:
                bar.wait()
                for _ in range(3):
                    out[t] = ix.range_search_multi(qs, radii, masks, mask_of)
            except Exception as e:  # noqa: BLE001
                errs.append(e)

        ths = [threading.Thread(target=work, args=(t,)) for t in range(2)]
        for th in ths:
            th.start()
        for th in ths:
            th.join()
        assert not errs, errs
        for t in range(2):
            _same_range(out[t], serial, ("thread", t))
        for m in masks:
            m.close()
    finally:
        ix.close()
